"""Time the R2D2 dueling head kernels (ops/hip/r2d2_head.hip) against the
torch chain of R2D2LstmQ._head on the same tensors: N = 128 rows at H = 64
and N = 640 rows at H = 512 (A = 4), the no-grad window form (and the older
one-launch head where it takes the width) and forward + backward.

Each variant is REP back-to-back calls captured in a graph (GPU time only),
timed over 50 replays with device events, five times; a line shows min..max
of the five in microseconds per call.

Usage: python scripts/r2d2_head_sweep.py
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_reinforcement_learning_amd import ops  # noqa: E402

A, REP, BURN, W = 4, 20, 7, 8
torch.manual_seed(0)


def timed(fn, label):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            fn()
    for _ in range(5):
        g.replay()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(50):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / (50 * REP))
    print(f"{label}: {min(ts):.1f}..{max(ts):.1f} us", flush=True)


for N, H in ((128, 64), (640, 512)):
    trunk = nn.Linear(H, 128).cuda().bfloat16()
    out = nn.Linear(128, A + 1).cuda().bfloat16()
    params = [*trunk.parameters(), *out.parameters()]

    def lib(h):
        y = out(F.relu(trunk(h.to(torch.bfloat16))))
        return y[..., :A] - y[..., A:]

    B = N // W
    h_all = torch.randn(B, BURN + W, H, device="cuda")
    dq = torch.randn(B, W, A, device="cuda").bfloat16()
    tag = f"N={N} H={H}"
    with torch.no_grad():
        timed(lambda: ops.r2d2_head(h_all, trunk, out, BURN),
              f"custom no-grad window {tag}")
        timed(lambda: lib(h_all[:, BURN:]), f"library no-grad window {tag}")
        if H <= 256:
            ext = ops.require_ext()
            timed(lambda: ext.dueling_head_fwd(h_all, *params, BURN),
                  f"older one-launch head {tag}")
    hg = h_all[:, BURN:].contiguous().requires_grad_()

    def train(f):
        torch.autograd.grad(f(hg), [hg] + params, dq)

    timed(lambda: ops.r2d2_head(hg, trunk, out), f"custom fwd train {tag}")
    timed(lambda: train(lambda h: ops.r2d2_head(h, trunk, out)),
          f"custom fwd+bwd {tag}")
    timed(lambda: lib(hg), f"library fwd train {tag}")
    timed(lambda: train(lib), f"library fwd+bwd {tag}")
