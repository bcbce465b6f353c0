"""Time the Ape-X dueling Q head kernels (ops/hip/dueling_q.hip) against the
library chain on the same tensors at the learner's shapes (K = 3392, A = 4):
the no-grad forward at N = 32, forward and forward + backward at N = 64 with
grad_rows 32 and 64, and the forward at every first-layer K-split.

Each variant is REP back-to-back calls captured in a graph (GPU time only),
timed over 50 replays with device events, five times; a line shows min..max
of the five in microseconds per call.

Usage: python scripts/dueling_q_sweep.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_reinforcement_learning_amd import ops  # noqa: E402
from distributed_reinforcement_learning_amd.models.blocks import (  # noqa: E402
    MLPHead,
)

K, A, REP = 3392, 4, 20
torch.manual_seed(0)
vb = MLPHead(K, [256, 256], A, None).cuda().bfloat16()
mb = MLPHead(K, [256, 256], 1, None).cuda().bfloat16()
params = [*vb.parameters(), *mb.parameters()]


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


def lib(feat):
    return vb(feat) - mb(feat)


for N, G in ((32, None), (64, 32), (64, 64)):
    feat = torch.randn(N, K, device="cuda").bfloat16()
    dq = torch.randn(N, A, device="cuda").bfloat16()
    if G is None:
        with torch.no_grad():
            timed(lambda: ops.dueling_q(feat, vb, mb), f"custom fwd no-grad N={N}")
            timed(lambda: lib(feat), f"library fwd no-grad N={N}")
        continue
    dq[G:] = 0
    fg = feat.clone().requires_grad_()

    def train(f):
        q = f()
        torch.autograd.grad(q, [fg] + params, dq)

    timed(lambda: ops.dueling_q(fg, vb, mb, G), f"custom fwd train N={N} G={G}")
    timed(lambda: train(lambda: ops.dueling_q(fg, vb, mb, G)),
          f"custom fwd+bwd N={N} G={G}")
    timed(lambda: lib(fg), f"library fwd train N={N}")
    timed(lambda: train(lambda: lib(fg)), f"library fwd+bwd N={N}")
ext = ops.require_ext()
feat = torch.randn(64, K, device="cuda").bfloat16()
pv, pm = list(vb.parameters()), list(mb.parameters())
with torch.no_grad():
    for S in (1, 2, 4, 6, 9, 13, 16):
        timed(lambda: ext._dq_head_fwd(feat, pv, pm, -1, S), f"fwd N=64 split {S}")
    f32 = feat[:32].contiguous()
    for S in (1, 2, 4, 6, 9, 13, 16):
        timed(lambda: ext._dq_head_fwd(f32, pv, pm, -1, S), f"fwd N=32 split {S}")
