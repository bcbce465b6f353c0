"""Time the R2D2 LSTM projection kernels (ops/hip/lstm_proj.hip) against the
torch chain of R2D2LstmQ on the same tensors, each direction alone, at
(M, H) = (128, 64), (640, 64), (1280, 64) and (640, 512) with the shipped
F1 = 3136, F2 = 256:

  forward   _lstm_proj_fwd            vs  cat, matmul, bias add
  dgrad     _lstm_proj_dgrad          vs  dxg @ W[:F]^T and its two slices
  wgrad     _lstm_proj_wgrad          vs  feat^T @ dxg, h_prev^T @ dxg, the
                                          column sum and the cat of the two
  --splits  also the forward at forced K-splits from 1 to 16 (the launcher's
            own choice is printed on the plain forward line)

Each variant is REP back-to-back calls captured in a graph (GPU time only),
timed over 50 replays with device events, five times; a line shows min..max
of the five in microseconds per call.

Usage: python scripts/lstm_proj_sweep.py [--splits]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_reinforcement_learning_amd import ops  # noqa: E402

F1, F2, REP = 3136, 256, 20
F = F1 + F2
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


ext = ops.require_ext()
with torch.no_grad():
    for M, H in ((128, 64), (640, 64), (1280, 64), (640, 512)):
        N = 4 * H
        mk = lambda *s: (torch.randn(*s, device="cuda") * 0.1).bfloat16()
        conv, emb, w, b = mk(M, F1), mk(M, F2), mk(F + H, N), mk(N)
        hp, dxg = mk(M, H), mk(M, N)
        tag = f"M={M} H={H}"

        def lib_dgrad():
            d = dxg @ w[:F].t()
            return d[:, :F1].contiguous(), d[:, F1:].contiguous()

        def lib_wgrad():
            feat = torch.cat([conv, emb], 1)
            return (torch.cat([feat.t() @ dxg, hp.t() @ dxg], 0),
                    dxg.sum(0, dtype=torch.float32).bfloat16())

        timed(lambda: ext._lstm_proj_fwd(conv, emb, w, b),
              f"custom forward {tag} "
              f"(split {ext._lstm_proj_split(M, F, N)})")
        timed(lambda: torch.cat([conv, emb], 1) @ w[:F] + b,
              f"library forward {tag}")
        timed(lambda: ext._lstm_proj_dgrad(dxg, w, F1, F2),
              f"custom dgrad {tag}")
        timed(lib_dgrad, f"library dgrad {tag}")
        timed(lambda: ext._lstm_proj_wgrad(conv, emb, hp, dxg),
              f"custom wgrad {tag}")
        timed(lib_wgrad, f"library wgrad {tag}")
        if "--splits" in sys.argv:
            for S in (1, 2, 3, 4, 6, 8, 10, 13, 16):
                timed(lambda: ext._lstm_proj_fwd(conv, emb, w, b, S),
                      f"custom forward {tag} split {S}")
