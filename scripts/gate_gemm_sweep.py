"""Time the gate GEMM kernels against the library at the flagship shape
(M = 640, K = 3656, N = 1024): the forward at every K-split, dgrad (with and
without grad_cols) and wgrad.

Each variant is CALLS back-to-back launches captured in a graph (GPU time
only), timed over REPLAYS replays with device events, REPEATS times; the
table shows min and max of the repeats in microseconds per call. The tile
height (DRLA_GG_*_MT in drla_common.h) is a compile-time constant: to compare
heights, build each and run this script once per build, naming it in LABEL.

Usage: python scripts/gate_gemm_sweep.py [out.md] [LABEL]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_reinforcement_learning_amd import ops  # noqa: E402

M, K, N, GRAD_COLS = 640, 3656, 1024, 3392
CALLS, REPLAYS, REPEATS = 20, 10, 5


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        for _ in range(REPLAYS):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / (REPLAYS * CALLS) * 1000)
    return min(us), max(us)


def main():
    ext = ops.require_ext()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    label = sys.argv[2] if len(sys.argv) > 2 else "default build"
    torch.manual_seed(0)
    bf = dict(dtype=torch.bfloat16, device="cuda")
    xh = torch.randn(M, K, **bf)
    w = torch.randn(K, N, **bf) * 0.02
    dg = torch.randn(M, N, **bf)
    variants = [("fwd library", lambda: torch.mm(xh, w))]
    for s in (1, 2, 3, 4, 6, 8, 12, 16):
        variants.append((f"fwd custom S={s}",
                         lambda s=s: ext._gate_gemm_fwd(xh, w, s)))
    variants += [
        ("dgrad library", lambda: torch.mm(dg, w.t())),
        ("dgrad custom, all columns", lambda: ext._gate_gemm_dgrad(dg, w, K)),
        (f"dgrad custom, grad_cols={GRAD_COLS}",
         lambda: ext._gate_gemm_dgrad(dg, w, GRAD_COLS)),
        ("wgrad library", lambda: torch.mm(xh.t(), dg)),
        ("wgrad custom", lambda: ext._gate_gemm_wgrad(xh, dg)),
    ]
    lines = [f"Gate GEMM at M={M}, K={K}, N={N} ({label}; launcher rule "
             f"S={ext._gate_gemm_split(M, K, N)}); {CALLS} calls per graph, "
             f"{REPLAYS} replays per timing, min..max of {REPEATS} timings.",
             "", "| variant | min us | max us |", "|---|---|---|"]
    for name, fn in variants:
        lo, hi = timed(fn)
        lines.append(f"| {name} | {lo:.2f} | {hi:.2f} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
