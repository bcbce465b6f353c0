"""Sweep DRLA_WGRAD_SPLIT per conv layer at the flagship shape (N = 640).

The split is read once per process, so every value runs in a child process.
Each child captures CALLS back-to-back conv_wgrad launches of one layer in a
graph (GPU time only, no host launch cost) and times REPLAYS replays with
device events, REPEATS times; the table shows the min and max of the repeats
in microseconds per call, so a difference can be held against the spread.

Usage: python scripts/wgrad_sweep.py [out.md]
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = {0: [128, 192, 256, 384, 512, 768],
          2: [32, 40, 48, 64, 96],
          3: [24, 32, 48, 64, 96]}
CALLS, REPLAYS, REPEATS = 20, 10, 5

CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
layers = [int(a) for a in sys.argv[2].split(",")]
CALLS, REPLAYS, REPEATS = (int(a) for a in sys.argv[3:6])
from distributed_reinforcement_learning_amd import ops as _ops
ext = _ops.require_ext()
torch.manual_seed(0)
shapes = {0: ((640, 84, 84, 4), (640, 20, 20, 32)),
          2: ((640, 20, 20, 32), (640, 9, 9, 64)),
          3: ((640, 9, 9, 64), (640, 7, 7, 64))}
for layer in layers:
    ishape, oshape = shapes[layer]
    if layer == 0:
        x = torch.randint(0, 256, ishape, dtype=torch.uint8, device="cuda")
    else:
        x = (torch.randn(ishape, device="cuda") * 0.5).to(torch.bfloat16)
    dy = torch.randn(oshape, device="cuda").to(torch.bfloat16)
    for _ in range(3):
        ext.conv_wgrad(layer, x, dy)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            ext.conv_wgrad(layer, x, dy)
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
    print(f"RESULT {layer} {min(us):.2f} {max(us):.2f}", flush=True)
'''


def main():
    by_split = {}
    for layer, splits in SPLITS.items():
        for s in splits:
            by_split.setdefault(s, []).append(layer)
    rows = []
    for split in sorted(by_split):
        env = dict(os.environ, DRLA_WGRAD_SPLIT=str(split))
        layers = ",".join(str(l) for l in by_split[split])
        r = subprocess.run(
            [sys.executable, "-c", CHILD, ROOT, layers, str(CALLS),
             str(REPLAYS), str(REPEATS)],
            env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            print(f"split={split}: child failed rc={r.returncode}\n"
                  f"{r.stderr[-400:]}", flush=True)
            sys.exit(1)
        for line in r.stdout.splitlines():
            if line.startswith("RESULT"):
                _, layer, lo, hi = line.split()
                rows.append((int(layer), split, float(lo), float(hi)))
                print(f"L{layer} split={split}: {lo}..{hi} us", flush=True)
    lines = [f"conv_wgrad per call at N = 640, {CALLS} calls per graph, "
             f"{REPLAYS} replays per timing, min..max of {REPEATS} timings.",
             "", "| layer | split | min us | max us |", "|---|---|---|---|"]
    for layer, split, lo, hi in sorted(rows):
        lines.append(f"| {layer} | {split} | {lo:.2f} | {hi:.2f} |")
    text = "\n".join(lines)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
