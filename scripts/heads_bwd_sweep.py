"""Time the two IMPALA heads backward kernels alone (drla_mlp_heads_bwd and
drla_heads_wgrad) at the flagship shape N = 640, A = 18, on the
tensors a real forward leaves behind.

Each kernel is REP back-to-back calls captured in a graph (GPU time only),
timed over 50 replays with device events, five times; a line shows min..max
of the five in microseconds per call. --short does one timed round of five
replays (for a counter run, where every dispatch is serialised).

Usage: python scripts/heads_bwd_sweep.py [--short]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_reinforcement_learning_amd import ops  # noqa: E402
from distributed_reinforcement_learning_amd.models.blocks import (  # noqa: E402
    MLPHead,
)

N, A, REP = 640, 18, 20
SHORT = "--short" in sys.argv
torch.manual_seed(0)
ext = ops.require_ext()
ph = MLPHead(256, [256, 256], A, None).cuda().bfloat16()
vh = MLPHead(256, [256, 256], 1, None).cuda().bfloat16()
weights = [ph.hidden[0].weight, ph.hidden[1].weight, ph.out.weight,
           vh.hidden[0].weight, vh.hidden[1].weight, vh.out.weight]
biases = [ph.hidden[0].bias, ph.hidden[1].bias, ph.out.bias,
          vh.hidden[0].bias, vh.hidden[1].bias, vh.out.bias]
weights = [w.detach().contiguous() for w in weights]
biases = [b.detach().contiguous() for b in biases]


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
    rounds, replays = (1, 5) if SHORT else (5, 50)
    for _ in range(2 if SHORT else 5):
        g.replay()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / (replays * REP))
    print(f"{label}: {min(ts):.1f}..{max(ts):.1f} us", flush=True)


h = torch.randn(N, 256, device="cuda")
logits, value, stash, ws, packed = ext.mlp_heads_fwd(
    h, weights, biases, A, want_bwd_bufs=True)
wT = [packed.narrow(0, 0, 65536).view(256, 256),
      packed.narrow(0, 65536, 65536).view(256, 256),
      packed.narrow(0, 131072, 8192).view(256, 32),
      packed.narrow(0, 139264, 65536).view(256, 256),
      packed.narrow(0, 204800, 65536).view(256, 256),
      packed.narrow(0, 270336, 256).view(1, 256)]
dlogits = (torch.randn(N, A, device="cuda") * 0.1).bfloat16()
dvalue = torch.randn(N, device="cuda") * 0.1
# the repeated calls keep adding into the one workspace: the sums are not
# results here, only the time is
res = ext.mlp_heads_bwd(dlogits, dvalue, stash, wT, A, ws=ws)
dz1p, dz2p, dz1v, dz2v = res[:4]

timed(lambda: ext.mlp_heads_bwd(dlogits, dvalue, stash, wT, A, ws=ws),
      f"drla_mlp_heads_bwd N={N} A={A}")
timed(lambda: ext.mlp_heads_wgrad(dz1p, dz2p, dz1v, dz2v, dlogits, dvalue,
                                  stash, ws, A),
      f"drla_heads_wgrad N={N} A={A}")
