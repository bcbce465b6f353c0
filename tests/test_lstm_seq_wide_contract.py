"""What the Python side and the HIP headers must agree on for the LSTM
sequence kernels' hidden-size cap, and that the CPU route is untouched by
it. No GPU needed."""

import os
import re

import torch

from distributed_reinforcement_learning_amd.models import R2D2LstmQ, r2d2_lstm
from distributed_reinforcement_learning_amd.ops import build as ops_build
from distributed_reinforcement_learning_amd.ops import lstm_op


def test_python_cap_equals_the_header_cap():
    with open(os.path.join(ops_build.HIP_DIR, "drla_common.h"),
              encoding="utf-8") as f:
        m = re.search(r"^#define LSTM_SEQ_MAX_HIDDEN (\d+)$", f.read(), re.M)
    assert m, "drla_common.h does not define LSTM_SEQ_MAX_HIDDEN"
    assert int(m.group(1)) == lstm_op.LSTM_SEQ_MAX_HIDDEN == 512


def test_kernel_route_predicate():
    ok = r2d2_lstm.seq_kernels_ok
    assert ok(True, torch.bfloat16, 64)
    assert ok(True, torch.bfloat16, 128)
    assert ok(True, torch.bfloat16, 512)
    assert not ok(True, torch.bfloat16, 513)
    assert not ok(False, torch.bfloat16, 64)
    assert not ok(True, torch.float32, 64)


def test_cpu_unroll_at_512_equals_its_step_loop():
    torch.manual_seed(3)
    H, B, L = 512, 2, 3
    m = R2D2LstmQ([84, 84, 1], 4, H)
    s = torch.rand(B, L, 84, 84, 1)
    pa = torch.randint(0, 4, (B, L))
    h0 = torch.randn(B, H) * 0.1
    c0 = torch.randn(B, H) * 0.1
    done = torch.zeros(B, L, dtype=torch.bool)
    done[0, 1] = True
    with torch.no_grad():
        q = m.unroll_sequence(s, pa, h0, c0, done)
        h, c = h0, c0
        qs = []
        for i in range(L):
            qi, h, c = m.single_step(s[:, i], pa[:, i], h, c)
            qs.append(qi)
            keep = (~done[:, i]).float().unsqueeze(1)
            h, c = h * keep, c * keep
        q_win = m.q_window(s, pa, h0, c0, done, 1)
    want = torch.stack(qs, dim=1)
    assert torch.allclose(q, want, atol=1e-5, rtol=1e-5)
    assert torch.allclose(q_win, want[:, 1:], atol=1e-5, rtol=1e-5)
