"""lr_t_for: the value a captured step writes into lr_buf before a replay.
RMSProp applies the schedule's lr as is; Adam folds its bias correction
into it (TF AdamOptimizer: lr * sqrt(1 - b2^t) / (1 - b1^t))."""

import math

import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.zeros(4))]


@pytest.mark.parametrize("t", [1, 10])
def test_rmsprop_lr_t_is_identity(t):
    from distributed_reinforcement_learning_amd.ops.optim import FusedRMSProp
    opt = FusedRMSProp(_params(), lr=1e-3)
    assert opt.lr_t_for(6e-4, t) == 6e-4


@pytest.mark.parametrize("t", [1, 10])
def test_adam_lr_t_is_bias_corrected(t):
    from distributed_reinforcement_learning_amd.ops.optim import FusedAdam
    b1, b2, lr = 0.9, 0.999, 1e-4
    opt = FusedAdam(_params(), lr=lr, beta1=b1, beta2=b2)
    want = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    assert opt.lr_t_for(lr, t) == pytest.approx(want, rel=1e-12)
    assert opt.lr_t_for(lr, t) != lr
