"""3x3 / stride 2 / padding 1 max-pool on NHWC bf16 (ops/hip/maxpool.hip).

The forward returns the pooled tensor and, when a gradient is wanted, one
byte per output element: tap = kh*3 + kw of the winning window element
(scan kh then kw, first maximum wins, NaN propagates - the rule of
F.max_pool2d). That byte tensor is all the backward saves; the backward is a
gather that writes every input-gradient element once.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from distributed_reinforcement_learning_amd import ops as _ops


class _MaxPool3x3S2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, want_tap: bool):
        ext = _ops.require_ext()
        y, tap = ext._maxpool3s2_fwd(x.contiguous(), want_tap)
        if want_tap:
            ctx.save_for_backward(tap)
            ctx.hw = (x.shape[1], x.shape[2])
        return y

    @staticmethod
    def backward(ctx, dy):
        (tap,) = ctx.saved_tensors
        ext = _ops.require_ext()
        return ext._maxpool3s2_bwd(dy.contiguous(), tap, *ctx.hw), None


def library_pool3x3s2(x_nhwc: torch.Tensor) -> torch.Tensor:
    """F.max_pool2d on the channels_last view: the NCHW view of an NHWC
    tensor IS channels_last and the pool keeps that format, so neither
    permute copies."""
    y = F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, stride=2, padding=1)
    return y.permute(0, 2, 3, 1)


def max_pool3x3s2(x_nhwc: torch.Tensor) -> torch.Tensor:
    """[N, H, W, C] -> [N, (H-1)//2 + 1, (W-1)//2 + 1, C], both NHWC.
    GPU: bf16 with C = 16 or 32, on the custom kernels (the extension is
    required). CPU: library_pool3x3s2."""
    if not x_nhwc.is_cuda:
        return library_pool3x3s2(x_nhwc)
    # Function.forward runs with grad mode off: decide here
    want_tap = torch.is_grad_enabled() and x_nhwc.requires_grad
    return _MaxPool3x3S2.apply(x_nhwc, want_tap)
