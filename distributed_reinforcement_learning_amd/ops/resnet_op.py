"""Custom MFMA path of the IMPALA ResNet torso (ops/hip/conv3x3.hip).

Layer ids (DRLA_CONV3_LAYERS in hip/drla_common.h), all 3x3 / stride 1 /
zero padding 1, NHWC bf16: 4 = 4->16 @84, 5 = 16->16 @42, 6 = 16->32 @42,
7 = 32->32 @21, 8 = 32->32 @11.

A section conv is one forward launch; its backward is wgrad (+ bias
gradient, same pass) and, except for the first layer, dgrad. A residual block
x + c2(relu(c1(relu(x)))) is two forward launches (input ReLU fused into the
A-tile staging, skip add fused into the second epilogue) and four backward
MFMA launches plus the two wgrad finalizes; the ReLU masks and the skip
gradient ride in the dgrad epilogues, so no elementwise torch op runs.
Weights are consumed as the channels_last flat view [CO][9*CI], built
in-graph so the gradients flow back to the nn.Conv2d parameters.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from distributed_reinforcement_learning_amd import ops as _ops

# (section conv layer id, residual block layer id) per section
SECTION_LAYERS = ((4, 5), (6, 7), (7, 8))
_CHANNELS = (16, 32, 32)


def _flat(conv: torch.nn.Conv2d) -> torch.Tensor:
    w = conv.weight
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_flat, bias, layer: int):
        ext = _ops.require_ext()
        x = x.contiguous()
        y, _ = ext.conv_fwd(layer, x, w_flat.contiguous(), bias.contiguous(),
                            False)
        ctx.save_for_backward(x, w_flat)
        ctx.layer = layer
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_flat = ctx.saved_tensors
        ext = _ops.require_ext()
        dy = dy.contiguous()
        dw, db = ext.conv_wgrad(ctx.layer, x, dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ext.conv_dgrad(ctx.layer, dy, w_flat.contiguous())
        return dx, dw, db, None


class _ResBlock3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, layer: int):
        ext = _ops.require_ext()
        x = x.contiguous()
        y1, _ = ext.conv_fwd(layer, x, w1.contiguous(), b1.contiguous(),
                             False, relu_in=True)
        out, _ = ext.conv_fwd(layer, y1, w2.contiguous(), b2.contiguous(),
                              False, relu_in=True, residual=x)
        ctx.save_for_backward(x, y1, w1, w2)
        ctx.layer = layer
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y1, w1, w2 = ctx.saved_tensors
        ext = _ops.require_ext()
        layer = ctx.layer
        dout = dout.contiguous()
        dw2, db2 = ext.conv_wgrad(layer, y1, dout, relu_in=True)
        dy1 = ext.conv_dgrad(layer, dout, w2.contiguous(), mask_src=y1)
        dw1, db1 = ext.conv_wgrad(layer, x, dy1, relu_in=True)
        dx = ext.conv_dgrad(layer, dy1, w1.contiguous(), mask_src=x,
                            addend=dout)
        return dx, dw1, db1, dw2, db2, None


def conv3x3(x_nhwc: torch.Tensor, conv: torch.nn.Conv2d,
            layer: int) -> torch.Tensor:
    """NHWC bf16 in, NHWC bf16 conv(x) + bias out (no activation)."""
    return _Conv3x3.apply(x_nhwc, _flat(conv), conv.bias, layer)


def res_block(x_nhwc: torch.Tensor, block, layer: int) -> torch.Tensor:
    """x + c2(relu(c1(relu(x)))) for a models.impala_resnet._ResBlock."""
    return _ResBlock3x3.apply(x_nhwc, _flat(block.c1), block.c1.bias,
                              _flat(block.c2), block.c2.bias, layer)


def resnet_torso(torso, x_nhwc: torch.Tensor) -> torch.Tensor:
    """bf16 [N,84,84,4] -> the torso's [N,256] features. Convs, input ReLUs
    and skip adds run on the custom kernels; max-pool, the last ReLU and fc
    stay torch ops on channels_last views (the NCHW view of an NHWC tensor
    IS channels_last, and the pool keeps that format, so neither permute
    copies)."""
    x = x_nhwc
    for sec, (lc, lr) in zip(torso.sections, SECTION_LAYERS):
        x = conv3x3(x, sec.conv, lc)
        x = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride=2, padding=1)
        x = x.permute(0, 2, 3, 1)
        x = res_block(x, sec.r1, lr)
        x = res_block(x, sec.r2, lr)
    x = F.relu(x)
    return F.relu(torso.fc(x.flatten(1)))


def resnet_torso_ok(torso, x: torch.Tensor) -> bool:
    """True when the custom path can and should run: CUDA input of 84x84x4
    frames, bf16 weights, channels (16, 32, 32), built extension, and
    DRLA_RESNET_CONV not "0" (read at call time: the A/B switch)."""
    if os.environ.get("DRLA_RESNET_CONV") == "0":
        return False
    if not (x.is_cuda and len(x.shape) == 4
            and tuple(x.shape[1:]) == (84, 84, 4)):
        return False
    convs = [s.conv for s in torso.sections]
    if tuple(c.out_channels for c in convs) != _CHANNELS:
        return False
    if convs[0].in_channels != 4:
        return False
    if convs[0].weight.dtype != torch.bfloat16:
        return False
    return _ops.available()
