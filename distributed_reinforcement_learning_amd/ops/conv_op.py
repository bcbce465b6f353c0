"""Custom MFMA conv stack autograd wrapper (K1, ops/hip/conv.hip).

Layer ids (DRLA_CONV_LAYERS in hip/drla_common.h): 0 = 84x84x4 u8 ->
20x20x32 (IMPALA/A3C/Ape-X), 1 = 84x84x1 u8 (R2D2 POMDP), 2 = 20x20x32 ->
9x9x64, 3 = 9x9x64 -> 7x7x64.

The forward fuses /255-normalize (u8 layers), bias and ReLU. A single layer
(conv_layer / _ConvLayer) goes back as relu-mask -> custom wgrad (MFMA,
split-M atomics, its own finalize) + dgrad (MFMA implicit GEMM) + bias column
reduction. Weight layout is the channels_last flat view [CO][KH*KW*CI],
built in-graph so grads flow back to the nn.Conv2d weight.

The three-layer stack (atari_conv_stack) is ONE autograd node, _ConvStack,
whose backward is a chain of seven launches instead of eleven:

    relu_mask_bwd(dy3, y3)                 layer 3's mask + bias partials
    wgrad_l3(finalize=False)
    dgrad_l3(mask_src=y2, slot=2)          layer 2's mask and bias partials
    wgrad_l2(finalize=False)               in the dgrad epilogue
    dgrad_l2(mask_src=y1, slot=l1)         ... and layer 1's
    wgrad_l1(finalize=False)
    _conv_wgrad_finalize_all([l1, 2, 3])   one launch: every dW and dbias

All six gradients are final in stream order before backward() returns any of
them: a gradient handed back from a node may be read at once (AccumulateGrad
adds it into .grad immediately in eager mode), so a finalize is never
deferred across nodes. DRLA_CONV_FUSED_BWD=0 (read once at import into
FUSED_BWD) keeps the stack on three _ConvLayer nodes, for A/B runs.
"""

from __future__ import annotations

import os

import torch

from distributed_reinforcement_learning_amd import ops as _ops
from distributed_reinforcement_learning_amd.ops import input_slots

_LAYER_CO = {0: 32, 1: 32, 2: 64, 3: 64}

# atari_conv_stack as one autograd node with the fused backward chain
FUSED_BWD = os.environ.get("DRLA_CONV_FUSED_BWD") != "0"

# The weight gradients feed ONLY the optimizer (after the whole backward),
# while dx continues the critical dgrad chain — so the wgrad+finalize pair
# runs on a dedicated side stream and overlaps the rest of the backward
# (~95 us of MFMA wgrad work hidden behind dgrad/heads/embed). Under
# hipGraph capture the fork becomes graph edges and the graph owner joins
# once at capture end (join_wgrad_stream); eagerly each backward joins
# immediately (correctness over overlap — warmup only).
_WGRAD_STREAM = None


def _side_enabled() -> bool:
    # measured SLOWER inside the captured step on ROCm 7.2 (cross-stream
    # graph edges cost more than the overlap wins — 0.59 -> 1.01 ms/step,
    # r2); opt-in for experiments
    return os.environ.get("DRLA_WGRAD_SIDE") == "1"


def wgrad_stream() -> torch.cuda.Stream:
    global _WGRAD_STREAM
    if _WGRAD_STREAM is None:
        _WGRAD_STREAM = torch.cuda.Stream()
    return _WGRAD_STREAM


def join_wgrad_stream() -> None:
    """Order the current stream after all pending side-stream wgrads —
    call at the END of a captured backward region."""
    if _WGRAD_STREAM is not None:
        torch.cuda.current_stream().wait_stream(_WGRAD_STREAM)


# when True (set by GraphedImpalaStep around its warmup+captures), the u8
# layer-1 forward kernel bundles a pass-through copy of its input and the
# backward consumes THAT — the graphed step's overlapped H2D rewrites the
# static input during the backward otherwise (torn l1 wgrad reads)
STASH_INPUTS = False


def _mask_input(dy: torch.Tensor) -> torch.Tensor:
    """dy as relu_mask_bwd reads it: contiguous, or an N-strided 16 B-aligned
    view (a slice of the fused xh gradient); anything else is copied."""
    if not (dy.is_contiguous() or (dy.stride(-1) == 1
                                    and dy.dim() >= 2
                                    and dy.stride(0) % 8 == 0
                                    and dy.storage_offset() % 8 == 0)):
        dy = dy.contiguous()
    return dy


class _ConvLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w_flat: torch.Tensor,
                bias_f32: torch.Tensor, layer: int, out_slab=None):
        ext = _ops.require_ext()
        stash = STASH_INPUTS and layer <= 1
        # out_slab: the kernel stores into the leading columns of this wider
        # [N, R] buffer and y is that strided view (ops/xh_op.py)
        slot, dist = input_slots.lookup(x) if layer <= 1 else (None, 0)
        y, x_st = ext.conv_fwd(layer, x.contiguous(), w_flat.contiguous(),
                               bias_f32.contiguous(), stash, out_slab,
                               slot=slot,
                               slot_dist=[dist] if slot is not None else [])
        ctx.save_for_backward(x_st if stash else x, w_flat, y)
        ctx.layer = layer
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w_flat, y = ctx.saved_tensors
        ext = _ops.require_ext()
        layer = ctx.layer
        co = _LAYER_CO[layer]
        # mask kernel writes bias-grad partials into a persistent slot
        # buffer; the wgrad finalize that follows sums them -> bf16 dbias
        dy_m = ext.relu_mask_bwd(_mask_input(dy), y, co, layer)
        if _side_enabled():
            cur = torch.cuda.current_stream()
            side = wgrad_stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                dw, dbias = ext.conv_wgrad(layer, x, dy_m)
            if not torch.cuda.is_current_stream_capturing():
                # eager: join now, pin allocator lifetimes across streams
                cur.wait_stream(side)
                for t in (dw, dbias):
                    t.record_stream(cur)
                for t in (x, dy_m):
                    t.record_stream(side)
        else:
            dw, dbias = ext.conv_wgrad(layer, x, dy_m)
        dx = None
        if layer >= 2 and ctx.needs_input_grad[0]:
            dx = ext.conv_dgrad(layer, dy_m, w_flat)
        return dx, dw, dbias, None, None


class _ConvStack(torch.autograd.Function):
    """The three layers as one node (backward chain: module docstring)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, l1: int, out_slab=None):
        ext = _ops.require_ext()
        slot, dist = input_slots.lookup(x)
        y1, x_st = ext.conv_fwd(l1, x.contiguous(), w1.contiguous(),
                                b1.contiguous(), STASH_INPUTS, None,
                                slot=slot,
                                slot_dist=[dist] if slot is not None else [])
        y2, _ = ext.conv_fwd(2, y1, w2.contiguous(), b2.contiguous(), False)
        y3, _ = ext.conv_fwd(3, y2, w3.contiguous(), b3.contiguous(), False,
                             out_slab)
        ctx.save_for_backward(x_st if STASH_INPUTS else x, w2, w3, y1, y2, y3)
        ctx.l1 = l1
        return y3

    @staticmethod
    def backward(ctx, dy3: torch.Tensor):
        x, w2, w3, y1, y2, y3 = ctx.saved_tensors
        ext = _ops.require_ext()
        l1 = ctx.l1
        dy3_m = ext.relu_mask_bwd(_mask_input(dy3), y3, _LAYER_CO[3], 3)
        ext.conv_wgrad(3, y2, dy3_m, finalize=False)
        dy2_m = ext.conv_dgrad(3, dy3_m, w3, mask_src=y2, slot=2)
        ext.conv_wgrad(2, y1, dy2_m, finalize=False)
        dy1_m = ext.conv_dgrad(2, dy2_m, w2, mask_src=y1, slot=l1)
        ext.conv_wgrad(l1, x, dy1_m, finalize=False)
        (dw1, db1), (dw2, db2), (dw3, db3) = \
            ext._conv_wgrad_finalize_all([l1, 2, 3])
        return None, dw1, db1, dw2, db2, dw3, db3, None, None


def _flat_weight(conv: torch.nn.Conv2d) -> torch.Tensor:
    w = conv.weight
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv_layer(x: torch.Tensor, conv: torch.nn.Conv2d,
               layer: int, out_slab=None) -> torch.Tensor:
    """x NHWC (u8 for layers 0/1, bf16 for 2/3); returns NHWC bf16 output.

    conv.weight must be bf16 channels_last ([CO][KH][KW][CI] physically) —
    the flat view below is then a no-copy reshape.
    """
    return _ConvLayer.apply(x, _flat_weight(conv), conv.bias, layer, out_slab)


def atari_conv_stack(stack, x_u8_nhwc: torch.Tensor,
                     out_slab=None) -> torch.Tensor:
    """Full custom stack: u8 [N,84,84,C] -> flat [N,3136] bf16 features,
    flattened in NHWC order (identical to the torch path in
    models/blocks.AtariConvStack). With out_slab ([N, R >= 3136] bf16) the
    last layer stores straight into the slab's leading columns and the
    NHWC [N,7,7,64] strided view of them is returned unflattened."""
    ci = x_u8_nhwc.shape[-1]
    l1 = 0 if ci == 4 else 1
    if FUSED_BWD:
        y = _ConvStack.apply(
            x_u8_nhwc, _flat_weight(stack.conv1), stack.conv1.bias,
            _flat_weight(stack.conv2), stack.conv2.bias,
            _flat_weight(stack.conv3), stack.conv3.bias, l1, out_slab)
    else:
        y = conv_layer(x_u8_nhwc, stack.conv1, l1)
        y = conv_layer(y, stack.conv2, 2)
        y = conv_layer(y, stack.conv3, 3, out_slab)
    if out_slab is not None:
        return y
    return y.reshape(y.shape[0], -1)


def custom_stack_ok(stack, x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.uint8
            and x.shape[1] == 84 and x.shape[2] == 84
            and x.shape[3] in (1, 4)
            and stack.conv1.weight.dtype == torch.bfloat16
            and _ops.available())
