"""Gate-GEMM input assembled in place (no cat, no cast launch).

The IMPALA cell's GEMM input is xh = [conv features | action embedding | h |
pad] as one [N, 3136 + 256 + H + 8] bf16 matrix (pad = the ones-column block
of models/blocks._AugGateWeight). Instead of producing the parts separately
and copying them together, the producers store straight into one
preallocated slab: conv layer 3 writes its output with a row stride
(ops/conv_op.py, out_slab), and the action-embedding forward writes its
output, bf16(h) and the pad columns (ops/embed_op.py, xh_slab). This module
holds the slab layout and the autograd node that stands where the cat stood.
"""

from __future__ import annotations

import torch

PAD = 8  # models/blocks._AugGateWeight.PAD


def slab_width(conv_features: int, emb_features: int, hidden: int) -> int:
    return conv_features + emb_features + hidden + PAD


class _AssembleXh(torch.autograd.Function):
    """Forward launches nothing: conv_y and emb are already views of slab,
    which is returned as the assembled xh. Backward hands the column slices
    of dxh back as views, exactly as cat's backward does; the h and pad
    columns get no grad."""

    @staticmethod
    def forward(ctx, conv_y: torch.Tensor, emb: torch.Tensor,
                slab: torch.Tensor):
        ctx.conv_shape = conv_y.shape
        ctx.n_conv = conv_y[0].numel()
        ctx.n_emb = emb.shape[1]
        return slab.view_as(slab)

    @staticmethod
    def backward(ctx, dxh: torch.Tensor):
        n_conv, n_emb = ctx.n_conv, ctx.n_emb
        d_conv = dxh[:, :n_conv].view(ctx.conv_shape)
        d_emb = dxh[:, n_conv:n_conv + n_emb]
        return d_conv, d_emb, None


def assemble_xh(conv_y: torch.Tensor, emb: torch.Tensor,
                slab: torch.Tensor) -> torch.Tensor:
    """conv_y [N,7,7,64] and emb [N,256]: strided views of slab written by
    their kernels -> slab as the autograd-connected xh [N, R]."""
    return _AssembleXh.apply(conv_y, emb, slab)
