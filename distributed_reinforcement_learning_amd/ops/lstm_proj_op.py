"""The R2D2 LSTM layer's input projection and weight gradients on the
hand-written kernels (ops/hip/lstm_proj.hip).

The LSTM input is [conv | emb] along the features and lstm.weight is
[F + H, 4H] with F = F1 + F2. lstm_proj(conv, emb, weight, bias) is
bf16(conv @ weight[:F1] + emb @ weight[F1:F] + bias): the concatenation is
never written, the weight is read in place, the bias is added in f32 before
the one rounding. lstm_seq_layer is the whole trained layer as one autograd
node: the projection, the existing recurrence kernels, and on the way back one
launch for all of dW and db and one for dconv and demb.
"""

from __future__ import annotations

import os

import torch

from distributed_reinforcement_learning_amd import ops as _ops
from distributed_reinforcement_learning_amd.ops.lstm_op import (
    LSTM_SEQ_MAX_HIDDEN,
)

# Which uses run on the custom kernels by default: calls that store nothing
# for a backward (burn-in, target net, scoring) and the trained window. A
# False one stays on the library path because it has not passed the project's
# rule (KERNELS.md, "R2D2 LSTM projection"; profiles/lstm_proj_r14.md).
# DRLA_LSTM_PROJ=1 forces both, DRLA_LSTM_PROJ=0 turns the op off.
CUSTOM_NOGRAD = False
CUSTOM_TRAIN = False


def _rows_ok(t: torch.Tensor) -> bool:
    """2-D bf16 on the GPU, unit column stride, columns a positive multiple of
    8, every row at a multiple of 16 bytes."""
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2):
        return False
    rows, cols = t.shape
    ld = t.stride(0) if rows > 1 else cols
    return (cols >= 8 and cols % 8 == 0 and t.stride(1) == 1 and ld >= cols
            and ld % 8 == 0 and t.data_ptr() % 16 == 0)


def lstm_proj_ok(conv: torch.Tensor, emb: torch.Tensor, weight: torch.Tensor,
                 bias: torch.Tensor) -> bool:
    """True when the launchers take these operands and this use is switched
    on: the built extension; conv [M, F1], emb [M, F2] and weight
    [F1 + F2 + H, 4H] bf16 on the GPU with unit column stride and 16-byte
    aligned rows; F1 a multiple of 64, F2 of 8; H even in
    [2, LSTM_SEQ_MAX_HIDDEN]; bias [4H] dense and aligned; and
    DRLA_LSTM_PROJ / the CUSTOM_* flag of the use (grad mode picks it, as it
    picks the model's branch)."""
    env = os.environ.get("DRLA_LSTM_PROJ")
    if env == "0" or not _ops.available():
        return False
    if not (_rows_ok(conv) and _rows_ok(emb) and _rows_ok(weight)):
        return False
    f1, f2, n = conv.shape[1], emb.shape[1], weight.shape[1]
    hid = n // 4
    if not (conv.shape[0] == emb.shape[0] and f1 % 64 == 0 and n == 4 * hid
            and hid % 2 == 0 and 2 <= hid <= LSTM_SEQ_MAX_HIDDEN
            and weight.shape[0] == f1 + f2 + hid
            and conv.shape[0] * n < 2 ** 31):
        return False
    if not (bias.is_cuda and bias.dtype == torch.bfloat16
            and tuple(bias.shape) == (n,) and bias.stride(0) == 1
            and bias.data_ptr() % 16 == 0):
        return False
    flag = CUSTOM_TRAIN if torch.is_grad_enabled() else CUSTOM_NOGRAD
    return env == "1" or flag


def lstm_proj(conv: torch.Tensor, emb: torch.Tensor, weight: torch.Tensor,
              bias: torch.Tensor) -> torch.Tensor:
    """xg [M, 4H] bf16, forward only (no graph is recorded). The launcher
    refuses operands it cannot take (see lstm_proj_ok)."""
    return _ops.require_ext()._lstm_proj_fwd(
        conv.detach(), emb.detach(), weight.detach(), bias.detach())


class _LstmSeqLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, conv, emb, weight, bias, h0, c0, done, forget_bias):
        ext = _ops.require_ext()
        B, L = done.shape
        feat = conv.shape[1] + emb.shape[1]
        done = done.contiguous()
        xg = ext._lstm_proj_fwd(conv, emb, weight, bias)
        # the trailing H rows of a row-major weight: a dense view, no copy
        h_out, h_fin, c_fin, acts, c_prev, h_prev = ext.lstm_seq_train_fwd(
            xg.view(B, L, -1), weight[feat:].contiguous(), h0.contiguous(),
            c0.contiguous(), done, forget_bias)
        ctx.save_for_backward(conv, emb, weight, acts, c_prev, h_prev, done)
        ctx.set_materialize_grads(False)
        return h_out, h_fin, c_fin

    @staticmethod
    def backward(ctx, dh_out, dh_fin, dc_fin):
        conv, emb, weight, acts, c_prev, h_prev, done = ctx.saved_tensors
        ext = _ops.require_ext()
        B, L, H = c_prev.shape
        feat = conv.shape[1] + emb.shape[1]
        if dh_out is None:
            dh_out = torch.zeros(B, L, H, dtype=torch.float32,
                                 device=c_prev.device)
        dxg, dh0, dc0 = ext.lstm_seq_train_bwd(
            dh_out.float().contiguous(),
            None if dh_fin is None else dh_fin.float().contiguous(),
            None if dc_fin is None else dc_fin.float().contiguous(),
            acts, c_prev, weight[feat:].contiguous(), done)
        dxg = dxg.view(B * L, 4 * H)
        dw, db = ext._lstm_proj_wgrad(conv, emb, h_prev.view(B * L, H), dxg)
        dconv, demb = ext._lstm_proj_dgrad(dxg, weight, conv.shape[1],
                                           emb.shape[1])
        return dconv, demb, dw, db, dh0, dc0, None, None


def lstm_seq_layer(conv, emb, weight, bias, h0, c0, done,
                   forget_bias: float = 1.0):
    """conv [B*L, F1], emb [B*L, F2] bf16 (row b * L + t), weight
    [F1 + F2 + H, 4H], bias [4H] bf16, h0 / c0 [B, H] f32, done [B, L] bool ->
    (h_out [B, L, H] f32, h_fin, c_fin) of the done-masked recurrence, with
    gradients to conv, emb, weight, bias, h0 and c0."""
    return _LstmSeqLayer.apply(conv, emb, weight, bias, h0, c0, done,
                               float(forget_bias))
