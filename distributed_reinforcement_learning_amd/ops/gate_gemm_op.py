"""The LSTM cell's gate GEMM on the hand-written kernels (ops/hip/gate_gemm.hip).

gate_gemm(xh, w) = xh @ w for bf16 xh [M, K] and w [K, N] with unit column
stride; row strides are free, so the xh slab (ops/xh_op.py) and the
as_strided augmented weight (models/blocks._AugGateWeight) are read in place.
The backward is two more kernels: dxh = dg @ w^T, computed only for the
leading grad_cols columns (the rest are stored as zeros), and dw = xh^T @ dg.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from distributed_reinforcement_learning_amd import ops as _ops

# Which directions run on the custom kernels by default; a False one stays on
# the library GEMM because it measured slower than it at the flagship shape
# (KERNELS.md, "Gate GEMM"; profiles/gate_gemm_r10.md). DRLA_GATE_GEMM=1
# forces all three, DRLA_GATE_GEMM=0 turns the op off (gate_gemm_ok).
CUSTOM_FWD = True
CUSTOM_DGRAD = False
CUSTOM_WGRAD = False


def _custom(flag: bool) -> bool:
    return flag or os.environ.get("DRLA_GATE_GEMM") == "1"


def _operand_ok(t: torch.Tensor) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2
            and t.shape[1] >= 8 and t.shape[1] % 8 == 0 and t.stride(1) == 1
            and (t.shape[0] <= 1 or (t.stride(0) >= t.shape[1]
                                     and t.stride(0) % 8 == 0))
            and t.data_ptr() % 16 == 0)


def gate_gemm_ok(xh: torch.Tensor, w: torch.Tensor) -> bool:
    """True when gate_gemm takes these operands: CUDA, bf16, the built
    extension, 16-byte-aligned rows of a multiple of 8 columns, and
    DRLA_GATE_GEMM != "0"."""
    return (os.environ.get("DRLA_GATE_GEMM") != "0" and _ops.available()
            and _operand_ok(xh) and _operand_ok(w)
            and xh.shape[1] == w.shape[0])


class _GateGemm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh, w, grad_cols: int, split: int):
        ext = _ops.require_ext()
        ctx.save_for_backward(xh, w)
        ctx.grad_cols = grad_cols
        if _custom(CUSTOM_FWD):
            return ext._gate_gemm_fwd(xh, w, split)
        return torch.mm(xh, w)

    @staticmethod
    def backward(ctx, dg):
        xh, w = ctx.saved_tensors
        ext = _ops.require_ext()
        if dg.stride(1) != 1 or dg.stride(0) % 8 or dg.data_ptr() % 16:
            dg = dg.contiguous()
        dxh = dw = None
        if ctx.needs_input_grad[0]:
            if _custom(CUSTOM_DGRAD):
                dxh = ext._gate_gemm_dgrad(dg, w, ctx.grad_cols)
            else:
                dxh = torch.mm(dg, w.t())
        if ctx.needs_input_grad[1]:
            if _custom(CUSTOM_WGRAD):
                dw = ext._gate_gemm_wgrad(xh, dg)
            else:
                dw = torch.mm(xh.t(), dg)
        return dxh, dw, None, None


def gate_gemm(xh: torch.Tensor, w: torch.Tensor,
              grad_cols: Optional[int] = None, split: int = 0) -> torch.Tensor:
    """xh [M, K] @ w [K, N] -> [M, N] bf16 (requires gate_gemm_ok).
    grad_cols: how many leading xh columns get a gradient (default: all);
    the rest of dxh is zero. split: forward K-split, 0 = the launcher's rule
    (ext._gate_gemm_split)."""
    if grad_cols is None:
        grad_cols = xh.shape[1]
    return _GateGemm.apply(xh, w, int(grad_cols), int(split))
