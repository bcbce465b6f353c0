"""The R2D2 dueling head on the hand-written kernels (ops/hip/r2d2_head.hip).

r2d2_head(h_all, trunk, out, burn) = y[..., :A] - y[..., A:] with y =
out(relu(trunk(bf16(h_all[:, burn:])))) for trunk = nn.Linear(H, 128) and
out = nn.Linear(128, A + 1) in bf16, h_all [B, L, H] f32 as the LSTM sequence
kernels return it: one launch forward, two backward, the nn.Linear weights
read in place, the window slice and the f32 -> bf16 cast done in the kernel.
"""

from __future__ import annotations

import os

import torch

from distributed_reinforcement_learning_amd import ops as _ops

# Which uses run on the custom kernels by default: calls that store nothing
# for a backward (target net, scoring, acting on a sequence) and calls that do
# (the trained window). A False one stays on the path it had because it did
# not pass the project's rule (KERNELS.md, "R2D2 dueling head";
# profiles/r2d2_head_r12.md): the no-grad head is 2.4 - 23 times faster alone,
# but in the learner step it runs on the target net's side stream, off the
# critical path, and the step did not move. DRLA_R2D2_HEAD=1 forces both,
# DRLA_R2D2_HEAD=0 turns the op off.
CUSTOM_NOGRAD = False
CUSTOM_TRAIN = True

MID = 128
MAX_HIDDEN = 512
MAX_ACTIONS = 63


def _params(trunk, out):
    return [trunk.weight, trunk.bias, out.weight, out.bias]


def _wants_grad(h_all, params) -> bool:
    return torch.is_grad_enabled() and (
        h_all.requires_grad or any(p.requires_grad for p in params))


def r2d2_head_ok(h_all: torch.Tensor, trunk, out) -> bool:
    """True when r2d2_head takes these operands and this use is switched on:
    the built extension, h_all [B, L, H] f32 on the GPU, contiguous and
    16-byte aligned, H a multiple of 8 in [8, 512], trunk [128, H] and out
    [A + 1, 128] contiguous bf16 with 1 <= A <= 63, and DRLA_R2D2_HEAD / the
    CUSTOM_* flag of the use."""
    env = os.environ.get("DRLA_R2D2_HEAD")
    if env == "0" or not _ops.available():
        return False
    if not (h_all.is_cuda and h_all.dtype == torch.float32
            and h_all.dim() == 3 and h_all.is_contiguous()
            and h_all.data_ptr() % 16 == 0):
        return False
    hid = h_all.shape[2]
    if not (8 <= hid <= MAX_HIDDEN and hid % 8 == 0):
        return False
    p = _params(trunk, out)
    n_out = p[2].shape[0]
    if not ([tuple(t.shape) for t in p] == [(MID, hid), (MID,), (n_out, MID),
                                            (n_out,)]
            and 1 <= n_out - 1 <= MAX_ACTIONS
            and all(t.is_cuda and t.dtype == torch.bfloat16
                    and t.is_contiguous() for t in p)
            and all(t.data_ptr() % 16 == 0 for t in p[:3])):
        return False
    train = _wants_grad(h_all, p)
    return env == "1" or (CUSTOM_TRAIN if train else CUSTOM_NOGRAD)


class _R2D2Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, wt, bt, wo, bo):
        ext = _ops.require_ext()
        q, z = ext._r2d2_head_fwd(h, wt, bt, wo, bo, 0, True)
        ctx.save_for_backward(h, z, wt, wo)
        return q

    @staticmethod
    def backward(ctx, dq):
        ext = _ops.require_ext()
        h, z, wt, wo = ctx.saved_tensors
        dh, dwt, dbt, dwo, dbo = ext._r2d2_head_bwd(
            dq.reshape(-1, dq.shape[-1]).contiguous(),
            h.reshape(-1, h.shape[-1]), z, wt, wo)
        return dh.view_as(h), dwt, dbt, dwo, dbo


def r2d2_head(h_all: torch.Tensor, trunk, out, burn: int = 0) -> torch.Tensor:
    """Q [B, L - burn, A] bf16 of the steps from burn on. The launcher refuses
    operands it cannot take (see r2d2_head_ok). With a gradient wanted the
    kernels see the window as a tensor of its own, so dh comes back dense."""
    p = _params(trunk, out)
    if not _wants_grad(h_all, p):
        return _ops.require_ext()._r2d2_head_fwd(h_all, *p, int(burn),
                                                 False)[0]
    if burn:
        h_all = h_all[:, burn:].contiguous()
    return _R2D2Head.apply(h_all, *p)
