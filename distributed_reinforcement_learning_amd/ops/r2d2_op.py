"""Fused R2D2 sequence-TD tail (K9) autograd wrapper.

One kernel each way over the post-burn-in Q windows replaces the ~18
eager torch launches of reference agent/r2d2.py:62-93's tail (reward
clip, discounts, slices, double-DQN argmax+gathers, value rescaling
h/h^-1 from optimizer/burn_in.py:23-32, squared error, three means, IS
weighting) — the R2D2 replay graph's remaining torch glue (VERDICT r1
item 7). Returns (loss, per-sequence priorities). ``n_step`` > 1 or a
``priority_eta`` selects the n-step forward (drla_r2d2_nstep_loss_fwd:
truncated n-step returns under h, eta*max|td| + (1-eta)*mean|td|
priorities); the backward is the same kernel either way.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from distributed_reinforcement_learning_amd import ops as _ops

_CLIP_MODE = {"abs_one": 0, "soft_asymmetric": 1, "none": 2}


class _FusedR2d2Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, main_q, target_q, actions, rewards, done, weights,
                gamma, clip_mode, n_step, eta):
        ext = _ops.require_ext()
        actions = actions.contiguous()
        weights = weights.contiguous()
        loss, td_st, td_out = ext.r2d2_loss_fwd(
            main_q.contiguous(), target_q.contiguous(), actions,
            rewards.contiguous(), done.contiguous(), weights, gamma,
            clip_mode, n_step, eta)
        ctx.save_for_backward(td_st, actions, weights)
        ctx.shape = (main_q.shape[1], main_q.shape[2])
        ctx.want_bf16 = main_q.dtype == torch.bfloat16
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(td_out)
        return loss[0], td_out

    @staticmethod
    def backward(ctx, g_loss, g_td):
        td_st, actions, weights = ctx.saved_tensors
        ext = _ops.require_ext()
        W, A = ctx.shape
        if g_loss is None:
            g_loss = torch.zeros(1, device=td_st.device)
        dmq = ext.r2d2_loss_bwd(td_st, actions, weights,
                                g_loss.reshape(1).float().contiguous(),
                                W, A, ctx.want_bf16)
        return (dmq,) + (None,) * 9


def fused_r2d2_loss(main_q: torch.Tensor, target_q: torch.Tensor,
                    actions: torch.Tensor, rewards: torch.Tensor,
                    done: torch.Tensor, weights: torch.Tensor,
                    gamma: float, reward_clipping: str, n_step: int = 1,
                    priority_eta: Optional[float] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """main_q [B,W,A] (bf16/f32, grad ok — the POST-burn-in window),
    target_q [B,W,A] (no grad), actions [B,W] int, rewards [B,W] f32 RAW,
    done [B,W] bool, weights [B] f32 -> (loss scalar, priorities [B]).
    Targets are n_step returns truncated at the window end; priorities are
    |mean td| when priority_eta is None, else eta*max|td| +
    (1-eta)*mean|td| (algorithms/nstep.py is the reference math)."""
    if n_step < 1:
        raise ValueError(f"n_step={n_step} must be >= 1")
    if priority_eta is not None and not 0.0 <= priority_eta <= 1.0:
        raise ValueError(f"priority_eta={priority_eta} must be in [0, 1]")
    # the extension takes a negative eta for the legacy |mean td| priority
    eta = -1.0 if priority_eta is None else float(priority_eta)
    return _FusedR2d2Loss.apply(
        main_q, target_q, actions.to(torch.int32), rewards, done, weights,
        float(gamma), _CLIP_MODE[reward_clipping], int(n_step), eta)


class _FusedDuelingHeadTrain(torch.autograd.Function):
    """Grad-carrying dueling head q = y[:A]-y[A], y = relu(h@Wt^T+bt)@Wo^T
    + bo over the R2D2 trained window: 1-launch forward (post-ReLU stash),
    2-launch backward (fused dz/dx/dh chain + weight-grad finalize) —
    replaced ~13 eager torch launches (~80 us/step at [608, 64])."""

    @staticmethod
    def forward(ctx, h, Wt, bt, Wo, bo):
        ext = _ops.require_ext()
        q, x_st = ext.dhead_train_fwd(h.contiguous(), Wt.contiguous(),
                                      bt.contiguous(), Wo.contiguous(),
                                      bo.contiguous())
        ctx.save_for_backward(x_st, h, Wt, Wo)
        ctx.set_materialize_grads(False)
        return q

    @staticmethod
    def backward(ctx, dq):
        x_st, h, Wt, Wo = ctx.saved_tensors
        ext = _ops.require_ext()
        if dq is None:
            return (None,) * 5
        dh, dWt, dbt, dWo, dbo = ext.dhead_train_bwd(
            dq.to(torch.bfloat16).contiguous(), x_st, h.contiguous(),
            Wt.contiguous(), Wo.contiguous())
        return dh, dWt, dbt, dWo, dbo


def fused_dueling_head_train(h: torch.Tensor, trunk, out) -> torch.Tensor:
    """h [N, IN] f32 (grad ok); trunk/out are the R2D2 head nn.Linears
    (bf16). Returns q [N, A] bf16 with full autograd."""
    return _FusedDuelingHeadTrain.apply(h, trunk.weight, trunk.bias,
                                        out.weight, out.bias)
