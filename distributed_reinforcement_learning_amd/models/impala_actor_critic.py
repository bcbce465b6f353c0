"""IMPALA conv+LSTM actor-critic (reference model/impala_actor_critic.py).

Key MI355X-first redesign: the reference evaluates the network 3x(T-2) times
per train step — once per timestep per first/middle/last window
(impala_actor_critic.py:71-114) — even though each LSTM step re-initializes
(h, c) from the *stored actor state* of that timestep, making every timestep
evaluation independent and the three windows overlapping slices of the same
T positions. Here ``unroll`` evaluates all B*T positions in ONE batched pass
(one conv launch, one fused gate GEMM), and the windows are views — identical
outputs, ~2.7x fewer evaluations, and launch shapes big enough to fill 256 CUs.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from distributed_reinforcement_learning_amd.models.blocks import (
    ActionEmbedding, AtariConvStack, LSTMCellTF, MLPHead,
)


class ImpalaActorCritic(nn.Module):
    def __init__(self, input_shape, num_action: int, lstm_hidden_size: int = 256):
        super().__init__()
        h, w, c = input_shape
        assert (h, w) == (84, 84), "Atari conv stack expects 84x84 frames"
        self.num_action = num_action
        self.lstm_hidden_size = lstm_hidden_size
        self.conv = AtariConvStack(c)
        self.action_emb = ActionEmbedding(num_action)
        feat = self.conv.out_features + self.action_emb.out_features
        self.lstm = LSTMCellTF(feat, lstm_hidden_size)
        self.policy_head = MLPHead(lstm_hidden_size, [256, 256], num_action,
                                   "softmax")
        self.value_head = MLPHead(lstm_hidden_size, [256, 256], 1, None)

    def single_step(self, state: torch.Tensor, prev_action: torch.Tensor,
                    h: torch.Tensor, c: torch.Tensor):
        """One cell step (what the reference's length-1 dynamic_rnn computes).

        state [N,84,84,C] normalized NHWC float; prev_action [N];
        h, c [N, H]. Returns (policy [N,A], value [N], h' [N,H], c' [N,H]).
        """
        feat = torch.cat(
            [self.conv(state), self.action_emb(prev_action)], dim=1)
        new_h, new_c = self.lstm(feat, h, c)
        policy = self.policy_head(new_h)
        value = self.value_head(new_h).squeeze(-1)
        return policy, value, new_h, new_c

    def forward(self, state, prev_action, h, c):
        return self.single_step(state, prev_action, h, c)

    # measurement / parity switch: False keeps the torch.cat assembly
    USE_XH_SLAB = True

    def _xh_slab_ok(self, flat_state, flat_h) -> bool:
        """The in-place xh assembly needs all three custom producers: the
        HIP conv stack, the fused embed MLP, and the bias-augmented gate
        weight (its pad columns are part of the slab)."""
        if not (self.USE_XH_SLAB and flat_state.is_cuda
                and flat_state.dtype == torch.uint8):
            return False
        from distributed_reinforcement_learning_amd.ops.conv_op import (
            custom_stack_ok,
        )
        return (custom_stack_ok(self.conv, flat_state)
                and self.action_emb.fused_ok()
                and self.lstm._aug_weight_ok()
                and flat_h.dtype == torch.float32
                and flat_h.shape[1] % 8 == 0)

    def _unroll_features(self, traj_state, traj_prev_action, traj_h, traj_c):
        B, T = traj_state.shape[:2]
        flat_state = traj_state.reshape(B * T, *traj_state.shape[2:])
        flat_pa = traj_prev_action.reshape(B * T)
        flat_h = traj_h.reshape(B * T, -1)
        flat_c = traj_c.reshape(B * T, -1)
        if self._xh_slab_ok(flat_state, flat_h):
            # the gate-GEMM input assembled IN PLACE: conv-l3 and the embed
            # MLP store into one preallocated slab (the embed kernel also
            # drops bf16(h) and the ones-pad in) — same xh as the cat below
            # builds, minus the cat and the h cast launches (ops/xh_op.py)
            from distributed_reinforcement_learning_amd.ops import xh_op
            from distributed_reinforcement_learning_amd.ops.conv_op import (
                atari_conv_stack,
            )
            n_conv = self.conv.out_features
            H = flat_h.shape[1]
            slab = torch.empty(
                B * T, xh_op.slab_width(n_conv, self.action_emb.out_features,
                                        H),
                dtype=torch.bfloat16, device=flat_state.device)
            conv_y = atari_conv_stack(self.conv, flat_state, out_slab=slab)
            emb = self.action_emb.forward_into(flat_pa, slab, n_conv,
                                               flat_h.contiguous())
            xh = xh_op.assemble_xh(conv_y, emb, slab)
            new_h, _ = self.lstm.forward_slab(xh, flat_c)
            return new_h, B, T
        conv_out = self.conv(flat_state)
        emb = self.action_emb(flat_pa)
        # ONE cat builds the gate-GEMM input directly (conv || emb || h
        # [|| ones — bias augmentation, blocks._AugGateWeight]); backward
        # slices it in place — the strided-view support in the conv/LSTM
        # backward kernels means no .contiguous() copies
        new_h, _ = self.lstm.forward_cat([conv_out, emb, flat_h], flat_c)
        return new_h, B, T

    def unroll(self, traj_state: torch.Tensor, traj_prev_action: torch.Tensor,
               traj_h: torch.Tensor, traj_c: torch.Tensor):
        """Batched evaluation over a whole trajectory.

        traj_state [B,T,84,84,C], traj_prev_action [B,T],
        traj_h/traj_c [B,T,H] (per-timestep stored actor states).
        Returns (policy softmax [B,T,A] f32, value [B,T]).
        """
        h, B, T = self._unroll_features(traj_state, traj_prev_action,
                                        traj_h, traj_c)
        policy = self.policy_head(h)
        value = self.value_head(h).squeeze(-1)
        return policy.reshape(B, T, -1), value.reshape(B, T)

    def unroll_logits(self, traj_state, traj_prev_action, traj_h, traj_c):
        """Like unroll() but returns pre-softmax logits [B,T,A] (model
        dtype) — the input of the fused V-trace loss kernel
        (ops/vtrace_loss_op.py). On GPU at the flagship head shape both
        heads run as ONE fused kernel (ops/hip/mlp_heads.hip)."""
        h, B, T = self._unroll_features(traj_state, traj_prev_action,
                                        traj_h, traj_c)
        from distributed_reinforcement_learning_amd.ops.mlp_heads_op import (
            fused_mlp_heads, heads_fusable,
        )
        if heads_fusable(self, h):
            logits, value = fused_mlp_heads(h.float(), self.policy_head,
                                            self.value_head)
            return logits.reshape(B, T, -1), value.reshape(B, T)
        logits = self.policy_head.logits(h)
        value = self.value_head(h).squeeze(-1)
        return logits.reshape(B, T, -1), value.reshape(B, T)
