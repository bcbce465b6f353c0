"""R2D2 agent — capability-parity with reference agent/r2d2.py: recurrent
dueling double-DQN over stored sequences with burn-in, value-function
rescaling (optimizer/burn_in.py:23-32), per-sequence priorities
(|mean TD|, agent/r2d2.py:125-126,151-153), IS-weighted loss, and
main_to_target hard sync every 2500 steps (train_r2d2.py:164-165).

Burn-in redesign (BASELINE "burn_in hidden-state recompute" hot-path item):
by default the first ``burn_in`` steps run under no_grad purely to recompute
the hidden state (the R2D2 paper's burn-in), then the trained window unrolls
with gradient. ``burn_in_gradient=True`` reproduces the reference's exact
behavior (gradient flows through the burn-in steps; the loss is still sliced
at burn_in) for parity checks.

Beyond the reference: ``n_step`` > 1 trains on n-step returns under the
value rescaling, taken inside the post-burn-in window and truncated at its
end, and ``priority_eta`` switches the sequence priority to the R2D2
paper's eta*max|TD| + (1-eta)*mean|TD| (algorithms/nstep.py). The defaults
(1, None) are the reference's 1-step targets and |mean TD|.
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from distributed_reinforcement_learning_amd.agents.base import AgentBase, clip_rewards
from distributed_reinforcement_learning_amd.algorithms import burn_in as rescale
from distributed_reinforcement_learning_amd.algorithms import dqn
from distributed_reinforcement_learning_amd.algorithms import nstep
from distributed_reinforcement_learning_amd.models import R2D2LstmQ
from distributed_reinforcement_learning_amd.ops import FusedAdam


class Agent(AgentBase):
    def __init__(self, seq_len: int, burn_in: int, input_shape,
                 num_action: int, lstm_size: int, discount_factor: float,
                 start_learning_rate: float, end_learning_rate: float,
                 learning_frame: int, gradient_clip_norm: float,
                 reward_clipping: str = "abs_one", device: str = "cpu",
                 compute_dtype: torch.dtype = torch.bfloat16,
                 build_optimizer: bool = True, seed: Optional[int] = None,
                 burn_in_gradient: bool = False, n_step: int = 1,
                 priority_eta: Optional[float] = None):
        super().__init__(device=device, compute_dtype=compute_dtype)
        if int(n_step) != n_step or n_step < 1:
            raise ValueError(f"n_step={n_step!r} must be an integer >= 1")
        if priority_eta is not None and not 0.0 <= priority_eta <= 1.0:
            raise ValueError(
                f"priority_eta={priority_eta!r} must be in [0, 1] or None")
        # n-step returns inside the post-burn-in window, truncated at its
        # end (algorithms/nstep.py); priority_eta None keeps the
        # reference's |mean TD| sequence priority
        self.n_step = int(n_step)
        self.priority_eta = (None if priority_eta is None
                             else float(priority_eta))
        self.seq_len = seq_len
        self.burn_in = burn_in
        self.input_shape = tuple(input_shape)
        self.num_action = num_action
        self.lstm_size = lstm_size
        self.discount_factor = discount_factor
        self.start_learning_rate = start_learning_rate
        self.end_learning_rate = end_learning_rate
        self.learning_frame = learning_frame
        self.gradient_clip_norm = gradient_clip_norm
        self.reward_clipping = reward_clipping
        self.burn_in_gradient = burn_in_gradient
        if seed is not None:
            torch.manual_seed(seed)
        self.rng = np.random.default_rng(seed)

        self.model = self.finalize_model(
            R2D2LstmQ(self.input_shape, num_action, lstm_size))
        self.target_model = self.finalize_model(
            R2D2LstmQ(self.input_shape, num_action, lstm_size))
        self.target_model.load_state_dict(self.model.state_dict())
        for p in self.target_model.parameters():
            p.requires_grad_(False)
        self.optimizer = None
        if build_optimizer:
            # reference agent/r2d2.py:91: Adam(1e-4), no explicit clip — we
            # keep the constructor's clip_norm wired (pass None to disable)
            self.optimizer = FusedAdam(self.model.parameters(),
                                       lr=start_learning_rate,
                                       clip_norm=gradient_clip_norm)

    def main_to_target(self) -> None:
        self.target_model.load_state_dict(self.model.state_dict())

    def _checkpoint_extra(self):
        return {"target_model": self.target_model.state_dict()}

    def _load_checkpoint_extra(self, blob):
        if "target_model" in blob:
            self.target_model.load_state_dict(blob["target_model"])

    # -- core sequence evaluation -------------------------------------------

    def _unroll_q(self, model, s, pa, h0, c0, d, with_grad: bool):
        """Unroll ``model`` over the full sequence; by default the first
        burn_in steps run as a detached hidden-state recompute
        (model.burn_in_states — one fused kernel on GPU), and only the
        trained window unrolls with gradient."""
        if with_grad and not self.burn_in_gradient and self.burn_in > 0:
            b = self.burn_in
            h, c = model.burn_in_states(s[:, :b], pa[:, :b], h0, c0,
                                        d[:, :b])
            q_rest = model.unroll_sequence(s[:, b:], pa[:, b:], h.detach(),
                                           c.detach(), d[:, b:])
            # burn-in Q values never enter the loss (it slices [:, b:]);
            # pad with detached zeros to keep the [B, L] interface
            B = s.shape[0]
            pad = torch.zeros(B, b, q_rest.shape[-1], dtype=q_rest.dtype,
                              device=q_rest.device)
            return torch.cat([pad, q_rest], dim=1)
        ctx = torch.enable_grad() if with_grad else torch.no_grad()
        with ctx:
            return model.unroll_sequence(s, pa, h0, c0, d)

    def _prep_seq(self, state, previous_action, action, h0, c0, reward,
                  done):
        s = self.frames_to_device(state)
        pa = self.to_device(previous_action, torch.int64)
        a = self.to_device(action, torch.int64)
        r = self.to_device(reward, torch.float32)
        d = self.to_device(done, torch.bool)
        h = self.to_device(h0, torch.float32)
        c = self.to_device(c0, torch.float32)
        return s, pa, a, r, d, h, c

    def _use_fused_tail(self) -> bool:
        from distributed_reinforcement_learning_amd import ops as _ops
        return (self.device.type == "cuda" and not self.burn_in_gradient
                and self.seq_len - self.burn_in >= 2 and _ops.available())

    def _window_qs(self, s, pa, d, h, c, with_grad: bool):
        """Post-burn-in Q windows [B, L-burn_in, A]: main (grad per
        ``with_grad``), target (never). Both nets burn in via the fused
        no-grad state recompute and unroll only the trained window — no
        burn-in head evaluations, no zero-pad/cat (the eager _unroll_q
        padded to keep the [B,L] interface)."""
        b = self.burn_in
        # the target-net evaluation is independent of every main-net pass
        # and the seq-recurrence kernels run one block per sequence (B=16
        # workgroups on a 256-CU chip) — overlap it on a side stream.
        # Stream forks are capture-legal: hipGraph capture spans streams
        # and records the fork/join edges.
        import os as _os
        side = getattr(self, "_tgt_stream", None)
        if (side is None and self.device.type == "cuda"
                and _os.environ.get("DRLA_NO_TGT_STREAM") != "1"):
            side = self._tgt_stream = torch.cuda.Stream()
        main_stream = torch.cuda.current_stream() if side else None
        with torch.no_grad():
            if side is not None:
                side.wait_stream(main_stream)
                with torch.cuda.stream(side):
                    # ONE full-sequence pass (conv/embed/Wx once, one
                    # recurrence kernel, fused head on the window only)
                    tgt_w = self.target_model.q_window(s, pa, h, c, d, b)
            else:
                tgt_w = self.target_model.q_window(s, pa, h, c, d, b)
            if not with_grad:
                main_w = self.model.q_window(s, pa, h, c, d, b)
                if side is not None:
                    main_stream.wait_stream(side)
                    # allocated on side, consumed on main (eager only:
                    # inside capture the graph pool owns lifetimes)
                    if not torch.cuda.is_current_stream_capturing():
                        tgt_w.record_stream(main_stream)
                return main_w, tgt_w
            if b > 0:
                hm, cm = self.model.burn_in_states(s[:, :b], pa[:, :b],
                                                   h, c, d[:, :b])
            else:
                hm, cm = h, c
        # main net: separate no-grad burn-in keeps the trained window's
        # backward from sweeping the burn-in frames
        main_w = self.model.unroll_sequence(
            s[:, b:], pa[:, b:], hm.detach(), cm.detach(), d[:, b:])
        if side is not None:
            main_stream.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                tgt_w.record_stream(main_stream)
        return main_w, tgt_w

    def _fused_seq_loss(self, state, previous_action, action, h0, c0,
                        reward, done, w, with_grad: bool):
        """GPU fast path: one-kernel TD tail (K9, ops/hip/r2d2_loss.hip)
        over the trained window; the n-step kernel when n_step > 1 or
        priority_eta is set. Returns (weighted loss, priorities [B])."""
        from distributed_reinforcement_learning_amd.ops.r2d2_op import (
            fused_r2d2_loss,
        )
        s, pa, a, r, d, h, c = self._prep_seq(
            state, previous_action, action, h0, c0, reward, done)
        main_w, tgt_w = self._window_qs(s, pa, d, h, c, with_grad)
        b = self.burn_in
        return fused_r2d2_loss(main_w, tgt_w, a[:, b:], r[:, b:],
                               d[:, b:], w, self.discount_factor,
                               self.reward_clipping, n_step=self.n_step,
                               priority_eta=self.priority_eta)

    def _sequence_losses(self, state, previous_action, action, h0, c0,
                         reward, done, with_grad: bool):
        """Returns (per-sequence unweighted loss [B], target_value,
        state_action_value) over the post-burn-in window — the math of
        reference agent/r2d2.py:62-93."""
        s = self.frames_to_device(state)
        pa = self.to_device(previous_action, torch.int64)
        a = self.to_device(action, torch.int64)
        r = self.to_device(reward, torch.float32)
        d = self.to_device(done, torch.bool)
        h = self.to_device(h0, torch.float32)
        c = self.to_device(c0, torch.float32)

        with self.autocast():
            main_q = self._unroll_q(self.model, s, pa, h, c, d,
                                    with_grad).float()
            target_q = self._unroll_q(self.target_model, s, pa, h, c, d,
                                      False).float()

        clipped_r = clip_rewards(r, self.reward_clipping)
        discounts = (~d).float() * self.discount_factor

        b = self.burn_in
        bm, bt = main_q[:, b:], target_q[:, b:]
        br, bg, ba = clipped_r[:, b:], discounts[:, b:], a[:, b:]

        state_main_q = bm[:, :-1]
        act = ba[:, :-1]

        sav = dqn.take_state_action_value(state_main_q, act)
        # every row's own double-DQN bootstrap (row 0's is never used);
        # nstep_window_target picks row t+k for position t
        own_action = bm.argmax(dim=2)
        nsav = dqn.take_state_action_value(bt, own_action)
        rescaled_next = rescale.inverse_value_function_rescaling(nsav)
        rescaled_target = nstep.nstep_window_target(
            rescaled_next, br, bg, self.n_step).detach()
        target_value = rescale.value_function_rescaling(rescaled_target)
        unweighted = ((target_value - sav) ** 2).mean(dim=1)
        return unweighted, target_value, sav

    # -- public API ----------------------------------------------------------

    @torch.no_grad()
    def get_td_error(self, state, previous_action, action, h, c, reward,
                     done) -> float:
        """Priority for ONE freshly-arrived sequence: |mean TD| (reference
        agent/r2d2.py:97-127), or the eta max/mean mix when priority_eta
        is set. h/c are the per-step stored states; step 0's is the
        sequence's initial state."""
        h0 = np.asarray(h)[0]
        c0 = np.asarray(c)[0]
        _, target_value, sav = self._sequence_losses(
            np.asarray(state)[None], np.asarray(previous_action)[None],
            np.asarray(action)[None], h0[None], c0[None],
            np.asarray(reward)[None], np.asarray(done)[None],
            with_grad=False)
        return float(nstep.sequence_priority(target_value - sav,
                                             self.priority_eta)[0])

    @torch.no_grad()
    def get_td_error_batch(self, state, previous_action, action, h0, c0,
                           reward, done, as_tensor: bool = False):
        """Per-sequence |mean TD| for a whole [B, L] batch in one forward
        (device tensors ok; feeds the GPU replay shard directly)."""
        if self._use_fused_tail():
            B = state.shape[0]
            w1 = torch.ones(B, dtype=torch.float32, device=self.device)
            _, td = self._fused_seq_loss(state, previous_action, action,
                                         h0, c0, reward, done, w1,
                                         with_grad=False)
            return td if as_tensor else td.cpu().numpy()
        _, target_value, sav = self._sequence_losses(
            state, previous_action, action, h0, c0, reward, done,
            with_grad=False)
        td = nstep.sequence_priority(target_value - sav, self.priority_eta)
        return td if as_tensor else td.cpu().numpy()

    def compute_sequence_loss(self, state, previous_action, action, h0,
                              c0, reward, done, w):
        """Pure loss body (shared by train and the graphed replay step):
        returns (weighted scalar loss, per-sequence priority tensor —
        |mean TD|, or the priority_eta max/mean mix)."""
        if self._use_fused_tail():
            w_t = self.to_device(w, torch.float32)
            return self._fused_seq_loss(state, previous_action, action,
                                        h0, c0, reward, done, w_t,
                                        with_grad=True)
        unweighted, target_value, sav = self._sequence_losses(
            state, previous_action, action, h0, c0, reward, done,
            with_grad=True)
        loss = (unweighted * w).mean()
        td = nstep.sequence_priority(target_value - sav,
                                     self.priority_eta).detach()
        return loss, td

    def train(self, state, previous_action, action, h, c, reward, done,
              weight, as_tensor: bool = False) -> Tuple[float, np.ndarray]:
        """IS-weighted batch update; h/c [B, L, H] stored per step — the
        sequence-start state is index 0 (reference train_r2d2.py:135-136).
        Returns (loss, per-sequence |mean TD|)."""
        h0 = h[:, 0] if isinstance(h, torch.Tensor) else np.asarray(h)[:, 0]
        c0 = c[:, 0] if isinstance(c, torch.Tensor) else np.asarray(c)[:, 0]
        w = self.to_device(weight, torch.float32)
        loss, td_t = self.compute_sequence_loss(
            state, previous_action, action, h0, c0, reward, done, w)

        self.optimizer.zero_grad()
        loss.backward()
        self.reduce_gradients()
        lr = self.lr_at(self.global_step)
        self.optimizer.step(lr=lr)
        self.global_step += 1
        self.num_env_frames += int(np.prod(np.shape(reward)))
        if as_tensor:
            return loss.detach(), td_t
        return float(loss.detach()), td_t.cpu().numpy()

    @torch.no_grad()
    def main_q_value_test(self, state, h, c, done, previous_action):
        """Debug helper (reference agent/r2d2.py:188-199): main-net Q
        values over one stored sequence."""
        s = self.frames_to_device(np.asarray(state)[None])
        pa = self.to_device(np.asarray(previous_action)[None], torch.int64)
        d = self.to_device(np.asarray(done)[None], torch.bool)
        h0 = self.to_device(np.asarray(h)[0][None], torch.float32)
        c0 = self.to_device(np.asarray(c)[0][None], torch.float32)
        q = self.model.unroll_sequence(s, pa, h0, c0, d)
        return q[0].float().cpu().numpy()

    @torch.no_grad()
    def target_q_value_test(self, state, h, c, done, previous_action):
        """Debug helper (reference agent/r2d2.py:201-211): target-net Q
        values over one stored sequence."""
        s = self.frames_to_device(np.asarray(state)[None])
        pa = self.to_device(np.asarray(previous_action)[None], torch.int64)
        d = self.to_device(np.asarray(done)[None], torch.bool)
        h0 = self.to_device(np.asarray(h)[0][None], torch.float32)
        c0 = self.to_device(np.asarray(c)[0][None], torch.float32)
        q = self.target_model.unroll_sequence(s, pa, h0, c0, d)
        return q[0].float().cpu().numpy()

    @torch.no_grad()
    def get_actions_batch(self, states, h, c, previous_actions, epsilons):
        """Vectorized ε-greedy single step over E envs in ONE forward
        (vector actors, trainers/r2d2.py). Returns (actions [E], q_a [E],
        h' [E,H], c' [E,H])."""
        s = self.frames_to_device(np.asarray(states))
        pa = self.to_device(np.asarray(previous_actions), torch.int64)
        ht = self.to_device(np.asarray(h, dtype=np.float32), torch.float32)
        ct = self.to_device(np.asarray(c, dtype=np.float32), torch.float32)
        q, nh, nc = self.model.single_step(s, pa, ht, ct)
        qv = q.float().cpu().numpy()
        E = len(qv)
        greedy = qv.argmax(axis=1)
        rand = self.rng.integers(self.num_action, size=E)
        explore = self.rng.random(E) <= np.asarray(epsilons)
        actions = np.where(explore, rand, greedy).astype(np.int64)
        return (actions, qv[np.arange(E), actions].astype(np.float32),
                nh.float().cpu().numpy(), nc.float().cpu().numpy())

    @torch.no_grad()
    def get_action(self, state, h, c, previous_action, epsilon: float):
        """Epsilon-greedy single-step acting (reference agent/r2d2.py:166-186).
        Returns (action, q[action], h', c')."""
        s = self.frames_to_device(np.asarray(state)[None])
        pa = self.to_device(np.asarray([previous_action]), torch.int64)
        ht = self.to_device(np.asarray([h]), torch.float32)
        ct = self.to_device(np.asarray([c]), torch.float32)
        q, nh, nc = self.model.single_step(s, pa, ht, ct)
        qv = q[0].float().cpu().numpy()
        if self.rng.random() > epsilon:
            action = int(qv.argmax())
        else:
            action = int(self.rng.integers(self.num_action))
        return action, float(qv[action]), nh[0].float().cpu().numpy(), \
            nc[0].float().cpu().numpy()
