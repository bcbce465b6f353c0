"""hipGraph-captured IMPALA train step.

The eager step is launch-bound on MI355X: ~300 kernel dispatches per step,
~1.9 ms GPU-busy inside a ~4 ms wall step (rocprof r01,
profiles/impala_bench_r01_kernels.md). Capturing the
normalize -> unroll -> V-trace -> backward -> fused-optimizer pipeline into
hipGraphs cuts the replay to ~1.3 ms GPU (measured, profiles/ triage r03).

Two measured host-side traps shape this class (gpu_triage.py r03/r04):
  * a mid-flight ``.item()`` on the loss tensors costs ~11 ms (blocking-sync
    wake latency), so losses are NOT read per step — ``last_losses()`` reads
    them on demand (logging cadence), and the steady-state loop never syncs;
  * staging numpy -> pinned is a ~4 ms single-thread memcpy, so callers that
    can produce data straight into ``self.pinned`` (the trajectory queue, the
    bench pool) skip it entirely.

Step structure (three graphs + a copy stream). Every static input exists
twice; a device slot word says which set a replay reads:
  host:     one launch writes the decayed LR and the slot word (never blocks)
  copy str: the NEXT batch's pinned -> static-input H2D into the OTHER set,
            queued before graph 1 and ordered after the previous step's
            graph 1 (that set's last reader), so the 19.4 MB upload has the
            whole step to hide under. The four forward kernels that read
            static inputs take the set from the slot word
            (ops/input_slots.py, drla_slot_base)
  graph 1:  normalize frames, batched unroll (bf16), fused V-trace losses
            (forward only). Every read of a static input happens INSIDE
            graph 1:
            each forward kernel that reads a backward-read input (conv-l1:
            state; embed MLP: previous_action; LSTM tail: initial_c;
            V-trace loss: action) stashes a copy in passing, no clone
            launches. The embed and heads forwards also emit the W^T their
            backwards need and the heads forward zeroes the backward's
            atomics workspace, so graph 2 starts without pack or fill
            launches; the V-trace loss sums take no zero-fill either
            (ticketed fixed-order reduction)
  graph 2:  backward (autograd ASSIGNS scatter-mode grads — no
            AccumulateGrad adds)
  graph 3:  one-kernel grad gather + (world > 1: CAPTURED RCCL all-reduce)
            + fused global-norm clip + RMSProp update reading the LR buffer
  host:     record consume-event; losses stay on-device until
            last_losses()

The eager warmup, its snapshot/restore of training state and the capture of
graph 3 are shared with the other learners: runtime/_capture.py.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from distributed_reinforcement_learning_amd import ops as _ops
from distributed_reinforcement_learning_amd.ops import conv_op, input_slots
from distributed_reinforcement_learning_amd.runtime._capture import (
    CapturedStep, OptimizerGraph, warmup_preserving_state,
)


class GraphedImpalaStep(CapturedStep):
    def __init__(self, agent, batch_size: int, warmup_iters: int = 3):
        assert agent.device.type == "cuda", "graphed step needs a GPU"
        # u8 conv layers stash their input in-kernel from here on: the
        # overlapped H2D rewrites the static input buffers during the
        # backward, and the l1 wgrad re-reads the input (see _fwd)
        conv_op.STASH_INPUTS = True
        self.agent = agent
        B, T = batch_size, agent.trajectory
        A, H = agent.num_action, agent.lstm_hidden_size
        HH, WW, C = agent.input_shape
        dev = agent.device

        def z(shape, dtype):
            # two sets of every static input: the replay reads the set the
            # device slot word names while the copy stream fills the other
            return torch.zeros((2,) + tuple(shape), dtype=dtype, device=dev)

        self._pairs: Dict[str, torch.Tensor] = {
            "state": z((B, T, HH, WW, C), torch.uint8),
            "reward": z((B, T), torch.float32),
            # int32: the fused V-trace kernel consumes i32 and the ring
            # stores i32 — an i64 static input cost one [B,T] cast per
            # replay (actions feed nothing else in the captured step)
            "action": z((B, T), torch.int32),
            "done": z((B, T), torch.bool),
            "behavior_policy": z((B, T, A), torch.float32),
            "previous_action": z((B, T), torch.int64),
            "initial_h": z((B, T, H), torch.float32),
            "initial_c": z((B, T, H), torch.float32),
        }
        self._sets = [{k: v[s] for k, v in self._pairs.items()}
                      for s in (0, 1)]
        # today's shapes and dtypes: views of set 0 (their storages cover
        # both sets)
        self.inputs: Dict[str, torch.Tensor] = self._sets[0]
        self._slot_word = torch.zeros(1, dtype=torch.int32, device=dev)
        self._cur = 0  # the set the next replay reads
        self.pinned: Dict[str, torch.Tensor] = {
            k: torch.empty_like(v, device="cpu").pin_memory()
            for k, v in self.inputs.items()
        }
        self.lr_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self._consumed = torch.cuda.Event()
        self._consumed.record()
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        self._fwd_done = torch.cuda.Event()
        self._copy_stream = torch.cuda.Stream()
        self._primed = False
        self._last_lr = 0.0

        opt = agent.optimizer
        # the op wrappers hand the slot word and each field's set distance
        # to the four forward kernels that read static inputs, for the
        # warmup and the captures below (slot word 0 throughout)
        input_slots.register(self._slot_word, self._pairs)
        try:
            self._warmup_and_capture(agent, opt, dev, warmup_iters)
            # a field that reached something other than the four
            # slot-aware kernels (a model on a torch fallback path) is read
            # from set 0 whatever the word says: such a step keeps ONE set
            # and the upload-after-forward ordering
            self._double = not input_slots.unseen()
        finally:
            input_slots.clear()

    def _warmup_and_capture(self, agent, opt, dev, warmup_iters):
        warmup_preserving_state(opt, self._fwd_bwd, warmup_iters, self.lr_buf)

        # ---- capture ------------------------------------------------------
        # forward and backward are SEPARATE graphs, and _fwd() confines
        # every input read to graph 1 (in-kernel stashes of the
        # backward-read fields): a set is free for the next upload as soon
        # as the forward that read it is done. The upload is 19.4 MB in 8
        # copies at B=32, T=20, measured 445 us first start to last end, the
        # frames alone 329 us (profiles/impala_step_timeline_r04_parent.md);
        # it no longer fits under the backward alone.
        self.g_fwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_fwd):
            self._total, self.losses = self._fwd()
        # preallocated backward seed: backward() without an explicit
        # gradient fills a scalar ones(()) INSIDE the graph (one fill
        # kernel per replay)
        self._bwd_seed = torch.ones((), device=dev)
        self.g_bwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_bwd, pool=self.g_fwd.pool()):
            # retain_graph: the saved tensors live in the shared capture
            # pool and are rewritten by every g_fwd replay
            self._total.backward(gradient=self._bwd_seed,
                                 retain_graph=True)
            # join the side-stream conv wgrads (ops/conv_op.py) so the
            # capture region ends with a single ordered stream
            conv_op.join_wgrad_stream()
        # .grad now holds capture-pool tensors at replay-stable addresses
        opt.build_gather_table()
        self._opt = OptimizerGraph(agent, self.lr_buf, self.g_fwd.pool())

    def _fwd(self):
        agent = self.agent
        i = self.inputs
        # The overlapped H2D upload (copy stream) is ordered only after
        # the FORWARD, but four inputs feed backward kernels (conv-l1
        # wgrad: state; embed scatter: previous_action; V-trace bwd:
        # action; LSTM tail bwd: initial_c). Under conv_op.STASH_INPUTS
        # the forward kernel that reads each of them writes a copy in
        # passing and the backward consumes that copy, so every read of a
        # static buffer happens before the upload barrier without a clone
        # launch (a wrapper on a non-fused fallback clones for itself).
        s = agent.prepare_frames(i["state"])
        pi_loss, baseline_loss, entropy, total = agent.compute_losses(
            s, i["reward"], i["action"], i["done"], i["behavior_policy"],
            i["previous_action"], i["initial_h"], i["initial_c"])
        return total, (pi_loss.detach(), baseline_loss.detach(),
                       entropy.detach())

    def _fwd_bwd(self) -> Tuple[torch.Tensor, ...]:
        agent = self.agent
        if not agent.optimizer.scatter:
            agent.optimizer.flat_grads.zero_()
        total, losses = self._fwd()
        total.backward()
        return losses

    # -- input staging -------------------------------------------------------

    def stage_to_pinned(self, batch: Dict[str, np.ndarray]) -> None:
        """Host-side memcpy of a numpy batch into the pinned buffers
        (~4 ms for the reference shape; skip by filling self.pinned
        directly, e.g. TrajectoryQueue.sample_batch_into)."""
        for k, pin in self.pinned.items():
            pin.copy_(torch.as_tensor(np.asarray(batch[k])))

    def upload_inputs(self, src: Optional[Dict[str, torch.Tensor]] = None
                      ) -> None:
        """Synchronous-path upload (priming / non-pipelined callers), into
        the set the coming replay reads."""
        self._consumed.synchronize()
        src = src or self.pinned
        # a pipelined upload into this set may still be in flight
        torch.cuda.current_stream().wait_event(self._uploaded)
        for k, dst in self._sets[self._cur].items():
            dst.copy_(src[k], non_blocking=True)
        self._uploaded.record()
        self._primed = True

    def _upload_overlapped(self, src: Dict[str, torch.Tensor],
                           into: int) -> None:
        """Queue the NEXT step's H2D on the copy stream into set ``into``,
        ordered after the PREVIOUS call's forward, the last reader of that
        set: the upload runs under this call's forward, backward and
        optimizer."""
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(self._fwd_done)
            for k, dst in self._sets[into].items():
                dst.copy_(src[k], non_blocking=True)
            self._uploaded.record(self._copy_stream)

    def wait_pinned_free(self) -> None:
        """Block until the last async H2D has finished reading the pinned
        staging — call before overwriting self.pinned."""
        self._uploaded.synchronize()

    # -- stepping ------------------------------------------------------------

    def step(self, batch: Optional[Dict[str, np.ndarray]] = None,
             pinned_src: Optional[Dict[str, torch.Tensor]] = None
             ) -> Tuple[torch.Tensor, ...]:
        """Run one full train step. Sources, in priority order: ``batch``
        (numpy, staged through self.pinned), ``pinned_src`` (caller-owned
        pinned tensors), or self.pinned already filled. Never syncs; returns
        the loss TENSORS (device). Read them with last_losses() at logging
        cadence.

        Pipelined upload (pinned paths only): the FIRST call uploads
        synchronously; later calls replay on the set uploaded during the
        PREVIOUS call's step and queue this call's data into the other set
        stream — one-batch latency, which the asynchronous actor-learner
        loop does not notice (losses/scalars lag one batch). The numpy
        ``batch=`` path stays strictly synchronous."""
        agent = self.agent
        main = torch.cuda.current_stream()
        if batch is not None:
            # numpy path keeps same-batch semantics (no pipelining) — the
            # eager-parity test and train()-style callers rely on it
            self.stage_to_pinned(batch)
            self.upload_inputs()
            src = None
        else:
            src = pinned_src if pinned_src is not None else self.pinned
            if not self._primed:
                self.upload_inputs(src)
                src = None
        main.wait_event(self._uploaded)
        s = self._cur
        # host side of the step (OptimizerGraph.begin_step's part, plus the
        # slot word, in one launch): this replay reads set s
        opt = agent.optimizer
        self._last_lr = agent.lr_at(agent.global_step)
        opt.step_count += 1
        _ops.require_ext()._set_lr_slot(
            self.lr_buf, self._slot_word,
            float(opt.lr_t_for(self._last_lr, opt.step_count)), s)
        if src is not None and self._double:
            # this call's H2D goes into the other set, queued BEFORE the
            # forward replay; the replay below consumes the PREVIOUS
            # call's upload (one-batch pipeline)
            self._upload_overlapped(src, 1 - s)
            self._cur = 1 - s
        self.g_fwd.replay()
        self._fwd_done.record(main)
        if src is not None and not self._double:
            # one set: its only reader is the forward just replayed
            self._upload_overlapped(src, s)
        self.g_bwd.replay()
        self._opt.replay()
        self._consumed.record()
        agent.global_step += 1
        agent.num_env_frames += int(np.prod(self.inputs["reward"].shape))
        return self.losses

    def last_losses(self) -> Tuple[float, float, float, float]:
        """(pi_loss, baseline_loss, entropy, lr) of the most recent completed
        step — syncs the device."""
        pi, bl, ent = (float(x) for x in self.losses)
        return pi, bl, ent, self._last_lr
