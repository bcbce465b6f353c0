"""hipGraph-captured PER learner step (Ape-X / R2D2).

One graph replays sample -> gather -> loss forward+backward -> priority
update; a second replays grad-gather (+ captured RCCL all-reduce in DP) +
the fused Adam update. Everything that changes across steps is read from
device memory at replay time: the segment tree and payloads (mutated by the
eager ingest between steps), beta / n_entries (device buffers the host
advances), the RNG state (philox offsets are graph-managed), and lr_t (a
1-element buffer).

Warmup, snapshot/restore and the optimizer graph come from
runtime/_capture.py; here the priority tree and beta join what is restored."""

from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch

from distributed_reinforcement_learning_amd.ops.conv_op import (
    join_wgrad_stream,
)
from distributed_reinforcement_learning_amd.runtime._capture import (
    CapturedStep, OptimizerGraph, run_on_side_stream,
    warmup_preserving_state,
)


class GraphedReplayStep(CapturedStep):
    def __init__(self, agent, memory, batch_size: int,
                 loss_fn: Callable[[Dict[str, torch.Tensor], torch.Tensor],
                                   Tuple[torch.Tensor, torch.Tensor]],
                 warmup_iters: int = 3):
        assert agent.device.type == "cuda"
        self.agent = agent
        self.memory = memory
        self.batch_size = batch_size
        self._loss_fn = loss_fn
        self._steps = 0
        self.lr_buf = torch.zeros(1, dtype=torch.float32,
                                  device=agent.device)

        def _iter():
            rows, idxs, w = memory.sample_static(batch_size)
            b = memory.gather(rows)
            loss, td = loss_fn(b, w)
            loss.backward()
            join_wgrad_stream()  # side-stream conv wgrads (capture-safe)
            memory.update_batch(idxs, td)
            return loss.detach(), td

        opt = agent.optimizer
        snap_beta = memory.beta
        warmup_preserving_state(opt, _iter, warmup_iters, self.lr_buf,
                                extra=(memory.tree,))
        memory.beta = snap_beta
        memory.beta_buf.fill_(snap_beta)

        self.g_main = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_main):
            self.loss, self.td = _iter()
        opt.build_gather_table()
        self._opt = OptimizerGraph(agent, self.lr_buf, self.g_main.pool())

    REBUILD_EVERY = 2048  # steps between interior-sum drift repairs

    def step(self) -> torch.Tensor:
        """One sample+train+update step; never syncs. Returns the loss
        TENSOR (float() it only at logging cadence)."""
        self._steps += 1
        if self._steps % self.REBUILD_EVERY == 0:
            # eager, between replays: repair float32 tree drift
            self.memory.rebuild()
        self._opt.begin_step()
        self.memory.advance_beta()
        self.g_main.replay()
        self._opt.replay()
        self.agent.global_step += 1
        return self.loss


class GraphedTdScore:
    """hipGraph-captured ingest-side TD scoring (Ape-X get_td_error / R2D2
    get_td_error_batch): arriving unrolls have a fixed shape, and the
    no-grad scoring forward is ~half the learner loop's eager launches.
    ``score_fn(inputs) -> td tensor`` must be pure no-grad compute over the
    static input buffers."""

    def __init__(self, agent, example: Dict[str, torch.Tensor],
                 score_fn: Callable[[Dict[str, torch.Tensor]],
                                    torch.Tensor]):
        assert agent.device.type == "cuda"
        self.inputs = {k: torch.zeros_like(v) for k, v in example.items()}
        self._score_fn = score_fn

        def warm():
            for _ in range(2):
                score_fn(self.inputs)

        run_on_side_stream(warm)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.td = score_fn(self.inputs)

    def score(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Copies ``batch`` into the static buffers, replays, and returns
        the TD tensor (plus self.inputs holds the staged batch — feed BOTH
        straight into GpuMemory.add_batch)."""
        for k, dst in self.inputs.items():
            dst.copy_(batch[k], non_blocking=True)
        self.graph.replay()
        return self.td


class GraphedTrainStep(CapturedStep):
    """hipGraph-captured plain learner step (A3C flavor): static input
    buffers -> loss forward+backward as one graph, grad-gather (+ captured
    RCCL all-reduce in DP) + fused optimizer as a second, built on
    runtime/_capture.py like GraphedReplayStep."""

    def __init__(self, agent, example: Dict[str, torch.Tensor],
                 loss_fn: Callable[[Dict[str, torch.Tensor]],
                                   Tuple[torch.Tensor, ...]],
                 warmup_iters: int = 3):
        assert agent.device.type == "cuda"
        self.agent = agent
        self._loss_fn = loss_fn
        self.inputs = {k: v.detach().clone() for k, v in example.items()}
        self.lr_buf = torch.zeros(1, dtype=torch.float32,
                                  device=agent.device)

        def _iter():
            losses = loss_fn(self.inputs)
            losses[-1].backward()
            join_wgrad_stream()  # side-stream conv wgrads (capture-safe)
            return tuple(x.detach() for x in losses[:-1])

        opt = agent.optimizer
        warmup_preserving_state(opt, _iter, warmup_iters, self.lr_buf)

        self.g_main = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_main):
            self.losses = _iter()
        opt.build_gather_table()
        self._opt = OptimizerGraph(agent, self.lr_buf, self.g_main.pool())

    def step(self, batch: Dict[str, torch.Tensor]):
        """Copy batch into the static inputs and replay; returns the loss
        TENSORS plus this step's lr (floats only at logging cadence)."""
        for k, dst in self.inputs.items():
            dst.copy_(batch[k], non_blocking=True)
        lr = self._opt.begin_step()
        self.g_main.replay()
        self._opt.replay()
        self.agent.global_step += 1
        return self.losses + (lr,)
