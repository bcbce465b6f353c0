"""Capture scaffold shared by the graph-captured learner steps
(GraphedImpalaStep, GraphedReplayStep, GraphedTrainStep); nothing here knows
an algorithm.

Snapshot/restore discipline: hipGraph capture wants a few eager iterations
first (lazy allocations, autotuning, communicator setup), and those are real
train steps. So the weights, the fp32 master and the optimizer state (plus
whatever device tensors the caller names) are cloned before the warmup, the
warmup runs on a side stream with lr_buf still zero, and everything is copied
back before the first capture: building a step class never perturbs training.

The optimizer graph is captured last, into the pool of the caller's first
graph, after build_gather_table() has recorded where backward leaves the
scattered grads.
"""

from __future__ import annotations

import os
from typing import Callable, Sequence

import torch

from distributed_reinforcement_learning_amd.parallel.dist import (
    handle_capture_failure, is_distributed, world_size,
)


def run_on_side_stream(fn: Callable[[], object]) -> None:
    """Run ``fn`` on a fresh stream ordered after the current one, join it
    back and synchronize (capture needs a quiet device)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def warmup_preserving_state(opt, iter_fn: Callable[[], object],
                            warmup_iters: int, lr_buf: torch.Tensor,
                            extra: Sequence[torch.Tensor] = ()) -> None:
    """``warmup_iters`` eager forward+backward+update iterations that leave
    no trace: see the module docstring. ``extra`` names further device
    tensors ``iter_fn`` mutates (the replay's priority tree)."""
    # scatter-grad mode: backward ASSIGNS grads (no per-param
    # AccumulateGrad adds); one gather kernel packs them (ops/optim.py)
    opt.enable_scatter_grads()
    live = [opt.flat_params, *opt._state_tensors().values(), *extra]
    if opt.mixed:
        live.append(opt.master)
    snap = [t.detach().clone() for t in live]

    def warm():
        for _ in range(warmup_iters):
            iter_fn()
            opt.gather_grads_eager()
            opt.step_tensor_lr(lr_buf)

    run_on_side_stream(warm)
    with torch.no_grad():
        for t, s in zip(live, snap):
            t.copy_(s)
        opt.flat_grads.zero_()


class OptimizerGraph:
    """The captured optimizer step: one-kernel grad gather (+ world > 1:
    captured RCCL all-reduce) + fused clip and update reading ``lr_buf``."""

    def __init__(self, agent, lr_buf: torch.Tensor, pool):
        self.agent = agent
        self.lr_buf = lr_buf
        opt = agent.optimizer
        self.distributed = is_distributed() and (
            world_size() > 1 or bool(os.environ.get("DRLA_FORCE_DIST_GRAPH")))
        self.eager_reduce = False
        self.graph = torch.cuda.CUDAGraph()
        if self.distributed:
            # capture gather + RCCL all-reduce + update as ONE graph
            # (NCCL/RCCL collectives are capture-legal and every rank
            # replays in lockstep). Capture failure is FATAL by default —
            # a silent per-rank eager fallback deadlocks the lockstep
            # replay; parallel/dist.py decides (DRLA_ALLOW_EAGER_REDUCE).
            try:
                # prime the communicator outside capture
                agent.reduce_gradients()
                torch.cuda.synchronize()
                with torch.cuda.graph(self.graph, pool=pool):
                    opt.gather_grads()
                    agent.reduce_gradients()
                    opt.step_tensor_lr(lr_buf)
            except Exception as exc:
                handle_capture_failure(exc)
                self.eager_reduce = True
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, pool=pool):
                    opt.step_tensor_lr(lr_buf)
        else:
            with torch.cuda.graph(self.graph, pool=pool):
                # single-GPU: the gather rides inside the optimizer graph
                opt.gather_grads()
                opt.step_tensor_lr(lr_buf)

    def begin_step(self) -> float:
        """Host side of a step, before any replay: this step's scheduled lr
        goes into ``lr_buf`` in the optimizer's own form (lr_t_for) and is
        returned as scheduled. Never blocks."""
        agent, opt = self.agent, self.agent.optimizer
        lr = agent.lr_at(agent.global_step)
        opt.step_count += 1
        self.lr_buf.fill_(opt.lr_t_for(lr, opt.step_count))
        return lr

    def replay(self) -> None:
        if self.eager_reduce:
            self.agent.optimizer.gather_grads()
            self.agent.reduce_gradients()
        self.graph.replay()


class CapturedStep:
    """Base of the step classes: what callers read off a step about its
    optimizer graph (``self._opt``, an OptimizerGraph)."""

    g_opt = property(lambda self: self._opt.graph)
    _distributed = property(lambda self: self._opt.distributed)
    _eager_reduce = property(lambda self: self._opt.eager_reduce)
