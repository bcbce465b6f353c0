#!/usr/bin/env python3
"""Driver benchmark entry. Default (the driver contract): IMPALA deep-conv
learner, env-frames/sec (whole job).

BASELINE.json metric: "learner env-frames/sec (whole node), IMPALA deep-conv
84x84x4 at 1/2/4/8 MI355X". One train step consumes B*T = 32*20 = 640 env
frames per rank (reference config.json:130,136; global-step accounting at
agent/impala.py:95-100). Weak scaling: per-GPU batch fixed at 32, global
batch = 32*N.

Each timed step is the FULL learner update on synthetic uint8 frames with
random-init weights: H2D upload of the uint8 batch, on-device /255 normalize,
batched conv+LSTM+heads forward (bf16), V-trace, backward, flat all-reduce
(N>1, RCCL), fused global-norm-clip + RMSProp update. Nothing is cached or
skipped; data is synthetic because this image has no network (BASELINE.json
mandates synthetic frames).

--algo {impala,apex,r2d2} additionally covers BASELINE configs #3/#4
(VERDICT r1 item 3): the Ape-X and R2D2 runs time the full
sample -> gather -> loss fwd+bwd -> priority-update -> optimizer replay
iteration against a device-resident PER shard (reference loops
train_apex.py:124-155 / train_r2d2.py:122-162). R2D2 defaults to the
BASELINE shape seq_len=80 / burn_in=40 (config #4); --seq-len 15
--burn-in 7 reproduces the reference config.json:88-101 shape.

A plain run does only what the headline figure needs: setup, warmup, the
timed steps, the result line. --dump-outputs DIR additionally writes what the
last timed step computed (for build-vs-build comparison); --full is where
any secondary measurement belongs.

Launch (driver contract):
    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_reinforcement_learning_amd.utils import tunableop
tunableop.enable()  # shipped hipBLASLt tuning table (+3.5%; must precede torch GEMMs)

import numpy as np
import torch


def parse_args(argv):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--algo", default="impala",
                   choices=["impala", "apex", "r2d2"],
                   help="impala = the driver's headline metric; apex/r2d2 "
                        "cover BASELINE configs #3/#4 (PER replay step)")
    p.add_argument("--batch", type=int, default=None,
                   help="per-rank batch (reference: impala/apex 32, "
                        "r2d2 16)")
    p.add_argument("--trajectory", type=int, default=20)
    p.add_argument("--num-action", type=int, default=18)
    p.add_argument("--lstm", type=int, default=256)
    p.add_argument("--seq-len", type=int, default=80,
                   help="r2d2 sequence length (BASELINE config #4: 80; "
                        "reference config.json: 15)")
    p.add_argument("--burn-in", type=int, default=40,
                   help="r2d2 burn-in (BASELINE config #4: 40; "
                        "reference: 7)")
    p.add_argument("--pool", type=int, default=8,
                   help="distinct synthetic batches cycled through")
    p.add_argument("--no-graph", action="store_true",
                   help="disable hipGraph capture (eager launches)")
    p.add_argument("--model", default="deep_conv",
                   choices=["deep_conv", "resnet"],
                   help="flagship (deep_conv) or IMPALA ResNet-large "
                        "(BASELINE config #5, stresses the all-reduce)")
    p.add_argument("--min-warm-s", type=float, default=1.25,
                   help="minimum UNTIMED busy time before the timed region: "
                        "keeps stepping past --warmup until the GPU has run "
                        "this long, so short-run contracts (K=20, W=5) "
                        "measure boost-clock steady state, not DVFS ramp")
    p.add_argument("--step-times", action="store_true",
                   help="print per-step GPU ms to stderr (diagnostics)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the LAST timed "
                        "step computed (losses, updated parameters, "
                        "gradients) as DIR/<name>.npy (float32). That "
                        "step is made to start from the freshly seeded "
                        "training state on a fixed batch, so two runs with "
                        "the same arguments agree output for output to "
                        "rounding (--algo impala only)")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement/check the "
                        "benchmark carries besides its headline figure. A "
                        "plain run does setup, warmup, the timed steps and "
                        "the result line only; anything beyond that belongs "
                        "behind this flag (currently there is none)")
    args = p.parse_args(argv)
    if args.dump_outputs and args.algo != "impala":
        p.error("--dump-outputs is implemented for --algo impala only")
    return args


# at most 64 MB of float32 per --dump-outputs directory, split over the two
# large arrays (params, grads); the three losses are scalars
DUMP_MAX_ELEMS = 7_000_000


class ImpalaState:
    """Snapshot/restore of everything a train step mutates, so the step a
    --dump-outputs run writes out starts from a reproducible state. Two
    things make the state after many updates differ between runs: the
    clock-priming loop in run_timed() runs for a fixed TIME, i.e. a
    machine-dependent number of updates, and the kernels' atomic
    accumulation order puts last-bit noise into every gradient, which
    training amplifies (measured: 4e-7 relative on the parameters after one
    update, a few percent after 50)."""

    def __init__(self, agent):
        self.agent = agent

    def _tensors(self):
        opt = self.agent.optimizer
        t = {"flat_params": opt.flat_params, "master": opt.master}
        t.update(opt._state_tensors())
        return t

    def save(self):
        a = self.agent
        self._snap = {k: v.detach().clone()
                      for k, v in self._tensors().items()}
        self._counters = (a.optimizer.step_count, a.global_step,
                          a.num_env_frames)

    def restore(self):
        a = self.agent
        with torch.no_grad():
            for k, v in self._tensors().items():
                v.copy_(self._snap[k])
        (a.optimizer.step_count, a.global_step,
         a.num_env_frames) = self._counters


def dump_outputs(out_dir: str, agent, losses) -> None:
    """Write the last timed step's results as float32 .npy files: the three
    losses, the updated fp32 parameters and the (gathered, pre-clip)
    gradients. Arrays above DUMP_MAX_ELEMS are reduced to a fixed seeded
    sample of their elements."""
    os.makedirs(out_dir, exist_ok=True)
    opt = agent.optimizer
    out = {
        "pi_loss": losses[0], "baseline_loss": losses[1],
        "entropy": losses[2], "params": opt.master, "grads": opt.flat_grads,
    }
    for name, v in out.items():
        arr = (v.detach().float().cpu().numpy() if torch.is_tensor(v)
               else np.asarray(v)).astype(np.float32).reshape(-1)
        if arr.size > DUMP_MAX_ELEMS:
            idx = np.random.default_rng(0).choice(
                arr.size, DUMP_MAX_ELEMS, replace=False)
            idx.sort()
            arr = arr[idx]
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def run_timed(step, args, world: int, have_gpu: bool, device: str,
              state=None) -> float:
    """Warmup (+ untimed clock priming), then time EXACTLY args.steps steps
    bracketed by barrier+synchronize; returns MAX-over-ranks elapsed
    seconds. ``step(i)`` must run one full train step.

    ``state`` (save()/restore(), --dump-outputs runs only): the seeded
    initial training state is saved before the first step and put back
    right before the LAST timed step, and the batch index of the timed
    steps is fixed, so that step computes one update from bit-identical
    weights on the same batch in every run. The restore is three
    stream-ordered device copies (~40 MB, tens of microseconds) inside the
    timed region of such runs only; plain runs are untouched."""

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if have_gpu:
            torch.cuda.synchronize()

    t_warm0 = time.perf_counter()
    i = 0
    if state is not None:
        state.save()
    for _ in range(args.warmup):
        step(i)
        i += 1
    if have_gpu and args.min_warm_s > 0:
        # clock priming, still untimed: a fresh MI355X ramps its boost
        # clocks over O(100 ms) of sustained load; W=5 warmup steps
        # (~4 ms of GPU work) leave the first timed steps measuring the
        # DVFS ramp (BENCH_r01: 1.07 ms/step at K=20 vs 0.71 steady)
        torch.cuda.synchronize()
        while time.perf_counter() - t_warm0 < args.min_warm_s:
            step(i)
            i += 1
    barrier_sync()
    if state is not None:
        # the priming loop above advanced i by a machine-dependent count:
        # restart the batch index where the warmup left it (the absorbing
        # step below queues batch i for the pipelined upload, which the
        # first timed step then consumes)
        i = args.warmup
    if have_gpu:
        # the FIRST replay after a full device sync intermittently costs
        # ~1-2 ms extra (driver wake-up); absorb it untimed so the short
        # timed window measures steady state
        step(i)
        i += 1
    barrier_sync()

    events = None
    if args.step_times and have_gpu:
        events = [torch.cuda.Event(enable_timing=True)
                  for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    if events:
        events[0].record()
    for k in range(args.steps):
        if state is not None and k == args.steps - 1:
            state.restore()  # stream-ordered before the step below
        step(i)
        i += 1
        if events:
            events[k + 1].record()
    barrier_sync()
    dt = time.perf_counter() - t0
    if events:
        times = [events[k].elapsed_time(events[k + 1])
                 for k in range(args.steps)]
        print("step_ms=" + json.dumps([round(x, 3) for x in times]),
              file=sys.stderr, flush=True)

    if world > 1:
        dt_t = torch.tensor([dt], dtype=torch.float64,
                            device=device if have_gpu else "cpu")
        torch.distributed.all_reduce(dt_t,
                                     op=torch.distributed.ReduceOp.MAX)
        dt = float(dt_t.item())
    return dt


def emit(rank: int, metric: str, value: float, unit: str, world: int,
         args, dt: float, config: dict, dtype: str) -> None:
    if rank != 0:
        return
    print(json.dumps({
        "metric": metric,
        "value": value,
        "unit": unit,
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": "synthetic",
        "config": config,
    }), flush=True)


# --------------------------------------------------------------- impala --

def bench_impala(args, rank, world, local_rank, have_gpu, device):
    from distributed_reinforcement_learning_amd.agents import impala

    B = args.batch or 32
    T, A, H = args.trajectory, args.num_action, args.lstm
    agent = impala.Agent(
        trajectory=T, input_shape=[84, 84, 4], num_action=A,
        lstm_hidden_size=H, discount_factor=0.99, start_learning_rate=6e-4,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", device=device, seed=1234 + rank,
        model_arch=args.model)
    if world > 1:
        from distributed_reinforcement_learning_amd.parallel.dist import (
            broadcast_module,
        )
        broadcast_module(agent.model)
        agent.setup_all_reduce()

    # synthetic trajectory batches, shaped exactly like the queue's output
    rng = np.random.default_rng(99 + rank)
    pool = []
    for _ in range(args.pool):
        pool.append(dict(
            state=rng.integers(0, 255, (B, T, 84, 84, 4), dtype=np.uint8),
            reward=rng.normal(size=(B, T)).astype(np.float32),
            action=rng.integers(0, A, (B, T)).astype(np.int32),
            done=(rng.random((B, T)) < 0.02),
            behavior_policy=np.full((B, T, A), 1.0 / A, dtype=np.float32),
            previous_action=rng.integers(0, A, (B, T)).astype(np.int32),
            initial_h=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
            initial_c=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
        ))

    graphed = None
    pinned_pool = None
    if have_gpu and not args.no_graph:
        from distributed_reinforcement_learning_amd.runtime import (
            GraphedImpalaStep,
        )
        graphed = GraphedImpalaStep(agent, B)
        # data sits in pinned host memory, as the production ingest path
        # delivers it (TrajectoryQueue.sample_batch_into); the per-step H2D
        # upload stays inside the timed region.
        pinned_pool = []
        for b in pool:
            pinned_pool.append({
                k: torch.as_tensor(np.asarray(v)).to(
                    graphed.pinned[k].dtype).pin_memory()
                for k, v in b.items()})

    last = [None]  # what the most recent step returned to its caller

    def step(i: int):
        if graphed is not None:
            last[0] = graphed.step(
                pinned_src=pinned_pool[i % len(pinned_pool)])
            return last[0]
        b = pool[i % len(pool)]
        last[0] = agent.train(
            state=b["state"], reward=b["reward"], action=b["action"],
            done=b["done"], behavior_policy=b["behavior_policy"],
            previous_action=b["previous_action"], initial_h=b["initial_h"],
            initial_c=b["initial_c"])
        return last[0]

    dt = run_timed(step, args, world, have_gpu, device,
                   state=ImpalaState(agent) if args.dump_outputs else None)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, agent, last[0])
    frames = args.steps * B * T * world
    emit(rank,
         "learner env-frames/sec (whole node), IMPALA deep-conv 84x84x4",
         frames / dt, "frames/s", world, args, dt,
         {
             "model": ("impala deep-conv 84x84x4 + LSTM256 V-trace"
                       if args.model == "deep_conv"
                       else "impala resnet-large 84x84x4 + LSTM256 V-trace"),
             "global_batch": B * world,
             "seq_len": T,
             "parallelism": f"dp{world}",
             "num_action": A,
             "frames_per_step_per_rank": B * T,
         },
         "bf16" if have_gpu else "fp32")


# ----------------------------------------------------------- apex/r2d2 --

def _dist_setup(agent, world):
    if world > 1:
        from distributed_reinforcement_learning_amd.parallel.dist import (
            broadcast_module,
        )
        broadcast_module(agent.model)
        if getattr(agent, "target_model", None) is not None:
            broadcast_module(agent.target_model)
        agent.setup_all_reduce()


def bench_apex(args, rank, world, local_rank, have_gpu, device):
    """BASELINE config #3: Ape-X DQN, PER shard on-GPU, DP learners.
    Timed region = the reference's PER train iteration
    (train_apex.py:124-155): stratified sample -> payload gather -> fused
    double-DQN loss fwd+bwd -> priority update -> all-reduce (N>1) ->
    fused Adam — one hipGraph replay pair per step."""
    from distributed_reinforcement_learning_amd.agents import apex as apex_agent

    B = args.batch or 32
    H, W, C = 84, 84, 4
    A = 4  # reference config.json apex model_output (Breakout)
    T = 32
    agent = apex_agent.Agent(
        input_shape=[H, W, C], num_action=A, discount_factor=0.99,
        gradient_clip_norm=40.0, reward_clipping="abs_one",
        start_learning_rate=1e-4, end_learning_rate=0.0,
        learning_frame=10 ** 14, device=device, build_optimizer=True,
        seed=3 + rank)
    _dist_setup(agent, world)
    rng = np.random.default_rng(7 + rank)

    def synth_unroll():
        return {
            "state": rng.integers(0, 255, (T, H, W, C), dtype=np.uint8),
            "next_state": rng.integers(0, 255, (T, H, W, C),
                                       dtype=np.uint8),
            "previous_action": rng.integers(0, A, T).astype(np.int32),
            "action": rng.integers(0, A, T).astype(np.int32),
            "reward": rng.normal(size=T).astype(np.float32),
            "done": (rng.random(T) < 0.02),
        }

    if have_gpu:
        from distributed_reinforcement_learning_amd.replay.gpu_memory import (
            GpuMemory,
        )
        from distributed_reinforcement_learning_amd.runtime import (
            GraphedReplayStep,
        )
        mem = GpuMemory(100_000, fields={
            "state": ((H, W, C), torch.uint8),
            "next_state": ((H, W, C), torch.uint8),
            "previous_action": ((), torch.int32),
            "action": ((), torch.int32),
            "reward": ((), torch.float32),
            "done": ((), torch.bool)}, device=device, seed=3 + rank)
        for _ in range(40):
            u = {k: torch.as_tensor(v).to(device)
                 for k, v in synth_unroll().items()}
            td = agent.get_td_error(
                u["state"], u["next_state"], u["previous_action"],
                u["action"], u["reward"], u["done"], as_tensor=True)
            mem.add_batch(td, u)

        def loss_fn(b, w):
            return agent.compute_distributed_loss(
                agent.frames_to_device(b["state"]),
                agent.frames_to_device(b["next_state"]),
                b["previous_action"].long(), b["action"].long(),
                b["reward"], b["done"], w)

        graphed = GraphedReplayStep(agent, mem, B, loss_fn)

        def step(i: int):
            graphed.step()
        dtype = "bf16"
    else:
        # CPU fallback (contract tests only): same sample -> train ->
        # priority-update loop against the float64 CPU Memory
        from distributed_reinforcement_learning_amd.replay.memory import (
            Memory,
        )
        mem = Memory(10_000, seed=3 + rank)
        for _ in range(4):
            u = synth_unroll()
            for t in range(T):
                mem.add(float(rng.random()),
                        {k: v[t] for k, v in u.items()})

        def step(i: int):
            samples, idxs, w = mem.sample(B)
            batch = {k: np.stack([s[k] for s in samples])
                     for k in samples[0]}
            _, td = agent.distributed_train(
                batch["state"], batch["next_state"],
                batch["previous_action"], batch["action"],
                batch["reward"], batch["done"], w)
            mem.update_batch(idxs, np.abs(td))
        dtype = "fp32"

    dt = run_timed(step, args, world, have_gpu, device)
    emit(rank,
         "Ape-X learner transitions/sec (whole node), PER replay step "
         "84x84x4 dueling double-DQN",
         args.steps * B * world / dt, "transitions/s", world, args, dt,
         {
             "model": "apex dueling double-DQN 84x84x4",
             "global_batch": B * world,
             "parallelism": f"dp{world}",
             "num_action": A,
             "replay": "GPU PER shard 1e5" if have_gpu else "CPU PER",
             "frames_per_step_per_rank": B,
         },
         dtype)


def bench_r2d2(args, rank, world, local_rank, have_gpu, device):
    """BASELINE config #4: R2D2 LSTM POMDP, burn-in=40 seq=80 (default;
    --seq-len 15 --burn-in 7 reproduces reference config.json:88-101).
    Timed region = the reference's recurrent PER train iteration
    (train_r2d2.py:122-162): sample -> gather -> burn-in recompute +
    trained-window unroll fwd+bwd -> per-sequence priority update ->
    all-reduce (N>1) -> fused Adam."""
    from distributed_reinforcement_learning_amd.agents import r2d2 as r2d2_agent

    B = args.batch or 16
    L, BI = args.seq_len, args.burn_in
    H, W, C = 84, 84, 1
    A = 4
    LSTM = 64
    agent = r2d2_agent.Agent(
        seq_len=L, burn_in=BI, input_shape=[H, W, C], num_action=A,
        lstm_size=LSTM, discount_factor=0.997, start_learning_rate=1e-4,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        gradient_clip_norm=40.0, reward_clipping="abs_one", device=device,
        build_optimizer=True, seed=3 + rank)
    _dist_setup(agent, world)
    rng = np.random.default_rng(11 + rank)

    def synth_seqs(n):
        return {
            "state": rng.integers(0, 255, (n, L, H, W, C), dtype=np.uint8),
            "previous_action": rng.integers(0, A, (n, L)).astype(np.int32),
            "action": rng.integers(0, A, (n, L)).astype(np.int32),
            "reward": rng.normal(size=(n, L)).astype(np.float32),
            "done": (rng.random((n, L)) < 0.02),
            "initial_h": (rng.normal(size=(n, L, LSTM)) * 0.1
                          ).astype(np.float32),
            "initial_c": (rng.normal(size=(n, L, LSTM)) * 0.1
                          ).astype(np.float32),
        }

    if have_gpu:
        from distributed_reinforcement_learning_amd.replay.gpu_memory import (
            GpuMemory,
        )
        from distributed_reinforcement_learning_amd.runtime import (
            GraphedReplayStep,
        )
        mem = GpuMemory(100_000, fields={
            "state": ((L, H, W, C), torch.uint8),
            "previous_action": ((L,), torch.int32),
            "action": ((L,), torch.int32),
            "reward": ((L,), torch.float32),
            "done": ((L,), torch.bool),
            "initial_h": ((L, LSTM), torch.float32),
            "initial_c": ((L, LSTM), torch.float32)},
            device=device, seed=3 + rank)
        for _ in range(12):
            u = {k: torch.as_tensor(v).to(device)
                 for k, v in synth_seqs(4).items()}
            td = agent.get_td_error_batch(
                u["state"], u["previous_action"], u["action"],
                u["initial_h"][:, 0], u["initial_c"][:, 0], u["reward"],
                u["done"], as_tensor=True)
            mem.add_batch(td, u)

        def loss_fn(b, w):
            return agent.compute_sequence_loss(
                b["state"], b["previous_action"], b["action"],
                b["initial_h"][:, 0], b["initial_c"][:, 0], b["reward"],
                b["done"], w)

        graphed = GraphedReplayStep(agent, mem, B, loss_fn)

        def step(i: int):
            graphed.step()
        dtype = "bf16"
    else:
        from distributed_reinforcement_learning_amd.replay.memory import (
            Memory,
        )
        mem = Memory(1_000, seed=3 + rank)
        seqs = synth_seqs(8)
        for s in range(8):
            mem.add(float(rng.random()),
                    {k: v[s] for k, v in seqs.items()})

        def step(i: int):
            samples, idxs, w = mem.sample(B)
            batch = {k: np.stack([s[k] for s in samples])
                     for k in samples[0]}
            _, td = agent.train(
                batch["state"], batch["previous_action"], batch["action"],
                batch["initial_h"], batch["initial_c"], batch["reward"],
                batch["done"], w)
            mem.update_batch(idxs, np.abs(td))
        dtype = "fp32"

    dt = run_timed(step, args, world, have_gpu, device)
    emit(rank,
         "R2D2 learner sequences/sec (whole node), recurrent PER "
         f"seq={L} burn-in={BI} POMDP 84x84x1",
         args.steps * B * world / dt, "sequences/s", world, args, dt,
         {
             "model": f"r2d2 conv+LSTM{LSTM} dueling 84x84x1",
             "global_batch": B * world,
             "seq_len": L,
             "burn_in": BI,
             "parallelism": f"dp{world}",
             "num_action": A,
             "replay": ("GPU recurrent PER shard 1e5" if have_gpu
                        else "CPU PER"),
             "frames_per_step_per_rank": B * L,
         },
         dtype)


def main(argv=None) -> None:
    args = parse_args(argv)
    # benchmark robustness: if the distributed optimizer-graph capture
    # refuses on some stack, continue with the LOUD eager all-reduce
    # rather than killing the whole scaling run — the eager rank issues
    # the same collective sequence as a captured rank, so mixed modes
    # stay consistent (tests/test_gpu_dist.py keeps the strict fail-fast
    # to prove capture actually works)
    os.environ.setdefault("DRLA_ALLOW_EAGER_REDUCE", "1")
    from distributed_reinforcement_learning_amd.parallel import dist as pdist

    local_rank = pdist.init_distributed()
    world = pdist.world_size()
    rank = pdist.rank()
    have_gpu = torch.cuda.is_available()
    device = f"cuda:{local_rank}" if have_gpu else "cpu"

    bench = {"impala": bench_impala, "apex": bench_apex,
             "r2d2": bench_r2d2}[args.algo]
    bench(args, rank, world, local_rank, have_gpu, device)


if __name__ == "__main__":
    main()
