"""Assertions shared by the tests that build a graph-captured learner step
(GraphedImpalaStep, GraphedTrainStep, GraphedReplayStep): constructing one
warms up eagerly and captures, and must leave every piece of training state
exactly where it found it; stepping it must advance the counters and write
the optimizer's own lr_t into lr_buf."""

import torch


def snapshot(agent, memory=None) -> dict:
    """Clones of everything the construction of a captured step may touch.
    Take it right before building the step."""
    opt = agent.optimizer
    snap = {
        "flat_params": opt.flat_params.detach().clone(),
        "master": opt.master.detach().clone(),
        "state": {k: v.detach().clone()
                  for k, v in opt._state_tensors().items()},
        "step_count": opt.step_count,
        "global_step": agent.global_step,
    }
    if memory is not None:
        snap["tree"] = memory.tree.detach().clone()
        snap["beta"] = memory.beta
        snap["beta_buf"] = float(memory.beta_buf)
    return snap


def assert_construction_preserved(agent, lr_buf, snap, memory=None) -> None:
    """Right after the step class is built: bit-equal weights, fp32 master
    and optimizer state, zero grads, untouched counters, scatter mode on,
    lr_buf still zero (and, for a replay, the whole tree and beta)."""
    torch.cuda.synchronize()
    opt = agent.optimizer
    assert torch.equal(opt.flat_params, snap["flat_params"])
    assert torch.equal(opt.master, snap["master"])
    state = opt._state_tensors()
    assert set(state) == set(snap["state"])
    for k, v in state.items():
        assert torch.equal(v, snap["state"][k]), k
    assert not opt.flat_grads.any()
    assert opt.step_count == snap["step_count"]
    assert agent.global_step == snap["global_step"]
    assert opt.scatter is True
    assert float(lr_buf) == 0.0
    if memory is not None:
        assert torch.equal(memory.tree, snap["tree"])
        assert memory.beta == snap["beta"]
        assert float(memory.beta_buf) == snap["beta_buf"]


def assert_after_steps(agent, lr_buf, k: int) -> float:
    """After k steps from a fresh agent: both counters read k and lr_buf
    holds what the k-th step wrote, opt.lr_t_for(lr_at(k-1), k) rounded to
    the buffer's float32 (raw lr for RMSProp, bias-corrected for Adam).
    Returns the un-corrected lr of that step."""
    torch.cuda.synchronize()
    opt = agent.optimizer
    assert opt.step_count == k
    assert agent.global_step == k
    lr = agent.lr_at(k - 1)
    want = torch.tensor(opt.lr_t_for(lr, k), dtype=torch.float32)
    assert float(lr_buf) == float(want)
    return lr
