"""Fused V-trace loss without a zero-fill in front of its loss sums: the
blocks write per-block partials, take a ticket, and the last block sums them
in block order (ops/hip/vtrace_loss.hip). Repeated calls must give bit-equal
losses (fixed-order sum, counter restored by every launch) and the values
must still match the CPU composition. GPU-only."""

import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA, C_B, C_E = 0.99, 0.7, 0.03


def _inputs(B, T, A, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, A, generator=g) * 2
    value = torch.randn(B, T, generator=g)
    mu = torch.softmax(torch.randn(B, T, A, generator=g), -1)
    actions = torch.randint(0, A, (B, T), generator=g, dtype=torch.int32)
    rewards = torch.randn(B, T, generator=g) * 2.0
    done = torch.rand(B, T, generator=g) < 0.1
    return logits, value, mu, actions, rewards, done


def _cpu_reference(logits, value, mu, actions, rewards, done):
    """algorithms/vtrace.py composed on CPU in fp32 (what agents/impala.py
    runs on a CPU agent)."""
    from distributed_reinforcement_learning_amd.algorithms import vtrace
    rewards = rewards.clamp(-1, 1)  # abs_one
    discounts = (~done).float() * GAMMA
    policy = torch.softmax(logits.float(), dim=-1)
    actions = actions.long()
    p_f, p_m, _ = vtrace.split_data(policy)
    v_f, v_m, v_l = vtrace.split_data(value)
    a_f, a_m, _ = vtrace.split_data(actions)
    r_f, r_m, _ = vtrace.split_data(rewards)
    g_f, g_m, _ = vtrace.split_data(discounts)
    mu_f, mu_m, _ = vtrace.split_data(mu)
    vs, rho = vtrace.from_softmax(mu_f, p_f, a_f, g_f, r_f, v_f, v_m)
    vs1, _ = vtrace.from_softmax(mu_m, p_m, a_m, g_m, r_m, v_m, v_l)
    adv = (rho * (r_f + g_f * vs1 - v_f)).detach()
    pi = vtrace.compute_policy_gradient_loss(p_f, a_f, adv)
    bl = vtrace.compute_baseline_loss(vs, v_f)
    ent = vtrace.compute_entropy_loss(p_f)
    return float(pi), float(bl), float(ent), float(pi + C_B * bl + C_E * ent)


def _check_against_reference(got, ref):
    # the tolerances of tests/test_gpu_vtrace_loss.py (fp32 logits)
    pi, bl, ent, total = (float(x) for x in got)
    assert pi == pytest.approx(ref[0], rel=2e-4, abs=1e-2)
    assert bl == pytest.approx(ref[1], rel=2e-4, abs=1e-2)
    assert ent == pytest.approx(ref[2], rel=2e-4, abs=1e-2)
    assert total == pytest.approx(ref[3], rel=5e-3, abs=2e-2)


def _call(dev_inputs):
    from distributed_reinforcement_learning_amd.ops import fused_vtrace_loss
    logits, value, mu, actions, rewards, done = dev_inputs
    with torch.no_grad():
        out = fused_vtrace_loss(logits, value, mu, actions, rewards, done,
                                GAMMA, "abs_one", C_B, C_E)
    return torch.stack(out)


# B = 1: the only block is also the last one; 3: a few tickets; 33: more
# blocks than a wave has lanes. T = 3 is the smallest legal trajectory
# (a one-step first window), T = 20 the flagship's.
@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_repeated_calls_bit_equal_then_reference(B, T):
    A = 6
    x = _inputs(B, T, A, seed=B * 100 + T)
    y = _inputs(B, T, A, seed=B * 100 + T + 1)
    xd = tuple(t.cuda() for t in x)
    yd = tuple(t.cuda() for t in y)
    first = _call(xd)
    for _ in range(2):
        assert torch.equal(_call(xd), first)
    _check_against_reference(first, _cpu_reference(*x))
    # different inputs next: nothing of the earlier calls may leak in
    _check_against_reference(_call(yd), _cpu_reference(*y))


@pytest.mark.parametrize("T", [3, 20])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_captured_call_replays_bit_equal(B, T):
    A = 6
    x = _inputs(B, T, A, seed=B * 100 + T + 2)
    y = _inputs(B, T, A, seed=B * 100 + T + 3)
    static = tuple(t.cuda() for t in x)
    _call(static)  # eager warm-up: persistent buffers exist before capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _call(static)
    results = []
    for _ in range(3):
        g.replay()
        results.append(out.clone())
    assert torch.equal(results[0], results[1])
    assert torch.equal(results[0], results[2])
    _check_against_reference(results[0], _cpu_reference(*x))
    for dst, src in zip(static, y):
        dst.copy_(src)
    g.replay()
    _check_against_reference(out, _cpu_reference(*y))


def test_nofill_matches_the_atomic_path():
    """ext-level: the ticketed sums against the default zero-filled
    atomicAdd path of the same kernel, same inputs."""
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    B, T, A = 33, 20, 6
    logits, value, mu, actions, rewards, done = (
        t.cuda() for t in _inputs(B, T, A, seed=7))
    args = (logits, value, mu, actions, rewards, done, GAMMA, 0, C_B, C_E)
    atomic = ext.vtrace_loss_fwd(*args)
    ticket = ext.vtrace_loss_fwd(*args, nofill=True)
    # only the summation order of the 33 f32 block partials differs: the
    # worst case is 2*(B-1)*eps*sum|partial| with |partial| <= ~T*A*few
    # ~ 1e2, i.e. 2*32*6e-8*33*1e2 ~ 1.3e-2
    assert torch.allclose(ticket[0], atomic[0], rtol=0, atol=1.3e-2)
    for a, b in zip(atomic[1:], ticket[1:]):
        assert torch.equal(a, b)
