"""drla_r2d2_nstep_loss_fwd (n-step returns under the value rescaling,
eta max/mean priorities; ops/hip/r2d2_loss.hip) against the naive float64
loop of tests/_r2d2_nstep_ref.py, under the float32 bound derived in that
module's docstring (a few thousand u = 2^-24 on td, dominated by the
cancellation in h^-1; tests/test_r2d2_nstep.py shows a float32
transcription of the kernel meets it). Then the layers above it: op
routing, the agent's fused path against its eager one, graph capture.
GPU-only."""

import numpy as np
import pytest
import torch

import _r2d2_nstep_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = ref.U
G = 2.5                                   # upstream gradient
GAMMA = 0.997
ETA = 0.9


def _f32(x):
    """The number the kernel sees for a double passed by value."""
    return float(np.float32(x))


def _run(mq, tq, act, r, done, w, gamma, n, eta, clip="abs_one",
         bf16=False, g=G):
    """fused_r2d2_loss fwd + bwd from numpy inputs. Returns loss, prio and
    grad as float64 numpy, the grad dtype, and the naive reference fed
    exactly the values the kernel saw."""
    from distributed_reinforcement_learning_amd.ops.r2d2_op import (
        fused_r2d2_loss,
    )
    f32 = dict(dtype=torch.float32, device=DEV)
    q = torch.as_tensor(mq, **f32)
    t = torch.as_tensor(tq, **f32)
    if bf16:
        q, t = q.bfloat16(), t.bfloat16()
    q.requires_grad_(True)
    a = torch.as_tensor(act, dtype=torch.int64, device=DEV)
    rt = torch.as_tensor(r, **f32)
    dt = torch.as_tensor(done, dtype=torch.bool, device=DEV)
    wt = torch.as_tensor(w, **f32)
    loss, prio = fused_r2d2_loss(q, t, a, rt, dt, wt, gamma, clip,
                                 n_step=n, priority_eta=eta)
    (g * loss).backward()
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and prio.dtype == torch.float32
    want = ref.naive(
        q.detach().double().cpu().numpy(), t.double().cpu().numpy(),
        act, rt.double().cpu().numpy(), done, wt.double().cpu().numpy(),
        _f32(gamma), n, eta=None if eta is None else _f32(eta), g=g,
        clip=clip)
    return (float(loss.detach().double()),
            prio.double().cpu().numpy(), q.grad.double().cpu().numpy(),
            q.grad.dtype, want)


def _check(loss, prio, grad, want, w, eta, bf16=False, g=G):
    B, T1 = want["td"].shape
    eta = None if eta is None else _f32(eta)
    lb = ref.loss_bound(want, w)
    pb = ref.prio_bound(want, eta)
    print(f"loss err {abs(loss - want['loss']):.3e} bound {lb:.3e}; "
          f"prio err {np.abs(prio - want['prio']).max():.3e} "
          f"bound {pb.max():.3e}")
    assert abs(loss - want["loss"]) <= lb
    assert (np.abs(prio - want["prio"]) <= pb).all()
    bi, ti = np.meshgrid(np.arange(B), np.arange(T1), indexing="ij")
    col = want["col"][:, :T1]
    on = grad[bi, ti, col]
    gb = ref.grad_bound(want, w, g, bf16=bf16)
    gerr = np.abs(on - want["dq"][bi, ti, col])
    print(f"grad err / bound, max {(gerr / gb).max():.3f}")
    assert (gerr <= gb).all()
    off = grad.copy()
    off[bi, ti, col] = 0.0
    assert (off == 0.0).all()            # other columns, and all of row W-1
    assert (grad[:, T1] == 0.0).all()


def _window(rng, B, W, A):
    f = np.float32
    mq = (rng.standard_normal((B, W, A)) * 2).astype(f)
    tq = (rng.standard_normal((B, W, A)) * 2).astype(f)
    act = rng.integers(0, A, (B, W))
    act[0, 0], act[1, 0] = -1, A + 7     # clamped to the ends
    r = (rng.standard_normal((B, W)) * 2).astype(f)
    done = rng.random((B, W)) < 0.15
    w = (rng.random(B) + 0.5).astype(f)
    return mq, tq, act, r, done, w


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("A", [2, 6])
@pytest.mark.parametrize("W", [2, 3, 9, 17, 40])
def test_sweep_against_float64(W, A, bf16):
    """W = 2: one trained row. W = 9, 17: W-1 is a power of two, so the
    block has no thread for row W-1. W = 40: a block that is not full.
    eta is set so that n = 1 runs the n-step kernel too."""
    B = 5
    rng = np.random.default_rng(100 * W + A)
    args = _window(rng, B, W, A)
    for n in (1, 2, 5, W + 3):
        loss, prio, grad, gdtype, want = _run(*args, GAMMA, n, ETA,
                                              bf16=bf16)
        assert gdtype == (torch.bfloat16 if bf16 else torch.float32)
        assert want["col"][0, 0] == 0 and want["col"][1, 0] == A - 1
        _check(loss, prio, grad, want, args[5], ETA, bf16=bf16)


def _ext_td(mq, tq, act, r, done, gamma, n, clip="none"):
    """The td stash straight from the extension's keyword interface."""
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    f32 = dict(dtype=torch.float32, device=DEV)
    B = mq.shape[0]
    _, td_st, _ = ext.r2d2_loss_fwd(
        torch.as_tensor(mq, **f32), torch.as_tensor(tq, **f32),
        torch.as_tensor(act, dtype=torch.int32, device=DEV),
        torch.as_tensor(r, **f32),
        torch.as_tensor(done, dtype=torch.bool, device=DEV),
        torch.ones(B, **f32), gamma, {"abs_one": 0, "none": 2}[clip],
        n_step=n, priority_eta=0.5)
    torch.cuda.synchronize()
    return td_st.double().cpu().numpy()


def _structure_inputs(W, A=3):
    """One sequence. Target Q is constant along a row and 10 apart across
    rows (h^-1 of it: more than 10 apart), rewards are distinct eighths,
    main Q is 0 except a last column of ones (argmax = A-1; the state
    action 0 has value 0), so td = h(z) and z names the rows used."""
    mq = np.zeros((1, W, A), dtype=np.float32)
    mq[0, :, A - 1] = 1.0
    tq = np.zeros((1, W, A), dtype=np.float32)
    tq[0] = (10.0 * (np.arange(W) + 1))[:, None]
    act = np.zeros((1, W), dtype=np.int64)
    r = ((np.arange(W) + 1) / 8.0).astype(np.float32)[None]
    done = np.zeros((1, W), dtype=bool)
    return mq, tq, act, r, done


def test_structure_done_cuts_rewards_and_bootstrap():
    W, n = 9, 3
    mq, tq, act, r, done = _structure_inputs(W)
    done[0, 4] = True
    td = _ext_td(mq, tq, act, r, done, 0.5, n)[0]
    want = ref.naive(mq, tq, act, r, done, np.ones(1), 0.5, n,
                     clip="none")
    assert (np.abs(td - want["td"][0]) <= want["e"][0]).all()
    rr = r[0].astype(np.float64)
    boot = ref.hinv64(tq[0, :, 0].astype(np.float64))
    # t = 1: untouched by the done at row 4: rows 1..3, bootstrap row 4
    z1 = rr[1] + rr[2] / 2 + rr[3] / 4 + boot[4] / 8
    # t = 2: done at j = 2: rewards of rows 2..4, no bootstrap
    z2 = rr[2] + rr[3] / 2 + rr[4] / 4
    # t = 3: done at j = 1: rows 3 and 4 only; t = 4: its own reward only
    z3 = rr[3] + rr[4] / 2
    z4 = rr[4]
    # t = 5: past the done: rows 5..7 and the bootstrap of row 8
    z5 = rr[5] + rr[6] / 2 + rr[7] / 4 + boot[8] / 8
    for t, z in ((1, z1), (2, z2), (3, z3), (4, z4), (5, z5)):
        assert abs(td[t] - ref.h64(z)) <= want["e"][0, t], t
        assert want["e"][0, t] < 1e-3
    # what a kernel that ignored the done would give is far outside
    assert abs(ref.h64(z2 + boot[5] / 8) - ref.h64(z2)) > 0.5


def test_structure_truncation_uses_the_last_row():
    W, n = 9, 5
    mq, tq, act, r, done = _structure_inputs(W)
    td = _ext_td(mq, tq, act, r, done, 0.5, n)[0]
    want = ref.naive(mq, tq, act, r, done, np.ones(1), 0.5, n,
                     clip="none")
    assert (np.abs(td - want["td"][0]) <= want["e"][0]).all()
    rr = r[0].astype(np.float64)
    boot = ref.hinv64(tq[0, :, 0].astype(np.float64))
    T1 = W - 1
    for t in range(T1):
        k = min(n, T1 - t)
        z = sum(rr[t + j] / 2 ** j for j in range(k)) + boot[t + k] / 2 ** k
        assert abs(td[t] - ref.h64(z)) <= want["e"][0, t], t
    # t = 5, 6, 7 are cut to k = 3, 2, 1 and bootstrap from row W-1 = 8;
    # the neighbouring row would miss by far more than the bound
    assert want["e"].max() < 1e-3
    assert abs(ref.h64(rr[7] + boot[8] / 2) - ref.h64(rr[7] + boot[7] / 2)) \
        > 0.1


@pytest.mark.parametrize("W", [2, 9, 12])
def test_structure_large_n_is_the_full_truncation(W):
    mq, tq, act, r, done = _structure_inputs(W)
    done[0, W // 2] = W > 2
    full = _ext_td(mq, tq, act, r, done, 0.5, W - 1)
    for n in (W, W + 3, 10 ** 6, 2 ** 40):
        np.testing.assert_array_equal(
            _ext_td(mq, tq, act, r, done, 0.5, n), full)
    want = ref.naive(mq, tq, act, r, done, np.ones(1), 0.5, W - 1,
                     clip="none")
    assert (np.abs(full - want["td"]) <= want["e"]).all()


def test_argmax_ties_take_the_first_column():
    """The tie rows of tests/test_gpu_dqn_loss.py at the bootstrap row;
    target values name the column: td = h(h^-1(x)) = x up to the bound."""
    nm = np.array([
        [1.0, 3.0, 3.0, 0.0, -1.0],     # max at 1, 2
        [2.0, 0.0, 2.0, 1.0, 2.0],      # max at 0, 2, 4
        [0.5, 0.5, 0.5, 0.5, 0.5],      # all equal
        [-4.0, -2.0, -3.0, -2.0, -2.0],  # negative max at 1, 3, 4
        [0.0, -0.0, 0.0, -1.0, -2.0],   # +0 == -0 ties
        [0.0, 1.0, 2.0, 3.0, 3.0],      # max at the last two
    ], dtype=np.float32)
    B, A = nm.shape
    for W, n in ((2, 1), (4, 3)):
        mq = np.zeros((B, W, A), dtype=np.float32)
        mq[:, 1:] = 9.0 * np.eye(A, dtype=np.float32)[A - 1]  # decoys
        mq[:, W - 1] = nm
        tq = np.full((B, W, A), 32.0, dtype=np.float32)
        tq[:, W - 1] = np.array([1.0, 2.0, 4.0, 8.0, 16.0],
                                dtype=np.float32)
        act = np.zeros((B, W), dtype=np.int64)
        r = np.zeros((B, W), dtype=np.float32)
        done = np.zeros((B, W), dtype=bool)
        td = _ext_td(mq, tq, act, r, done, 1.0, n)
        want = ref.naive(mq, tq, act, r, done, np.ones(B), 1.0, n,
                         clip="none")
        assert (np.abs(td - want["td"]) <= want["e"]).all()
        assert want["e"].max() < 1e-3
        # position 0 bootstraps from row W-1 under both (W, n)
        assert np.round(td[:, 0]).tolist() == [2.0, 1.0, 1.0, 2.0, 1.0, 8.0]
        assert np.abs(td[:, 0] - np.round(td[:, 0])).max() < 1e-3


@pytest.mark.parametrize("eta", [0.0, 0.9, 1.0, None])
def test_priority_modes(eta):
    B, W, A = 5, 12, 4
    rng = np.random.default_rng(77)
    args = _window(rng, B, W, A)
    for n in (1, 3):
        if n == 1 and eta is None:
            continue                     # that is the 1-step kernel
        loss, prio, grad, _, want = _run(*args, GAMMA, n, eta)
        _check(loss, prio, grad, want, args[5], eta)
        a = np.abs(want["td"])
        if eta == 0.0:
            np.testing.assert_array_equal(want["prio"], a.mean(axis=1))
        if eta == 1.0:
            np.testing.assert_array_equal(want["prio"], a.max(axis=1))
            # a max of float32 values is one of them: no rounding at all
            assert (np.abs(prio - a.max(axis=1))
                    <= want["e"].max(axis=1)).all()
    # the modes differ by far more than the bound on this batch
    assert (a.max(axis=1) - a.mean(axis=1) > 0.1).all()
    assert (a.mean(axis=1) - np.abs(want["td"].mean(axis=1)) > 0.01).all()


def test_default_arguments_route_to_the_one_step_kernel():
    """n_step=1, priority_eta=None spelled out is the same kernel as the
    arguments omitted: priorities and gradients bit-equal. The loss is a
    float32 atomic sum over B blocks in any order: each run is within
    (B - 1) u of the exact sum of the same B non-negative terms."""
    from distributed_reinforcement_learning_amd.ops.r2d2_op import (
        fused_r2d2_loss,
    )
    B, W, A = 6, 15, 4
    torch.manual_seed(5)
    mq = (torch.randn(B, W, A, device=DEV) * 2).bfloat16()
    tq = (torch.randn(B, W, A, device=DEV) * 2).bfloat16()
    a = torch.randint(0, A, (B, W), device=DEV)
    r = torch.randn(B, W, device=DEV) * 2
    d = torch.rand(B, W, device=DEV) < 0.1
    w = torch.rand(B, device=DEV) + 0.5
    out = []
    for kw in (dict(), dict(n_step=1, priority_eta=None)):
        q = mq.clone().requires_grad_(True)
        loss, prio = fused_r2d2_loss(q, tq, a, r, d, w, GAMMA, "abs_one",
                                     **kw)
        (G * loss).backward()
        out.append((float(loss.detach().double()), prio, q.grad))
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2])
    assert abs(out[0][0] - out[1][0]) <= 2 * (B - 1) * U * max(out[0][0],
                                                               out[1][0])
    # and the n-step kernel at n = 1 agrees with it within the bound
    q = mq.clone().requires_grad_(True)
    _, prio_n = fused_r2d2_loss(q, tq, a, r, d, w, GAMMA, "abs_one",
                                n_step=1, priority_eta=1.0)
    want = ref.naive(mq.double().cpu().numpy(), tq.double().cpu().numpy(),
                     a.cpu().numpy(), r.double().cpu().numpy(),
                     d.cpu().numpy(), w.double().cpu().numpy(),
                     _f32(GAMMA), 1, eta=None)
    legacy = out[0][1].double().cpu().numpy()
    assert (np.abs(legacy - want["prio"])
            <= ref.prio_bound(want, None)).all()
    assert (prio_n.double().cpu().numpy()
            <= np.abs(want["td"]).max(axis=1) + want["e"].max(axis=1)).all()


def test_bad_arguments_are_errors():
    from distributed_reinforcement_learning_amd import ops
    from distributed_reinforcement_learning_amd.ops.r2d2_op import (
        fused_r2d2_loss,
    )
    ext = ops.require_ext()
    B, W, A = 2, 4, 3
    f32 = dict(dtype=torch.float32, device=DEV)
    q = torch.zeros(B, W, A, **f32)
    a = torch.zeros(B, W, dtype=torch.int32, device=DEV)
    z = torch.zeros(B, W, **f32)
    d = torch.zeros(B, W, dtype=torch.bool, device=DEV)
    w = torch.ones(B, **f32)
    with pytest.raises(RuntimeError, match="n_step"):
        ext.r2d2_loss_fwd(q, q, a, z, d, w, 0.99, 0, n_step=0)
    with pytest.raises(RuntimeError, match="priority_eta"):
        ext.r2d2_loss_fwd(q, q, a, z, d, w, 0.99, 0, priority_eta=1.5)
    for kw in (dict(n_step=0), dict(priority_eta=1.5),
               dict(priority_eta=-0.5)):
        with pytest.raises(ValueError):
            fused_r2d2_loss(q, q, a, z, d, w, 0.99, "abs_one", **kw)


def test_soft_asymmetric_clip_at_n3():
    """The tolerance of test_fused_r2d2_loss_soft_asymmetric_clip, 1e-4 on
    fp32 inputs: device tanhf has no bound in the project."""
    B, W, A = 4, 10, 6
    rng = np.random.default_rng(6)
    f = np.float32
    mq = rng.standard_normal((B, W, A)).astype(f)
    tq = rng.standard_normal((B, W, A)).astype(f)
    act = rng.integers(0, A, (B, W))
    r = (rng.standard_normal((B, W)) * 4).astype(f)
    done = np.zeros((B, W), dtype=bool)
    w = np.ones(B, dtype=f)
    loss, prio, _, _, want = _run(mq, tq, act, r, done, w, 0.99, 3, None,
                                  clip="soft_asymmetric")
    assert loss == pytest.approx(want["loss"], rel=1e-4)
    np.testing.assert_allclose(prio, want["prio"], atol=1e-4, rtol=1e-4)


# -- agent level --------------------------------------------------------------

def _agent(L, BI, A, H, **kw):
    from distributed_reinforcement_learning_amd.agents import r2d2
    return r2d2.Agent(seq_len=L, burn_in=BI, input_shape=[84, 84, 1],
                      num_action=A, lstm_size=H, discount_factor=0.997,
                      start_learning_rate=1e-4, end_learning_rate=0.0,
                      learning_frame=10 ** 9, gradient_clip_norm=40.0,
                      device=DEV, seed=0, n_step=5, priority_eta=0.9, **kw)


def _sequences(rng, B, L, A, H):
    return dict(
        state=torch.as_tensor(rng.integers(
            0, 255, (B, L, 84, 84, 1), dtype=np.uint8)).to(DEV),
        previous_action=torch.as_tensor(
            rng.integers(0, A, (B, L)).astype(np.int32)).to(DEV),
        action=torch.as_tensor(
            rng.integers(0, A, (B, L)).astype(np.int32)).to(DEV),
        reward=torch.as_tensor(
            rng.normal(size=(B, L)).astype(np.float32)).to(DEV),
        done=torch.as_tensor(rng.random((B, L)) < 0.1).to(DEV),
        initial_h=torch.zeros(B, L, H, device=DEV),
        initial_c=torch.zeros(B, L, H, device=DEV))


def test_agent_fused_nstep_matches_its_eager_path():
    """The shape and the 0.05 tolerances of
    test_agent_fused_path_matches_eager_composition (bf16 networks)."""
    from distributed_reinforcement_learning_amd.algorithms import nstep
    B, L, BI, A, H = 3, 12, 5, 4, 64
    agent = _agent(L, BI, A, H, build_optimizer=False)
    b = _sequences(np.random.default_rng(9), B, L, A, H)
    w = torch.ones(B, device=DEV)
    args = (b["state"], b["previous_action"].long(), b["action"].long(),
            b["initial_h"][:, 0], b["initial_c"][:, 0], b["reward"],
            b["done"])
    assert agent._use_fused_tail()
    loss_f, td_f = agent.compute_sequence_loss(*args, w)
    unweighted, tgt, sav = agent._sequence_losses(*args, with_grad=False)
    loss_e = (unweighted * w).mean()
    td_e = nstep.sequence_priority(tgt - sav, 0.9)
    assert float(loss_f.detach()) == pytest.approx(float(loss_e), rel=0.05)
    assert torch.allclose(td_f, td_e, atol=0.05, rtol=0.05)
    # scoring and training share the tail
    td_s = agent.get_td_error_batch(*args, as_tensor=True)
    assert torch.allclose(td_s, td_e, atol=0.05, rtol=0.05)


def test_graphed_replay_step_with_the_nstep_agent():
    from distributed_reinforcement_learning_amd.replay.gpu_memory import (
        GpuMemory,
    )
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedReplayStep,
    )
    N, L, BI, A, H = 12, 12, 5, 4, 64
    agent = _agent(L, BI, A, H, build_optimizer=True)
    mem = GpuMemory(64, fields={
        "state": ((L, 84, 84, 1), torch.uint8),
        "previous_action": ((L,), torch.int32),
        "action": ((L,), torch.int32),
        "reward": ((L,), torch.float32),
        "done": ((L,), torch.bool),
        "initial_h": ((L, H), torch.float32),
        "initial_c": ((L, H), torch.float32)}, device=DEV, seed=5)
    u = _sequences(np.random.default_rng(2), N, L, A, H)
    td = agent.get_td_error_batch(
        u["state"], u["previous_action"], u["action"],
        u["initial_h"][:, 0], u["initial_c"][:, 0], u["reward"], u["done"],
        as_tensor=True)
    assert (td >= 0).all()
    mem.add_batch(td, u)

    def loss_fn(b, w):
        return agent.compute_sequence_loss(
            b["state"], b["previous_action"], b["action"],
            b["initial_h"][:, 0], b["initial_c"][:, 0], b["reward"],
            b["done"], w)

    g = GraphedReplayStep(agent, mem, 4, loss_fn)
    params = [agent.optimizer.flat_params.detach().clone()]
    for _ in range(2):
        loss = float(g.step())
        assert np.isfinite(loss)
        assert (g.td >= 0).all() and torch.isfinite(g.td).all()
        params.append(agent.optimizer.flat_params.detach().clone())
    assert not torch.equal(params[0], params[1])
    assert not torch.equal(params[1], params[2])
    leaves = mem.tree[mem.capacity - 1:]
    assert (leaves >= 0).all() and torch.isfinite(leaves).all()
