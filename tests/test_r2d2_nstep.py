"""n-step returns and max/mean priorities for R2D2, on the CPU: the
reference math of algorithms/nstep.py against a naive loop, the agent's
eager path, the config keys, and a float32 transcription of the fused
kernel held to the bound the GPU test uses (derived in
tests/_r2d2_nstep_ref.py, in units of u = 2^-24)."""

import numpy as np
import pytest
import torch

import _r2d2_nstep_ref as ref
from distributed_reinforcement_learning_amd.agents import r2d2 as r2d2_agent
from distributed_reinforcement_learning_amd.agents.base import clip_rewards
from distributed_reinforcement_learning_amd.algorithms import burn_in as rs
from distributed_reinforcement_learning_amd.algorithms import dqn, nstep
from distributed_reinforcement_learning_amd.config import check_properties

GAMMA = float(np.float32(0.997))


def _window(rng, B, W, A, done_rate=0.15, bf16=False):
    """float32-valued window inputs (Q ~ N(0, 2^2))."""
    f = np.float32
    mq = (rng.standard_normal((B, W, A)) * 2).astype(f)
    tq = (rng.standard_normal((B, W, A)) * 2).astype(f)
    if bf16:
        mq = torch.as_tensor(mq).bfloat16().float().numpy()
        tq = torch.as_tensor(tq).bfloat16().float().numpy()
    act = rng.integers(0, A, (B, W))
    r = (rng.standard_normal((B, W)) * 2).astype(f)
    done = rng.random((B, W)) < done_rate
    w = (rng.random(B) + 0.5).astype(f)
    return mq, tq, act, r, done, w


def _torch_td(mq, tq, act, r, done, gamma, n, clip="abs_one"):
    """The composition agents/r2d2.py::_sequence_losses makes of the
    reference functions, in float64."""
    mq, tq = torch.as_tensor(mq).double(), torch.as_tensor(tq).double()
    cr = clip_rewards(torch.as_tensor(r).double(), clip)
    disc = (~torch.as_tensor(done)).double() * gamma
    a = torch.as_tensor(act).long()
    boot = rs.inverse_value_function_rescaling(
        dqn.take_state_action_value(tq, mq.argmax(dim=2)))
    z = nstep.nstep_window_target(boot, cr, disc, n)
    assert z.dtype == torch.float64 and z.shape == (mq.shape[0],
                                                    mq.shape[1] - 1)
    sav = dqn.take_state_action_value(mq[:, :-1], a[:, :-1])
    return rs.value_function_rescaling(z) - sav


@pytest.mark.parametrize("W", [2, 3, 9, 40])
def test_reference_matches_naive_loop(W):
    rng = np.random.default_rng(W)
    B, A = 4, 3
    mq, tq, act, r, done, w = _window(rng, B, W, A, done_rate=0.2)
    assert done[:, :-1].any() or W == 2
    for n in (1, 2, 5, W + 3):
        want = ref.naive(mq, tq, act, r, done, w, GAMMA, n, eta=0.9)
        td = _torch_td(mq, tq, act, r, done, GAMMA, n)
        np.testing.assert_allclose(td.numpy(), want["td"], rtol=0,
                                   atol=1e-12)
        for eta in (None, 0.0, 0.9, 1.0):
            want = ref.naive(mq, tq, act, r, done, w, GAMMA, n, eta=eta)
            got = nstep.sequence_priority(torch.as_tensor(want["td"]), eta)
            np.testing.assert_allclose(got.numpy(), want["prio"], rtol=0,
                                       atol=1e-13)


def test_done_cuts_later_rewards_and_the_bootstrap():
    """Hand-computed: gamma 0.5, rewards 1, 2, 4, ..., bootstrap 100 u."""
    W = 5
    boot = torch.arange(W, dtype=torch.float64)[None] * 100.0
    r = torch.tensor([[1.0, 2.0, 4.0, 8.0, 16.0]], dtype=torch.float64)
    disc = torch.full((1, W), 0.5, dtype=torch.float64)
    z = nstep.nstep_window_target(boot, r, disc, 3)
    # t=0: 1 + 2/2 + 4/4 + 300/8; t=1: 2 + 2 + 2 + 400/8;
    # t=2: k=2: 4 + 4 + 400/4; t=3: k=1: 8 + 400/2
    assert z.tolist() == [[40.5, 56.0, 108.0, 208.0]]
    disc[0, 1] = 0.0                                # done at row 1
    z = nstep.nstep_window_target(boot, r, disc, 3)
    assert z.tolist() == [[2.0, 2.0, 108.0, 208.0]]
    # every n >= W-1 is the full truncation
    full = nstep.nstep_window_target(boot, r, disc, W - 1)
    assert torch.equal(nstep.nstep_window_target(boot, r, disc, W + 3),
                       full)
    with pytest.raises(ValueError):
        nstep.nstep_window_target(boot, r, disc, 0)


def test_n1_equals_the_one_step_composition():
    """Bit for bit, in float32 and float64: r + disc z is the same two
    operations as the 1-step tail's z disc + r."""
    rng = np.random.default_rng(3)
    B, W, A = 6, 12, 4
    mq, tq, act, r, done, w = _window(rng, B, W, A)
    for dt in (torch.float32, torch.float64):
        mqt, tqt = torch.as_tensor(mq).to(dt), torch.as_tensor(tq).to(dt)
        cr = clip_rewards(torch.as_tensor(r).to(dt), "abs_one")
        disc = (~torch.as_tensor(done)).to(dt) * GAMMA
        # the 1-step composition of tests/test_gpu_r2d2_loss.py
        nsav = dqn.take_state_action_value(tqt[:, 1:],
                                           mqt[:, 1:].argmax(dim=2))
        old = rs.inverse_value_function_rescaling(nsav) * disc[:, :-1] \
            + cr[:, :-1]
        boot = rs.inverse_value_function_rescaling(
            dqn.take_state_action_value(tqt, mqt.argmax(dim=2)))
        new = nstep.nstep_window_target(boot, cr, disc, 1)
        assert new.dtype == dt
        assert torch.equal(new, old)


def test_priority_edge_cases():
    td = torch.tensor([[3.0, -3.0, 1.0, -1.0], [0.5, 0.5, -2.0, 0.0]],
                      dtype=torch.float64)
    assert nstep.sequence_priority(td, 0.0).tolist() == [2.0, 0.75]
    assert nstep.sequence_priority(td, 1.0).tolist() == [3.0, 2.0]
    assert nstep.sequence_priority(td, None).tolist() == [0.0, 0.25]
    assert nstep.sequence_priority(td).tolist() == [0.0, 0.25]
    mix = nstep.sequence_priority(td, 0.9)
    np.testing.assert_allclose(mix.numpy(), [0.9 * 3 + 0.1 * 2,
                                             0.9 * 2 + 0.1 * 0.75],
                               rtol=1e-15)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            nstep.sequence_priority(td, bad)


# -- agent on CPU -------------------------------------------------------------

def _agent(**kw):
    return r2d2_agent.Agent(
        seq_len=6, burn_in=2, input_shape=[84, 84, 1], num_action=4,
        lstm_size=8, discount_factor=0.997, start_learning_rate=1e-4,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        gradient_clip_norm=40.0, seed=0, **kw)


def _batch(B=2, L=6, lstm=8, seed=0):
    """The _r2d2_batch shape of tests/test_agents.py."""
    rng = np.random.default_rng(seed)
    return dict(
        state=rng.integers(0, 255, (B, L, 84, 84, 1), dtype=np.uint8),
        previous_action=rng.integers(0, 4, (B, L)).astype(np.int32),
        action=rng.integers(0, 4, (B, L)).astype(np.int32),
        h=rng.normal(size=(B, L, lstm)).astype(np.float32) * 0.1,
        c=rng.normal(size=(B, L, lstm)).astype(np.float32) * 0.1,
        reward=rng.normal(size=(B, L)).astype(np.float32),
        done=np.zeros((B, L), dtype=bool),
    )


@pytest.mark.parametrize("burn_grad", [False, True])
def test_agent_trains_one_nstep_step(burn_grad):
    agent = _agent(n_step=5, priority_eta=0.9, burn_in_gradient=burn_grad)
    loss, td = agent.train(**_batch(), weight=np.ones(2, np.float32))
    assert np.isfinite(loss)
    assert td.shape == (2,) and (td >= 0).all()


def test_agent_nstep_targets_differ_from_one_step():
    b = _batch()
    assert (b["reward"] != 0).all()
    args = (b["state"], b["previous_action"], b["action"], b["h"][:, 0],
            b["c"][:, 0], b["reward"], b["done"])
    one = _agent()                       # the defaults: 1-step, |mean td|
    assert one.n_step == 1 and one.priority_eta is None
    five = _agent(n_step=5, priority_eta=0.9)    # same seed, same weights
    _, tgt1, sav1 = one._sequence_losses(*args, with_grad=False)
    _, tgt5, sav5 = five._sequence_losses(*args, with_grad=False)
    assert torch.equal(sav1, sav5)
    # the last trained position is truncated to one step under any n
    assert torch.equal(tgt1[:, -1], tgt5[:, -1])
    assert (tgt1[:, :-1] != tgt5[:, :-1]).all()
    loss, prio = five.compute_sequence_loss(*args,
                                            torch.ones(2))
    want = nstep.sequence_priority(tgt5 - sav5, 0.9)
    assert torch.allclose(prio, want, rtol=1e-6, atol=0)
    assert float(loss.detach()) == pytest.approx(
        float(((tgt5 - sav5) ** 2).mean(dim=1).mean()), rel=1e-6)


def test_agent_td_error_is_row_zero_of_the_batch():
    agent = _agent(n_step=5, priority_eta=0.9)
    b = _batch(B=3, seed=4)
    batch = agent.get_td_error_batch(
        b["state"], b["previous_action"], b["action"], b["h"][:, 0],
        b["c"][:, 0], b["reward"], b["done"])
    assert batch.shape == (3,) and (batch >= 0).all()
    for i in (0, 2):
        one = agent.get_td_error(
            b["state"][i], b["previous_action"][i], b["action"][i],
            b["h"][i], b["c"][i], b["reward"][i], b["done"][i])
        assert one == pytest.approx(float(batch[i]), rel=1e-5)


def test_agent_rejects_bad_settings():
    for kw in (dict(n_step=0), dict(n_step=2.5), dict(priority_eta=1.5),
               dict(priority_eta=-0.1)):
        with pytest.raises(ValueError):
            _agent(build_optimizer=False, **kw)


# -- config -------------------------------------------------------------------

def _block(**extra):
    blk = dict(num_actors=2, env=["a", "b"], available_action=[4, 4],
               model_output=4, reward_clipping="abs_one")
    blk.update(extra)
    return blk


def test_config_validates_the_optional_keys():
    check_properties(_block())                      # neither key
    check_properties(_block(n_step=5, priority_eta=0.9))
    check_properties(_block(n_step=1, priority_eta=0))
    check_properties(_block(priority_eta=1.0))
    for bad in (dict(n_step=0), dict(n_step=-3), dict(n_step=2.5),
                dict(n_step="5"), dict(priority_eta=1.5),
                dict(priority_eta=-0.01), dict(priority_eta="0.9")):
        with pytest.raises(ValueError):
            check_properties(_block(**bad))


def test_trainer_passes_the_keys_to_the_agent(monkeypatch):
    from types import SimpleNamespace
    from distributed_reinforcement_learning_amd.config import load_config, \
        default_config_path
    from distributed_reinforcement_learning_amd.trainers import r2d2 as tr
    seen = {}
    monkeypatch.setattr(tr.r2d2_agent, "Agent",
                        lambda **kw: seen.update(kw) or "agent")
    cfg = load_config(default_config_path(), "r2d2")
    assert "n_step" not in cfg.raw and "priority_eta" not in cfg.raw
    assert tr.build_agent(SimpleNamespace(cfg=cfg), "cpu", False) == "agent"
    assert seen["n_step"] == 1 and seen["priority_eta"] is None
    cfg.raw.update(n_step=5, priority_eta=0.9)
    tr.build_agent(SimpleNamespace(cfg=cfg), "cpu", False)
    assert seen["n_step"] == 5 and seen["priority_eta"] == 0.9


# -- the kernel's formula in float32, against the GPU test's bound ------------

@pytest.mark.parametrize("contract", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W", [2, 3, 9, 17, 40])
def test_float32_transcription_meets_the_bound(W, bf16, contract):
    """The tolerance of tests/test_gpu_r2d2_nstep.py, shown feasible
    without a GPU: a float32 numpy transcription of the kernel (in source
    order, and with its multiply-adds contracted) stays inside the bound
    derived in tests/_r2d2_nstep_ref.py at the GPU sweep's shapes. The
    bound is not vacuous either: it stays below 2^-8 here, hundreds of
    times under the unit-sized errors a wrong row or column makes."""
    B, A = 5, 6
    rng = np.random.default_rng(1000 + W)
    mq, tq, act, r, done, w = _window(rng, B, W, A, bf16=bf16)
    eta = float(np.float32(0.9))
    for n in (1, 2, 5, W + 3):
        want = ref.naive(mq, tq, act, r, done, w, GAMMA, n, eta=eta)
        loss, td, prio = ref.kernel_f32(mq, tq, act, r, done, w, GAMMA, n,
                                        eta=eta, contract=contract)
        err = np.abs(td - want["td"])
        print(f"W={W} n={n}: max td err {err.max() / ref.U:.0f} u, "
              f"bound {want['e'].max() / ref.U:.0f} u")
        assert (err <= want["e"]).all()
        assert want["e"].max() < 2.0 ** -10
        assert abs(loss - want["loss"]) <= ref.loss_bound(want, w)
        assert (np.abs(prio - want["prio"])
                <= ref.prio_bound(want, eta)).all()
        want = ref.naive(mq, tq, act, r, done, w, GAMMA, n, eta=None)
        _, _, prio = ref.kernel_f32(mq, tq, act, r, done, w, GAMMA, n,
                                    eta=None, contract=contract)
        assert (np.abs(prio - want["prio"])
                <= ref.prio_bound(want, None)).all()
