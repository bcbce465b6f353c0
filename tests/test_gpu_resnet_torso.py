"""The IMPALA ResNet torso on the hand-written 3x3 conv kernels: parity with
the library path, dispatch, and the eager and graph-captured agent steps.
GPU-only."""

import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _capture_checks import (
    assert_after_steps, assert_construction_preserved, snapshot,
)

pytestmark = pytest.mark.gpu


def _torso(seed=0):
    from distributed_reinforcement_learning_amd.models.impala_resnet import (
        ImpalaResNetTorso,
    )
    torch.manual_seed(seed)
    return ImpalaResNetTorso(4).to("cuda").to(torch.bfloat16)


def _frames(n=4, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(n, 84, 84, 4, device="cuda", generator=g).bfloat16()


def _run(torso, x, gout):
    """Feature output and the gradients of all parameters, by name."""
    torso.zero_grad(set_to_none=True)
    out = torso(x)
    out.backward(gout.to(out.dtype))
    torch.cuda.synchronize()
    return out.detach(), {n: p.grad.detach().clone()
                          for n, p in torso.named_parameters()}


def _rel(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return float((a - ref).norm() / ref.norm())


def test_torso_parity_with_library_and_float32(monkeypatch):
    """Per tensor (the features and the gradients of all 32 parameters),
    err(path) = ||path - f32|| / ||f32|| against a float32 copy of the module
    holding the same (bf16-valued) weights. Both bf16 paths round every
    activation to bf16 about once per layer, at different points, so their
    errors are of equal order; a layout or border bug gives O(1). Required:
    err(custom) <= max(2 err(library), 2^-7) (2^-7 = two bf16 ulps)."""
    torso = _torso()
    assert len(list(torso.parameters())) == 32
    x = _frames()
    gout = torch.randn(4, 256, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(1))
    ref_mod = copy.deepcopy(torso).float()
    out_f, g_f = _run(ref_mod, x.float(), gout)

    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    out_c, g_c = _run(torso, x, gout)
    monkeypatch.setenv("DRLA_RESNET_CONV", "0")
    out_l, g_l = _run(torso, x, gout)

    rows = [("features", _rel(out_c, out_f), _rel(out_l, out_f))]
    for name in g_f:
        assert float(g_f[name].norm()) > 0, name
        rows.append((name, _rel(g_c[name], g_f[name]),
                     _rel(g_l[name], g_f[name])))
    for name, ec, el in rows:
        print(f"{name}: err(custom) {ec:.3e}  err(library) {el:.3e}")
    print(f"largest err(custom) {max(r[1] for r in rows):.3e}, "
          f"largest err(library) {max(r[2] for r in rows):.3e}")
    bad = [(n, ec, el) for n, ec, el in rows if ec > max(2 * el, 2.0 ** -7)]
    assert not bad, bad


def test_dispatch_and_env_switch(monkeypatch):
    """The op wrapper runs by default and not under DRLA_RESNET_CONV=0, where
    the output is bit-equal to plain nn.Conv2d modules run by hand; the pool
    output of the custom path comes back NHWC-contiguous (no hidden copy)."""
    from distributed_reinforcement_learning_amd.ops import resnet_op
    torso = _torso(seed=2)
    x = _frames(seed=3)
    calls = []
    real = resnet_op.resnet_torso

    def spy(t, xx):
        calls.append(tuple(xx.shape))
        return real(t, xx)

    monkeypatch.setattr(resnet_op, "resnet_torso", spy)
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    with torch.no_grad():
        out_c = torso(x)
    assert calls == [(4, 84, 84, 4)]

    monkeypatch.setenv("DRLA_RESNET_CONV", "0")
    with torch.no_grad():
        out_l = torso(x)
        # the library computation, spelled out
        y = x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        for s in torso.sections:
            y = F.max_pool2d(s.conv(y), 3, stride=2, padding=1)
            for r in (s.r1, s.r2):
                y = y + r.c2(F.relu(r.c1(F.relu(y))))
        plain = F.relu(torso.fc(F.relu(y).permute(0, 2, 3, 1).flatten(1)))
    assert len(calls) == 1
    assert torch.equal(out_l, plain)
    assert out_c.shape == out_l.shape

    monkeypatch.delenv("DRLA_RESNET_CONV")
    with torch.no_grad():
        y = resnet_op.conv3x3(x, torso.sections[0].conv, 4)
        p = F.max_pool2d(y.permute(0, 3, 1, 2), 3, stride=2, padding=1)
    assert p.permute(0, 2, 3, 1).is_contiguous()
    assert p.permute(0, 2, 3, 1).shape == (4, 42, 42, 16)


# ---- agent steps (helpers as in tests/test_gpu_graph.py, resnet arch) -------

def _agent(seed=0):
    from distributed_reinforcement_learning_amd.agents import impala
    return impala.Agent(
        trajectory=8, input_shape=[84, 84, 4], num_action=6,
        lstm_hidden_size=32, discount_factor=0.99, start_learning_rate=1e-3,
        end_learning_rate=0.0, learning_frame=10 ** 9,
        baseline_loss_coef=1.0, entropy_coef=0.05, gradient_clip_norm=40.0,
        reward_clipping="abs_one", device="cuda:0", seed=seed,
        model_arch="resnet")


def _batch(B=4, T=8, A=6, H=32, seed=0):
    rng = np.random.default_rng(seed)
    return dict(
        state=rng.integers(0, 255, (B, T, 84, 84, 4), dtype=np.uint8),
        reward=rng.normal(size=(B, T)).astype(np.float32),
        action=rng.integers(0, A, (B, T)).astype(np.int32),
        done=np.zeros((B, T), dtype=bool),
        behavior_policy=np.full((B, T, A), 1 / A, dtype=np.float32),
        previous_action=rng.integers(0, A, (B, T)).astype(np.int32),
        initial_h=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
        initial_c=(rng.normal(size=(B, T, H)) * 0.1).astype(np.float32),
    )


def _spy_on_torso(monkeypatch):
    from distributed_reinforcement_learning_amd.ops import resnet_op
    calls = []
    real = resnet_op.resnet_torso

    def spy(t, xx):
        calls.append(tuple(xx.shape))
        return real(t, xx)

    monkeypatch.setattr(resnet_op, "resnet_torso", spy)
    return calls


def test_agent_eager_train_step(monkeypatch):
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    calls = _spy_on_torso(monkeypatch)
    agent = _agent(seed=0)
    w0 = agent.optimizer.flat_params.detach().clone()
    out = agent.train(**_batch(seed=0))
    assert calls == [(32, 84, 84, 4)]
    assert all(np.isfinite(float(v)) for v in out[:3])
    assert not torch.equal(agent.optimizer.flat_params, w0)


def test_graphed_step_matches_eager(monkeypatch):
    from distributed_reinforcement_learning_amd.runtime import GraphedImpalaStep
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    calls = _spy_on_torso(monkeypatch)
    torch.manual_seed(0)
    a_eager = _agent(seed=0)
    a_graph = _agent(seed=0)
    a_graph.model.load_state_dict(a_eager.model.state_dict())
    a_graph.optimizer.flat_params.copy_(a_eager.optimizer.flat_params)

    snap = snapshot(a_graph)
    graphed = GraphedImpalaStep(a_graph, batch_size=4)
    assert calls, "the captured step did not take the custom torso"
    # graph construction must not have perturbed weights
    assert torch.equal(a_graph.optimizer.flat_params,
                       a_eager.optimizer.flat_params)
    assert_construction_preserved(a_graph, graphed.lr_buf, snap)

    for i in range(3):
        b = _batch(seed=i)
        out_e = a_eager.train(**b)
        graphed.step(b)
        out_g = graphed.last_losses()
        # bf16 forward: small numeric differences are expected; losses and
        # resulting weights must agree closely
        assert out_g[0] == pytest.approx(out_e[0], rel=5e-2, abs=5e-1)
        assert out_g[3] == out_e[3]  # identical lr schedule
    assert_after_steps(a_graph, graphed.lr_buf, 3)
    assert torch.allclose(a_graph.optimizer.flat_params,
                          a_eager.optimizer.flat_params, atol=1e-2)


def test_graphed_step_updates_weights_every_replay(monkeypatch):
    from distributed_reinforcement_learning_amd.runtime import GraphedImpalaStep
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    calls = _spy_on_torso(monkeypatch)
    agent = _agent(seed=1)
    graphed = GraphedImpalaStep(agent, batch_size=4)
    assert calls, "the captured step did not take the custom torso"
    w0 = agent.optimizer.flat_params.detach().clone()
    graphed.step(_batch(seed=10))
    w1 = agent.optimizer.flat_params.detach().clone()
    graphed.step(_batch(seed=11))
    w2 = agent.optimizer.flat_params.detach().clone()
    assert not torch.equal(w0, w1)
    assert not torch.equal(w1, w2)
    assert agent.global_step == 2
