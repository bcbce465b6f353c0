"""The wide LSTM sequence kernels (drla_lstm_seq_wide_*): hidden sizes past
the LDS-resident train pair (H > 123) and past one thread per gate
(H > 256), up to LSTM_SEQ_MAX_HIDDEN = 512, from the kernels up to the R2D2
agent. GPU-only.

The reference is the float32 torch loop on the same bf16 inputs, the one
tests/test_gpu_kernels.py checks the LDS-resident kernels against, at its
tolerances: forward 2e-2/2e-2, c_fin 3e-2, dxg/dh0/dc0 0.05/0.05, dWh atol
0.35 rtol 0.1. Wh ~ N(0, (1.6/sqrt(H))^2), which is that file's 0.2 at
H = 64 and keeps the pre-activations' spread the same at every H, so the
gates do not saturate at 512.

Observed max |error| (MI355X), train pair B=2 L=3, max|dWh| 2.4 ... 7.7:
    H    h_out   h_fin   c_fin   dxg     dWh     dh0     dc0
    124  2.5e-7  1.5e-7  3.7e-7  3.8e-6  1.6e-2  8.3e-7  9.5e-7
    128  4.8e-7  1.5e-7  3.6e-7  7.5e-9  3.1e-2  9.5e-7  6.6e-7
    141  3.3e-7  2.1e-7  3.9e-7  0       3.1e-2  1.1e-6  6.0e-7
    256  4.5e-7  2.4e-7  4.9e-7  9.5e-7  3.1e-2  1.3e-6  9.5e-7
    257  4.8e-7  2.7e-7  4.8e-7  6.1e-5  3.1e-2  9.5e-7  7.2e-7
    512  8.3e-7  4.2e-7  8.9e-7  1.5e-5  3.1e-2  1.4e-6  1.2e-6
    64   1.3e-7  8.9e-8  3.0e-7  7.6e-6  3.1e-2  1.4e-6  4.8e-7  (LDS pair)
    123  1.9e-7  1.7e-7  3.6e-7  1.5e-5  1.6e-2  6.6e-7  4.2e-7  (LDS pair)
carry through resets (B=3 L=9 H=256): h_out 5.7e-7, dxg 6.1e-5, dWh 3.1e-2,
dh0 7.5e-7. The dWh figure is one bf16 step of the GEMM's output at |dWh|
in [4, 8). No-grad forward at 257 / 512: h_out 3.0e-7 / 5.8e-7 for bf16
and f32 xg alike. Model routes vs the step loop, H = 128 and 512: 4.9e-4
(one bf16 step of Q). Agent fused vs eager: loss 0.08595 vs 0.08593 at
128, equal at 512; priorities within 1e-4.
"""

import numpy as np
import pytest
import torch

from _lstm_ref import lstm_seq_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available(), "HIP extension must be built on the GPU box"
    return ops.require_ext()


def _inputs(B, H, L, seed):
    torch.manual_seed(seed)
    xg = (torch.randn(B, L, 4 * H, device=DEV) * 0.5).to(torch.bfloat16)
    wh = (torch.randn(H, 4 * H, device=DEV) * (1.6 / H ** 0.5)).to(
        torch.bfloat16)
    h0 = torch.randn(B, H, device=DEV)
    c0 = torch.randn(B, H, device=DEV)
    g = torch.randn(B, L, H, device=DEV)
    g1 = torch.randn(B, H, device=DEV)
    g2 = torch.randn(B, H, device=DEV)
    return xg, wh, h0, c0, (g, g1, g2)


def _train_pair(fn, xg, wh, h0, c0, done, gs):
    """outputs and grads of ``fn`` under the loss
    (h_out*g).sum() + (h_fin*g1).sum() + (c_fin*g2).sum()"""
    leaves = [t.detach().clone().requires_grad_(True)
              for t in (xg, wh, h0, c0)]
    h_out, h_fin, c_fin = fn(*leaves, done)
    ((h_out * gs[0]).sum() + (h_fin * gs[1]).sum()
     + (c_fin * gs[2]).sum()).backward()
    return dict(h_out=h_out.detach(), h_fin=h_fin.detach(),
                c_fin=c_fin.detach(), dxg=leaves[0].grad.float(),
                dwh=leaves[1].grad.float(), dh0=leaves[2].grad,
                dc0=leaves[3].grad)


TOL = dict(h_out=(2e-2, 2e-2), h_fin=(2e-2, 2e-2), c_fin=(3e-2, 3e-2),
           dxg=(0.05, 0.05), dwh=(0.35, 0.1), dh0=(0.05, 0.05),
           dc0=(0.05, 0.05))


def _kernel_pair(xg, wh, h0, c0, done, gs):
    from distributed_reinforcement_learning_amd.ops.lstm_op import (
        lstm_seq_train,
    )
    return _train_pair(
        lambda a, b, c, d, dn: lstm_seq_train(a, b, c, d, dn, 1.0),
        xg, wh, h0, c0, done, gs)


def _check_train(B, H, L, done, seed=21):
    xg, wh, h0, c0, gs = _inputs(B, H, L, seed)
    got = _kernel_pair(xg, wh, h0, c0, done, gs)
    ref = _train_pair(lstm_seq_reference, xg, wh, h0, c0, done, gs)
    errs = {k: float((got[k] - ref[k]).abs().max()) for k in TOL}
    print(f"lstm_seq_train H={H} B={B} L={L} max|err| "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" max|dWh|={float(ref['dwh'].abs().max()):.2f}")
    for k, (atol, rtol) in TOL.items():
        assert torch.allclose(got[k], ref[k], atol=atol, rtol=rtol), \
            (k, errs[k])
    return got


# first size the LDS pair refuses, the common 128, first size past the
# LDS-resident forward, the old block cap, first size where a thread owns
# more than one gate (4H = 1028 is no multiple of 64), the new cap
@pytest.mark.parametrize("H", [124, 128, 141, 256, 257, 512])
def test_train_pair_matches_torch_loop(ext, H):
    done = torch.zeros(2, 3, dtype=torch.bool, device=DEV)
    done[0, 1] = True
    _check_train(2, H, 3, done)


def test_train_pair_carries_through_resets(ext):
    torch.manual_seed(5)
    done = torch.rand(3, 9, device=DEV) < 0.15
    _check_train(3, 256, 9, done)


@pytest.mark.parametrize("H", [257, 512])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_no_grad_forward_matches_torch_loop(ext, H, dtype):
    torch.manual_seed(31 + H)
    B, L = 1, 2
    xg = (torch.randn(B, L, 4 * H, device=DEV) * 0.5).to(dtype)
    wh = (torch.randn(H, 4 * H, device=DEV) * (1.6 / H ** 0.5)).to(
        torch.bfloat16)
    h0 = torch.randn(B, H, device=DEV)
    c0 = torch.randn(B, H, device=DEV)
    done = torch.tensor([[True, False]], device=DEV)
    h_out, h_fin, c_fin = ext.lstm_seq_fwd(xg, wh, h0, c0, done, 1.0)
    ref, h, c = lstm_seq_reference(xg, wh, h0, c0, done)
    print(f"lstm_seq_fwd H={H} {dtype} max|err| "
          f"h_out={float((h_out - ref).abs().max()):.2e} "
          f"h_fin={float((h_fin - h).abs().max()):.2e} "
          f"c_fin={float((c_fin - c).abs().max()):.2e}")
    assert torch.allclose(h_out, ref, atol=2e-2, rtol=2e-2)
    assert torch.allclose(h_fin, h, atol=2e-2, rtol=2e-2)
    assert torch.allclose(c_fin, c, atol=3e-2, rtol=3e-2)


def test_hidden_cap_is_named(ext):
    H = 513
    xg = torch.zeros(1, 1, 4 * H, device=DEV, dtype=torch.bfloat16)
    wh = torch.zeros(H, 4 * H, device=DEV, dtype=torch.bfloat16)
    h0 = torch.zeros(1, H, device=DEV)
    done = torch.zeros(1, 1, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match="512"):
        ext.lstm_seq_fwd(xg, wh, h0, h0.clone(), done, 1.0)
    with pytest.raises(RuntimeError, match="512"):
        ext.lstm_seq_train_fwd(xg, wh, h0, h0.clone(), done, 1.0)


@pytest.mark.parametrize("H", [64, 123])
def test_lds_resident_sizes_keep_their_route(ext, H):
    """The sizes the LDS-resident pair took before still run it: within
    the tolerances, and bit-equal across two calls (its sums are
    sequential per thread; a wave-shuffle reduction would also repeat, so
    this guards the dispatch only together with the by-hand comparison
    against the previous commit that KERNELS.md records)."""
    done = torch.zeros(2, 3, dtype=torch.bool, device=DEV)
    done[0, 1] = True
    first = _check_train(2, H, 3, done)
    xg, wh, h0, c0, gs = _inputs(2, H, 3, 21)
    again = _kernel_pair(xg, wh, h0, c0, done, gs)
    for k in TOL:
        assert torch.equal(first[k], again[k]), k


def _model_batch(H, B, L):
    s = torch.randint(0, 256, (B, L, 84, 84, 1), dtype=torch.uint8,
                      device=DEV)
    pa = torch.randint(0, 4, (B, L), device=DEV)
    h0 = torch.randn(B, H, device=DEV) * 0.1
    c0 = torch.randn(B, H, device=DEV) * 0.1
    done = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    done[:, L // 2] = True
    return s, pa, h0, c0, done


@pytest.mark.parametrize("H", [128, 512])
def test_model_routes_match_its_own_step_loop(H):
    from distributed_reinforcement_learning_amd.models import R2D2LstmQ
    torch.manual_seed(11)
    m = R2D2LstmQ([84, 84, 1], 4, H).to(DEV).bfloat16()
    B, L = 2, 4
    s, pa, h0, c0, done = _model_batch(H, B, L)
    with torch.no_grad():
        feat = m.features(s.reshape(B * L, 84, 84, 1).contiguous(),
                          pa.reshape(-1)).reshape(B, L, -1)
        h, c = h0, c0
        qs = []
        for i in range(L):
            h, c = m.lstm(feat[:, i], h, c)
            qs.append(m._head(h))
            keep = (~done[:, i]).to(h.dtype).unsqueeze(1)
            h, c = h * keep, c * keep
        q_loop = torch.stack(qs, dim=1).float()
        q_nograd = m.unroll_sequence(s, pa, h0, c0, done).float()
        q_win = m.q_window(s, pa, h0, c0, done, 1).float()
    q_grad = m.unroll_sequence(s, pa, h0, c0, done)
    for name, q, want in [("grad", q_grad.detach().float(), q_loop),
                          ("no_grad", q_nograd, q_loop),
                          ("q_window", q_win, q_loop[:, 1:])]:
        err = float((q - want).abs().max())
        print(f"R2D2LstmQ H={H} {name} max|err|={err:.2e}")
        assert torch.allclose(q, want, atol=5e-2, rtol=5e-2), (name, err)
    (q_grad.float() * torch.randn_like(q_loop)).sum().backward()
    gw = m.lstm.weight.grad
    assert torch.isfinite(gw).all() and bool((gw != 0).any())


def _agent(L, BI, H, **kw):
    from distributed_reinforcement_learning_amd.agents import r2d2
    return r2d2.Agent(seq_len=L, burn_in=BI, input_shape=[84, 84, 1],
                      num_action=4, lstm_size=H, discount_factor=0.997,
                      start_learning_rate=1e-4, end_learning_rate=0.0,
                      learning_frame=10 ** 9, gradient_clip_norm=40.0,
                      device=DEV, seed=0, **kw)


@pytest.mark.parametrize("H", [128, 512])
def test_agent_train_step(H):
    rng = np.random.default_rng(1)
    B, L = 2, 6
    agent = _agent(L, 2, H)
    before = agent.optimizer.flat_params.detach().clone()
    loss, td = agent.train(
        state=rng.integers(0, 255, (B, L, 84, 84, 1), dtype=np.uint8),
        previous_action=rng.integers(0, 4, (B, L)).astype(np.int32),
        action=rng.integers(0, 4, (B, L)).astype(np.int32),
        h=np.zeros((B, L, H), np.float32), c=np.zeros((B, L, H), np.float32),
        reward=rng.normal(size=(B, L)).astype(np.float32),
        done=np.zeros((B, L), bool), weight=np.ones(B, np.float32))
    assert np.isfinite(loss) and np.isfinite(td).all()
    assert not torch.equal(before, agent.optimizer.flat_params)


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


@pytest.mark.parametrize("H", [128, 512])
def test_agent_fused_path_matches_eager(H):
    B, L, BI = 3, 12, 5
    agent = _agent(L, BI, H, build_optimizer=False)
    b = _sequences(np.random.default_rng(9), B, L, 4, H)
    w = torch.ones(B, device=DEV)
    args = (b["state"], b["previous_action"], b["action"],
            b["initial_h"][:, 0], b["initial_c"][:, 0], b["reward"],
            b["done"])
    assert agent._use_fused_tail()
    loss_f, td_f = agent.compute_sequence_loss(*args, w)
    unweighted, tgt, sav = agent._sequence_losses(*args, with_grad=False)
    loss_e = (unweighted * w).mean()
    td_e = (tgt - sav).mean(dim=1).abs()
    print(f"r2d2 H={H} loss fused={float(loss_f.detach()):.5f} "
          f"eager={float(loss_e):.5f} "
          f"max|td diff|={float((td_f - td_e).abs().max()):.2e}")
    assert float(loss_f.detach()) == pytest.approx(float(loss_e), rel=0.05)
    assert torch.allclose(td_f, td_e, atol=0.05, rtol=0.05)


def test_graphed_replay_step_at_128():
    from distributed_reinforcement_learning_amd.replay.gpu_memory import (
        GpuMemory,
    )
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedReplayStep,
    )
    N, L, BI, A, H = 12, 12, 5, 4, 128
    agent = _agent(L, BI, H, build_optimizer=True)
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
    for _ in range(3):
        loss = float(g.step())
        assert np.isfinite(loss)
        assert (g.td >= 0).all() and torch.isfinite(g.td).all()
        params.append(agent.optimizer.flat_params.detach().clone())
    for a, b in zip(params, params[1:]):
        assert not torch.equal(a, b)
