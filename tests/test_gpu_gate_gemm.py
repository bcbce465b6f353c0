"""The hand-written LSTM gate GEMM (ops/hip/gate_gemm.hip): forward, dgrad and
wgrad exact against the float64 CPU product, the launcher contract, parity of
the H = 32 agent with the library GEMM and float32, and the captured step.
GPU-only."""

import copy
import functools

import pytest
import torch

from distributed_reinforcement_learning_amd import ops
from distributed_reinforcement_learning_amd.ops import gate_gemm_op
from test_gpu_resnet_torso import _batch, _rel
from test_gpu_xh_slab import _agent

pytestmark = pytest.mark.gpu

# (M, K, N): one piece; one partial tile; partial tiles in all three
# dimensions; several chunks with a k remainder of 8; the slab row of the
# H = 32 agent, whose forward the launcher splits (asserted below)
SHAPES = [(1, 8, 8), (6, 40, 64), (65, 72, 136), (130, 264, 128),
          (70, 3432, 128)]
SPLIT_SHAPE = (70, 3432, 128)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded integers in [-4, 4] as bf16 and the float64 CPU products: every
    partial sum is an integer below 2^24, so f32 accumulation in any order is
    exact and the one rounding equals bfloat16() of the float64 result."""
    M, K, N = shape
    g = torch.Generator().manual_seed(M * 7919 + K * 31 + N)
    xh, w, dg = (torch.randint(-4, 5, s, generator=g).bfloat16()
                 for s in ((M, K), (K, N), (M, N)))
    return (xh, w, dg, (xh.double() @ w.double()).bfloat16(),
            dg.double() @ w.double().t(),
            (xh.double().t() @ dg.double()).bfloat16())


# grad_cols: all columns, and a value with live and dead columns inside one
# 64-column tile (for K > 68 a wholly dead tile follows it)
@pytest.mark.parametrize("dead", [0, 68])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_three_kernels_exact(shape, dead, monkeypatch):
    monkeypatch.setenv("DRLA_GATE_GEMM", "1")  # all three directions custom
    xh, w, dg, g_ref, dxh_ref, dw_ref = _case(shape)
    K = shape[1]
    grad_cols = max(4, K - dead)
    if shape == SPLIT_SHAPE:
        assert ops.require_ext()._gate_gemm_split(*shape) > 1
    x = xh.cuda().requires_grad_()
    wt = w.cuda().requires_grad_()
    assert ops.gate_gemm_ok(x, wt)
    out = ops.gate_gemm(x, wt, grad_cols)
    out.backward(dg.cuda())
    dxh_ref = dxh_ref.clone()
    dxh_ref[:, grad_cols:] = 0
    assert torch.equal(out.detach().cpu(), g_ref)
    assert torch.equal(x.grad.cpu(), dxh_ref.bfloat16())
    assert torch.equal(wt.grad.cpu(), dw_ref)


def _cell_inputs(n):
    g = torch.Generator(device="cuda").manual_seed(3)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return ([mk(n, 3136).bfloat16(), mk(n, 256).bfloat16(), mk(n, 32)],
            mk(n, 32))


def test_launcher_contract_and_dispatch(monkeypatch):
    ext = ops.require_ext()
    monkeypatch.delenv("DRLA_GATE_GEMM", raising=False)
    bf = dict(dtype=torch.bfloat16, device="cuda")
    w = torch.ones(16, 8, **bf)
    empty = torch.empty(0, 16, **bf)
    assert ext._gate_gemm_fwd(empty, w).shape == (0, 8)
    assert ext._gate_gemm_dgrad(torch.empty(0, 8, **bf), w, 16).shape == (0, 16)
    dw = ext._gate_gemm_wgrad(empty, torch.empty(0, 8, **bf))
    assert dw.shape == (16, 8) and not dw.any()
    off = torch.ones(2 * 16 + 4, **bf)[4:].view(2, 16)
    with pytest.raises(RuntimeError, match="multiple of 16 bytes"):
        ext._gate_gemm_fwd(off, w)
    odd = torch.ones(2, 12, **bf)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext._gate_gemm_fwd(odd, torch.ones(12, 8, **bf))
    good = torch.ones(2, 16, **bf)
    assert ops.gate_gemm_ok(good, w)
    assert not ops.gate_gemm_ok(off, w)
    assert not ops.gate_gemm_ok(odd, torch.ones(12, 8, **bf))
    assert not ops.gate_gemm_ok(good.float(), w.float())
    assert not ops.gate_gemm_ok(good.cpu(), w.cpu())

    # forward_cat: the custom GEMM by default, never under DRLA_GATE_GEMM=0
    calls = []
    real = ext._gate_gemm_fwd
    monkeypatch.setattr(ext, "_gate_gemm_fwd",
                        lambda *a: calls.append(a[0].shape) or real(*a))
    model = _agent(32, 6, 3).model
    parts, c = _cell_inputs(5)
    with torch.no_grad():
        h_custom, _ = model.lstm.forward_cat(parts, c)
        assert calls == [(5, 3136 + 256 + 32 + 8)]
        monkeypatch.setenv("DRLA_GATE_GEMM", "0")
        assert not ops.gate_gemm_ok(good, w)
        h_lib, _ = model.lstm.forward_cat(parts, c)
    assert len(calls) == 1
    assert torch.allclose(h_custom, h_lib, atol=2.0 ** -6)


def test_unroll_features_parity_with_library_and_float32(monkeypatch):
    """h and every parameter gradient of _unroll_features, B * T = 6 rows:
    err(path) = ||path - f32|| / ||f32|| against a float32 copy of the model;
    required err(custom) <= max(2 err(library), 2^-7), the criterion of
    test_torso_parity_with_library_and_float32."""
    B, T, A, H = 2, 3, 6, 32
    model = _agent(H, A, T).model
    ref_model = copy.deepcopy(model).float()
    g = torch.Generator(device="cuda").manual_seed(5)
    state = torch.randint(0, 256, (B, T, 84, 84, 4), dtype=torch.uint8,
                          device="cuda", generator=g)
    pa = torch.randint(0, A, (B, T), device="cuda", generator=g)
    h0, c0 = (torch.randn(B, T, H, device="cuda", generator=g) * 0.5
              for _ in range(2))
    gout = torch.randn(B * T, H, device="cuda", generator=g)

    def run(m, s):
        m.zero_grad(set_to_none=True)
        new_h, _, _ = m._unroll_features(s, pa, h0, c0)
        new_h.backward(gout)
        out = {n: p.grad.detach().clone() for n, p in m.named_parameters()
               if p.grad is not None}
        out["h"] = new_h.detach().clone()
        return out

    calls = []
    real = gate_gemm_op._GateGemm.apply
    monkeypatch.setattr(gate_gemm_op._GateGemm, "apply",
                        lambda *a: calls.append(a[2]) or real(*a))
    r_f = run(ref_model, state.float() / 255)
    monkeypatch.setenv("DRLA_GATE_GEMM", "1")  # all three directions custom
    r_c = run(model, state)
    assert calls == [3136 + 256], "the slab path passes grad_cols"
    monkeypatch.setenv("DRLA_GATE_GEMM", "0")
    r_l = run(model, state)
    assert len(calls) == 1
    assert r_f.keys() == r_c.keys() == r_l.keys() and len(r_f) >= 11
    for name in r_f:
        ec, el = _rel(r_c[name], r_f[name]), _rel(r_l[name], r_f[name])
        print(f"{name}: err(custom) {ec:.3e}  err(library) {el:.3e}")
        assert ec <= max(2 * el, 2.0 ** -7), name


def test_graphed_step_with_custom_gate_gemm(monkeypatch):
    from distributed_reinforcement_learning_amd.runtime import GraphedImpalaStep
    monkeypatch.delenv("DRLA_GATE_GEMM", raising=False)
    calls = []
    real = gate_gemm_op._GateGemm.apply
    monkeypatch.setattr(gate_gemm_op._GateGemm, "apply",
                        lambda *a: calls.append(a[2]) or real(*a))
    agent = _agent(32, 6, 8)
    graphed = GraphedImpalaStep(agent, batch_size=4)
    assert calls, "the captured step did not take the custom gate GEMM"
    w0 = agent.optimizer.flat_params.detach().clone()
    graphed.step(_batch(seed=10))
    assert not torch.equal(agent.optimizer.flat_params, w0)
