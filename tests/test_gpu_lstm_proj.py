"""The R2D2 LSTM projection kernels (ops/hip/lstm_proj.hip): forward, dgrad and
wgrad exact against float64 CPU products, lstm_seq_layer against the existing
recurrence pieces, parity of R2D2LstmQ with the library path and float32, and
the launcher contract with the model's dispatch. GPU-only."""

import copy
import functools

import pytest
import torch

from distributed_reinforcement_learning_amd import ops
from distributed_reinforcement_learning_amd.models import R2D2LstmQ
from distributed_reinforcement_learning_amd.ops import lstm_op, lstm_proj_op
from test_gpu_resnet_torso import _rel

pytestmark = pytest.mark.gpu

# (M, F1, F2, H): one piece of everything; partial tiles in all three
# dimensions, 4H = 136, h_prev rows starting inside a dW tile; three
# reduction chunks with a remainder in the wgrad; the shipped feature width,
# whose forward the launcher splits (asserted below)
SHAPES = [(1, 64, 8, 2), (65, 64, 40, 34), (130, 128, 8, 16),
          (70, 3136, 256, 32)]
SPLIT_SHAPE = (70, 3136, 256, 32)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded integers in [-4, 4] as bf16 and the float64 CPU products: every
    partial sum is an integer below 2^24, so f32 accumulation in any order is
    exact and the one rounding equals bfloat16() of the float64 result."""
    M, F1, F2, H = shape
    F, N = F1 + F2, 4 * H
    g = torch.Generator().manual_seed(M * 7919 + F1 * 31 + F2 * 7 + H)
    conv, emb, w, b, hp, dxg = (
        torch.randint(-4, 5, s, generator=g).bfloat16()
        for s in ((M, F1), (M, F2), (F + H, N), (N,), (M, H), (M, N)))
    x64 = torch.cat([conv, emb, hp], 1).double()
    w64, d64 = w.double(), dxg.double()
    refs = dict(xg=x64[:, :F] @ w64[:F] + b.double(),
                dconv=d64 @ w64[:F1].t(), demb=d64 @ w64[F1:F].t(),
                dw=x64.t() @ d64, db=d64.sum(0))
    return (conv, emb, w, b, hp, dxg), {k: v.bfloat16()
                                        for k, v in refs.items()}


@pytest.mark.parametrize("shape", SHAPES)
def test_all_three_kernels_exact(shape):
    ext = ops.require_ext()
    M, F1, F2, H = shape
    if shape == SPLIT_SHAPE:
        assert ext._lstm_proj_split(M, F1 + F2, 4 * H) > 1
    ops_cpu, ref = _case(shape)
    conv, emb, w, b, hp, dxg = (t.cuda() for t in ops_cpu)
    got = dict(xg=ext._lstm_proj_fwd(conv, emb, w, b))
    got["dconv"], got["demb"] = ext._lstm_proj_dgrad(dxg, w, F1, F2)
    got["dw"], got["db"] = ext._lstm_proj_wgrad(conv, emb, hp, dxg)
    for name, r in ref.items():
        assert torch.equal(got[name].cpu(), r), name
    # the three row ranges of dW, by name
    F = F1 + F2
    for lo, hi in ((0, F1), (F1, F), (F, F + H)):
        assert torch.equal(got["dw"][lo:hi].cpu(), ref["dw"][lo:hi]), (lo, hi)


def test_seq_layer_against_the_existing_pieces():
    ext = ops.require_ext()
    B, L, H, F1, F2 = 2, 3, 16, 64, 8
    (conv, emb, w, b, _, _), ref = _case((B * L, F1, F2, H))
    conv, emb, w, b = (t.cuda().requires_grad_() for t in (conv, emb, w, b))
    g = torch.Generator(device="cuda").manual_seed(2)
    h0, c0 = (torch.randn(B, H, device="cuda", generator=g) for _ in range(2))
    gout = torch.randn(B, L, H, device="cuda", generator=g)
    done = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    done[1, 0] = True
    out = lstm_proj_op.lstm_seq_layer(conv, emb, w, b, h0, c0, done, 1.0)
    out[0].backward(gout)

    # the same recurrence kernels on the float64-exact xg
    xg = ref["xg"].cuda().view(B, L, 4 * H)
    wh = w.detach()[F1 + F2:].contiguous()
    want = lstm_op.lstm_seq_train(xg, wh, h0, c0, done, 1.0)
    for a, r in zip(out, want):
        assert torch.equal(a, r)
    _, _, _, acts, c_prev, h_prev = ext.lstm_seq_train_fwd(xg, wh, h0, c0,
                                                           done, 1.0)
    dxg = ext.lstm_seq_train_bwd(gout, None, None, acts, c_prev, wh, done)[0]
    dwh = h_prev.view(B * L, H).double().t() @ dxg.view(B * L, 4 * H).double()
    assert torch.equal(w.grad[F1 + F2:], dwh.bfloat16())
    assert conv.grad.shape == conv.shape and emb.grad.shape == emb.shape
    assert b.grad.shape == b.shape


def _model_case():
    torch.manual_seed(11)
    model = R2D2LstmQ([84, 84, 1], 4, 64).cuda().bfloat16()
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.randint(0, 256, (2, 3, 84, 84, 1), dtype=torch.uint8,
                      device="cuda", generator=g)
    pa = torch.randint(0, 4, (2, 3), device="cuda", generator=g)
    h0 = torch.randn(2, 64, device="cuda", generator=g) * 0.1
    done = torch.zeros(2, 3, dtype=torch.bool, device="cuda")
    done[0, 1] = True
    return model, s, pa, h0, done


def test_model_parity_with_library_and_float32(monkeypatch):
    """Q and every parameter gradient of unroll_sequence, and the no-grad
    q_window(burn=1), B = 2, L = 3, one done: err(path) = ||path - f32|| /
    ||f32|| against a float32 copy of the model; required err(custom) <=
    max(2 err(library), 2^-7), the criterion of
    test_torso_parity_with_library_and_float32."""
    model, s, pa, h0, done = _model_case()
    ref_model = copy.deepcopy(model).float()
    gout = torch.randn(2, 3, 4, device="cuda",
                       generator=torch.Generator(device="cuda").manual_seed(6))

    def run(m, state):
        m.zero_grad(set_to_none=True)
        q = m.unroll_sequence(state, pa, h0, h0, done)
        q.backward(gout.to(q.dtype))
        out = {n: p.grad.detach().clone() for n, p in m.named_parameters()
               if p.grad is not None}
        out["q"] = q.detach().clone()
        out["q_window"] = m.q_window(state, pa, h0, h0, done, 1)
        return out

    ext, calls = ops.require_ext(), []
    real = ext._lstm_proj_fwd
    monkeypatch.setattr(ext, "_lstm_proj_fwd",
                        lambda *a: calls.append(1) or real(*a))
    r_f = run(ref_model, s.float() / 255)
    monkeypatch.setenv("DRLA_LSTM_PROJ", "1")
    r_c = run(model, s)
    assert calls == [1, 1]
    monkeypatch.setenv("DRLA_LSTM_PROJ", "0")
    r_l = run(model, s)
    assert calls == [1, 1]
    assert r_f.keys() == r_c.keys() == r_l.keys() and len(r_f) >= 12
    for name in r_f:
        ec, el = _rel(r_c[name], r_f[name]), _rel(r_l[name], r_f[name])
        print(f"{name}: err(custom) {ec:.3e}  err(library) {el:.3e}")
        assert ec <= max(2 * el, 2.0 ** -7), name


def test_launcher_contract_and_dispatch(monkeypatch):
    ext = ops.require_ext()
    monkeypatch.setenv("DRLA_LSTM_PROJ", "1")
    bf = dict(dtype=torch.bfloat16, device="cuda")
    M, F1, F2, H = 3, 64, 8, 4
    conv, emb = torch.ones(M, F1, **bf), torch.ones(M, F2, **bf)
    w, b = torch.ones(F1 + F2 + H, 4 * H, **bf), torch.ones(4 * H, **bf)
    assert lstm_proj_op.lstm_proj_ok(conv, emb, w, b)
    off = torch.ones(M * F1 + 4, **bf)[4:].view(M, F1)
    for args, msg in [
            ((conv.float(), emb.float(), w.float(), b.float()),
             "must be bf16"),
            ((conv.cpu(), emb.cpu(), w.cpu(), b.cpu()), "GPU tensor"),
            ((conv, emb, torch.ones(F1 + F2 + 3, 12, **bf),
              torch.ones(12, **bf)), "multiple of 8"),  # odd H = 3
            ((torch.ones(M, 72, **bf), emb,
              torch.ones(72 + F2 + H, 4 * H, **bf), b), "multiple of 64"),
            ((off, emb, w, b), "multiple of 16 bytes")]:
        assert not lstm_proj_op.lstm_proj_ok(*args), msg
        with pytest.raises(RuntimeError, match=msg):
            ext._lstm_proj_fwd(*args)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ext._lstm_proj_dgrad(torch.ones(M, 4 * H, **bf),
                             torch.ones(72 + F2 + H, 4 * H, **bf), 72, F2)
    with pytest.raises(RuntimeError, match="multiple of 16 bytes"):
        ext._lstm_proj_wgrad(off, emb, torch.ones(M, H, **bf),
                             torch.ones(M, 4 * H, **bf))

    # M = 0: an empty xg, zero dW and db
    assert ext._lstm_proj_fwd(conv[:0], emb[:0], w, b).shape == (0, 4 * H)
    dw, db = ext._lstm_proj_wgrad(conv[:0], emb[:0],
                                  torch.empty(0, H, **bf),
                                  torch.empty(0, 4 * H, **bf))
    assert dw.shape == w.shape and db.shape == b.shape
    assert not dw.any() and not db.any()

    # one projection launch per unroll_sequence (trained and no-grad),
    # q_window and burn_in_states; none under DRLA_LSTM_PROJ=0
    calls = []
    real = ext._lstm_proj_fwd
    monkeypatch.setattr(ext, "_lstm_proj_fwd",
                        lambda *a: calls.append(a[0].shape) or real(*a))
    model, s, pa, h0, done = _model_case()

    def all_uses():
        model.unroll_sequence(s, pa, h0, h0, done).sum().backward()
        with torch.no_grad():
            model.unroll_sequence(s, pa, h0, h0, done)
        model.q_window(s, pa, h0, h0, done, 1)
        model.burn_in_states(s, pa, h0, h0, done)

    all_uses()
    assert calls == [(6, 3136)] * 4
    monkeypatch.setenv("DRLA_LSTM_PROJ", "0")
    assert not lstm_proj_op.lstm_proj_ok(conv, emb, w, b)
    all_uses()
    assert len(calls) == 4
