"""The Ape-X dueling Q head kernels (ops/hip/dueling_q.hip): forward and all
thirteen gradients exact against a float64 CPU run, the launcher contract and
the model's dispatch, parity of ApexDuelingQ with the library path and
float32, and the captured replay step. GPU-only."""

import copy
import functools

import numpy as np
import pytest
import torch

from distributed_reinforcement_learning_amd import ops
from distributed_reinforcement_learning_amd.models import ApexDuelingQ
from distributed_reinforcement_learning_amd.models.blocks import MLPHead
from distributed_reinforcement_learning_amd.ops import dueling_q_op

pytestmark = pytest.mark.gpu

# (N, K, A, grad_rows): one piece; a partial row block and a k remainder of 8;
# several row blocks with the dead rows starting on a block boundary; the
# model's K (split first layer, asserted below) with the dead rows starting
# inside a block; the widest A with every row live
CASES = [(1, 8, 1, 1), (17, 72, 3, 17), (130, 264, 4, 64),
         (65, 3392, 18, 33), (65, 3392, 32, 65)]


@functools.lru_cache(maxsize=None)
def _case(case):
    """Seeded small integers: feat and dQ in [-1, 1] (dQ rows >= grad_rows
    zero), every weight row min(8, K) / 4 / 3 entries of +-1 (layers 1 / 2 /
    3), biases in [-2, 2]. Then z1, z2, dz2, dz1 and d3m are integers far
    below 256 (exact in bf16), every f32 sum is an exact integer, and each
    output has one rounding: bfloat16() of the float64 CPU result.
    Returns feat, dQ, the two float32 CPU heads, Q and the 13 gradients
    (feat, then each head's parameters in order)."""
    N, K, A, G = case
    g = torch.Generator().manual_seed(N * 7919 + K * 31 + A)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def head(out):
        m = MLPHead(K, [256, 256], out, None)
        for lin, nnz in zip([*m.hidden, m.out], (min(8, K), 4, 3)):
            rows, cols = lin.weight.shape
            where = torch.rand(rows, cols, generator=g).argsort(1)[:, :nnz]
            w = torch.zeros(rows, cols).scatter_(
                1, where, ints(0, 1, rows, nnz) * 2 - 1)
            lin.weight.data.copy_(w)
            lin.bias.data.copy_(ints(-2, 2, rows))
        return m

    feat, dq, vb, mb = ints(-1, 1, N, K), ints(-1, 1, N, A), head(A), head(1)
    dq[G:] = 0
    f64 = feat.double().requires_grad_()
    v64, m64 = copy.deepcopy(vb).double(), copy.deepcopy(mb).double()
    q = v64(f64) - m64(f64)
    q.backward(dq.double())
    grads = [f64.grad] + [p.grad for p in [*v64.parameters(),
                                           *m64.parameters()]]
    return (feat, dq, vb, mb, q.detach().bfloat16(),
            [x.bfloat16() for x in grads])


@pytest.mark.parametrize("case", CASES)
def test_forward_and_every_gradient_exact(case, monkeypatch):
    monkeypatch.setenv("DRLA_DUELING_HEAD", "1")
    N, K, A, G = case
    feat, dq, vb, mb, q_ref, g_ref = _case(case)
    if K == 3392:
        assert ops.require_ext()._dq_l1_split(N, K) > 1
    vb, mb = (copy.deepcopy(m).cuda().bfloat16() for m in (vb, mb))
    x = feat.cuda().bfloat16().requires_grad_()
    assert ops.dueling_q_ok(x, vb, mb)
    q = ops.dueling_q(x, vb, mb, G)
    q.backward(dq.cuda().bfloat16())
    with torch.no_grad():
        assert torch.equal(ops.dueling_q(x, vb, mb).cpu(), q_ref)
    assert torch.equal(q.detach().cpu(), q_ref)
    got = [x.grad] + [p.grad for p in [*vb.parameters(), *mb.parameters()]]
    assert len(got) == len(g_ref) == 13
    assert not g_ref[0][G:].any()
    for i, (a, b) in enumerate(zip(got, g_ref)):
        assert torch.equal(a.cpu(), b), f"gradient {i}"


def test_launcher_contract_and_dispatch(monkeypatch):
    monkeypatch.delenv("DRLA_DUELING_HEAD", raising=False)
    N, K, A = 17, 72, 3

    def head(k, hidden, out):
        return MLPHead(k, hidden, out, None).cuda().bfloat16()

    feat = torch.zeros(N, K, device="cuda", dtype=torch.bfloat16)
    vb, mb = head(K, [256, 256], A), head(K, [256, 256], 1)
    with torch.no_grad():
        assert ops.dueling_q_ok(feat, vb, mb)
        assert ops.dueling_q(feat[:0], vb, mb).shape == (0, A)
        shifted = torch.zeros(N * K + 4, device="cuda",
                              dtype=torch.bfloat16)[4:].view(N, K)
        for f, v, m, msg in [
                (shifted, vb, mb, "16 bytes"),
                (feat[:, :12], head(12, [256, 256], A),
                 head(12, [256, 256], 1), "multiple of 8"),
                (feat, head(K, [256, 256], 33), mb, "1 to 32 actions"),
                (feat, head(K, [128, 128], A), head(K, [128, 128], 1),
                 r"\(256, 256\)")]:
            assert not ops.dueling_q_ok(f, v, m), msg
            with pytest.raises(RuntimeError, match=msg):
                ops.dueling_q(f, v, m)
        assert not ops.dueling_q_ok(feat.float(), vb.float(), mb.float())
        assert not ops.dueling_q_ok(feat.cpu(), vb.cpu(), mb.cpu())

        calls = []
        real = dueling_q_op.dueling_q
        monkeypatch.setattr(dueling_q_op, "dueling_q",
                            lambda *a: calls.append(a[3]) or real(*a))
        model = ApexDuelingQ((84, 84, 4), 4).cuda().bfloat16()
        s = torch.zeros(2, 84, 84, 4, dtype=torch.uint8, device="cuda")
        pa = torch.zeros(2, dtype=torch.long, device="cuda")
        assert model(s, pa).shape == (2, 4) and calls == [None]
        monkeypatch.setenv("DRLA_DUELING_HEAD", "0")
        assert model(s, pa).shape == (2, 4) and calls == [None]


def test_model_parity_with_library_and_float32(monkeypatch):
    """Q and every parameter gradient of ApexDuelingQ, 6 frames of which 3
    get a gradient: err(path) = ||path - f32|| / ||f32|| against a float32
    copy of the model; required err(custom) <= max(2 err(library), 2^-7), the
    criterion of test_unroll_features_parity_with_library_and_float32."""
    torch.manual_seed(11)
    model = ApexDuelingQ((84, 84, 4), 4).cuda().bfloat16()
    ref_model = copy.deepcopy(model).float()
    g = torch.Generator(device="cuda").manual_seed(5)
    state = torch.randint(0, 256, (6, 84, 84, 4), dtype=torch.uint8,
                          device="cuda", generator=g)
    pa = torch.randint(0, 4, (6,), device="cuda", generator=g)
    gout = torch.randn(6, 4, device="cuda", generator=g)
    gout[3:] = 0

    def run(m, s):
        m.zero_grad(set_to_none=True)
        q = m(s, pa, grad_rows=3)
        q.backward(gout.to(q.dtype))
        out = {n: p.grad.detach().float() for n, p in m.named_parameters()}
        out["q"] = q.detach().float()
        return out

    r_f = run(ref_model, state.float() / 255)
    monkeypatch.setenv("DRLA_DUELING_HEAD", "1")
    r_c = run(model, state)
    monkeypatch.setenv("DRLA_DUELING_HEAD", "0")
    r_l = run(model, state)
    assert r_f.keys() == r_c.keys() == r_l.keys() and len(r_f) >= 13
    for name in r_f:
        ec, el = ((r[name] - r_f[name]).norm() / r_f[name].norm()
                  for r in (r_c, r_l))
        print(f"{name}: err(custom) {ec:.3e}  err(library) {el:.3e}")
        assert ec <= max(2 * el, 2.0 ** -7), name


def test_captured_replay_step_takes_the_head(monkeypatch):
    from distributed_reinforcement_learning_amd.agents import apex
    from distributed_reinforcement_learning_amd.replay.gpu_memory import (
        GpuMemory,
    )
    from distributed_reinforcement_learning_amd.runtime import (
        GraphedReplayStep,
    )
    monkeypatch.delenv("DRLA_DUELING_HEAD", raising=False)
    calls = []
    real = dueling_q_op.dueling_q
    monkeypatch.setattr(dueling_q_op, "dueling_q",
                        lambda *a: calls.append(a[3]) or real(*a))
    A, T, B = 4, 32, 8
    agent = apex.Agent(
        input_shape=[84, 84, 4], num_action=A, discount_factor=0.99,
        gradient_clip_norm=40.0, reward_clipping="abs_one",
        start_learning_rate=1e-4, end_learning_rate=0.0,
        learning_frame=10 ** 9, device="cuda:0", build_optimizer=True, seed=5)
    frame = ((84, 84, 4), torch.uint8)
    mem = GpuMemory(256, fields={
        "state": frame, "next_state": frame,
        "previous_action": ((), torch.int32), "action": ((), torch.int32),
        "reward": ((), torch.float32), "done": ((), torch.bool)},
        device="cuda:0", seed=5)
    rng = np.random.default_rng(2)
    u = {"state": rng.integers(0, 255, (T, 84, 84, 4), dtype=np.uint8),
         "next_state": rng.integers(0, 255, (T, 84, 84, 4), dtype=np.uint8),
         "previous_action": rng.integers(0, A, T).astype(np.int32),
         "action": rng.integers(0, A, T).astype(np.int32),
         "reward": rng.normal(size=T).astype(np.float32),
         "done": rng.random(T) < 0.05}
    u = {k: torch.as_tensor(v).cuda() for k, v in u.items()}
    mem.add_batch(agent.get_td_error(*u.values(), as_tensor=True), u)
    assert calls and set(calls) == {None}, "get_td_error: no-grad calls only"
    del calls[:]

    def loss_fn(b, w):
        return agent.compute_distributed_loss(
            agent.frames_to_device(b["state"]),
            agent.frames_to_device(b["next_state"]),
            b["previous_action"].long(), b["action"].long(),
            b["reward"], b["done"], w)

    graphed = GraphedReplayStep(agent, mem, B, loss_fn)
    assert B in calls and None in calls, "main net with grad_rows, target net"
    w0 = agent.optimizer.flat_params.detach().clone()
    losses = [float(graphed.step()) for _ in range(2)]
    assert all(np.isfinite(losses))
    assert not torch.equal(agent.optimizer.flat_params, w0)
