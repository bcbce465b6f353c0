"""The hand-written 3x3 / stride 2 / padding 1 max-pool (ops/hip/maxpool.hip)
against F.max_pool2d on the CPU in float64: values, taps and the input
gradient are exact, so everything is compared bit for bit. GPU-only."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from distributed_reinforcement_learning_amd import ops
from test_gpu_resnet_torso import _agent, _batch, _frames, _rel, _run, _torso

pytestmark = pytest.mark.gpu

# one pixel, odd and even sizes, H != W, the three production sizes; N > 1
# lets a tile cross an image boundary
SHAPES = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (2, 6, 4), (3, 21, 21),
          (2, 42, 42), (1, 84, 84)]
CASES = [(c, s) for c in (16, 32) for s in SHAPES]


def _reference(x, dy=None):
    """x NHWC with bf16 values -> (y NHWC bf16, tap NHWC uint8, dx NHWC bf16
    or None) of the float64 CPU pool."""
    xd = x.double().permute(0, 3, 1, 2).requires_grad_()
    y, idx = F.max_pool2d(xd, 3, stride=2, padding=1, return_indices=True)
    W = x.shape[2]
    ho = torch.arange(y.shape[2]).view(1, 1, -1, 1)
    wo = torch.arange(y.shape[3]).view(1, 1, 1, -1)
    tap = (idx // W - (2 * ho - 1)) * 3 + (idx % W - (2 * wo - 1))
    dx = None
    if dy is not None:
        y.backward(dy.double().permute(0, 3, 1, 2))
        dx = xd.grad.permute(0, 2, 3, 1).bfloat16()
    return (y.detach().permute(0, 2, 3, 1).bfloat16(),
            tap.permute(0, 2, 3, 1).to(torch.uint8), dx)


@functools.lru_cache(maxsize=None)
def _case(C, shape):
    """Seeded input, integer dy in [-8, 8] and the reference, once per case."""
    N, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + H * W + N)
    x = torch.rand(N, H, W, C, generator=g).bfloat16()
    HO, WO = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(-8, 9, (N, HO, WO, C), generator=g).bfloat16()
    return (x, dy) + _reference(x, dy)


@pytest.mark.parametrize("C,shape", CASES)
def test_forward_exact(C, shape):
    x, _, y_ref, tap_ref, _ = _case(C, shape)
    y, tap = ops.require_ext()._maxpool3s2_fwd(x.cuda(), True)
    assert torch.equal(y.cpu(), y_ref)
    assert torch.equal(tap.cpu(), tap_ref)


def test_forward_constant_input_picks_first_in_bounds_tap():
    x = torch.full((2, 5, 6, 16), 0.5).bfloat16()
    y_ref, tap_ref, _ = _reference(x)
    assert tap_ref[0, 0, 0, 0] == 4 and tap_ref[0, 1, 1, 0] == 0
    y, tap = ops.require_ext()._maxpool3s2_fwd(x.cuda(), True)
    assert torch.equal(y.cpu(), y_ref)
    assert torch.equal(tap.cpu(), tap_ref)


def test_forward_nan_and_minus_inf_values():
    x = _case(16, (3, 5, 7))[0].clone()
    x[0, 2, 3, 1] = float("nan")
    x[1, :3, :3, 2] = float("-inf")   # a whole window of -inf
    x[2, 0, 0, 5] = float("-inf")
    y_ref = _reference(x)[0]
    assert y_ref.isnan().any() and y_ref.isinf().any()
    y, tap = ops.require_ext()._maxpool3s2_fwd(x.cuda(), False)
    assert tap is None
    torch.testing.assert_close(y.cpu(), y_ref, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("C,shape", CASES)
def test_backward_exact(C, shape):
    _, dy, _, tap_ref, dx_ref = _case(C, shape)
    dx = ops.require_ext()._maxpool3s2_bwd(dy.cuda(), tap_ref.cuda(),
                                           shape[1], shape[2])
    assert torch.equal(dx.cpu(), dx_ref)


def test_backward_addend():
    shape = (3, 5, 7)
    _, dy, _, tap_ref, dx_ref = _case(32, shape)
    add = torch.randint(-8, 9, dx_ref.shape,
                        generator=torch.Generator().manual_seed(7)).bfloat16()
    dx = ops.require_ext()._maxpool3s2_bwd(dy.cuda(), tap_ref.cuda(),
                                           shape[1], shape[2],
                                           addend=add.cuda())
    assert torch.equal(dx.cpu(), (dx_ref.float() + add.float()).bfloat16())


def test_launcher_takes_empty_batch_and_rejects_misaligned_input():
    ext = ops.require_ext()
    y, tap = ext._maxpool3s2_fwd(
        torch.empty(0, 5, 7, 16, dtype=torch.bfloat16, device="cuda"), True)
    assert y.shape == tap.shape == (0, 3, 4, 16)
    assert ext._maxpool3s2_bwd(y, tap, 5, 7).shape == (0, 5, 7, 16)
    flat = torch.zeros(5 * 7 * 16 + 4, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 16 bytes"):
        ext._maxpool3s2_fwd(flat[4:].view(1, 5, 7, 16), False)


def test_autograd_function_and_no_grad(monkeypatch):
    ext = ops.require_ext()
    x, dy, y_ref, _, dx_ref = _case(16, (3, 21, 21))
    wanted = []
    real = ext._maxpool3s2_fwd
    monkeypatch.setattr(ext, "_maxpool3s2_fwd",
                        lambda t, w: wanted.append(w) or real(t, w))
    xg = x.cuda().requires_grad_()
    y = ops.max_pool3x3s2(xg)
    y.backward(dy.cuda())
    assert torch.equal(y.detach().cpu(), y_ref)
    assert torch.equal(xg.grad.cpu(), dx_ref)
    with torch.no_grad():
        assert torch.equal(ops.max_pool3x3s2(xg).cpu(), y_ref)
    assert torch.equal(ops.max_pool3x3s2(x.cuda()).cpu(), y_ref)
    assert wanted == [True, False, False]
    # CPU tensors take F.max_pool2d
    assert torch.equal(ops.max_pool3x3s2(x), y_ref)


def test_torso_equal_to_library_pool(monkeypatch):
    """Custom pool against DRLA_RESNET_POOL=0 in the custom torso, N = 4: the
    features and the gradient each pool hands to its section conv are
    bit-equal. The 32 parameter gradients are not bit-equal even between two
    runs with ONE pool (a few weight gradients move by a bf16 ulp, up to
    4.9e-4 absolute: the order of the conv wgrad's f32 atomics), so they are
    held to the criterion of test_torso_parity_with_library_and_float32:
    err(custom pool) <= max(2 err(library pool), 2^-7) against float32."""
    from distributed_reinforcement_learning_amd.ops import resnet_op
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    torso, x = _torso(), _frames()
    gout = torch.randn(4, 256, device="cuda")
    _, g_f = _run(copy.deepcopy(torso).float(), x.float(), gout)
    pool_in = []
    real = resnet_op.conv3x3

    def spy(*a):
        pool_in.append(real(*a))
        pool_in[-1].retain_grad()
        return pool_in[-1]

    monkeypatch.setattr(resnet_op, "conv3x3", spy)
    monkeypatch.delenv("DRLA_RESNET_POOL", raising=False)
    out_c, g_c = _run(torso, x, gout)
    _, g_c2 = _run(torso, x, gout)
    monkeypatch.setenv("DRLA_RESNET_POOL", "0")
    out_l, g_l = _run(torso, x, gout)
    assert len(g_c) == 32 and len(pool_in) == 9
    assert torch.equal(out_c, out_l)
    for i in range(3):
        assert torch.equal(pool_in[i].grad, pool_in[6 + i].grad), i
    for name in g_c:
        ec, el = _rel(g_c[name], g_f[name]), _rel(g_l[name], g_f[name])
        print(f"{name}: max |custom - library| "
              f"{float((g_c[name] - g_l[name]).abs().max()):.3e}, two custom "
              f"runs {float((g_c[name] - g_c2[name]).abs().max()):.3e}, "
              f"err(custom) {ec:.3e}, err(library) {el:.3e}")
        assert ec <= max(2 * el, 2.0 ** -7), name


def test_graphed_step_with_custom_pool(monkeypatch):
    from distributed_reinforcement_learning_amd.ops import pool_op
    from distributed_reinforcement_learning_amd.runtime import GraphedImpalaStep
    monkeypatch.delenv("DRLA_RESNET_CONV", raising=False)
    monkeypatch.delenv("DRLA_RESNET_POOL", raising=False)
    calls = []
    real = pool_op._MaxPool3x3S2.apply
    monkeypatch.setattr(pool_op._MaxPool3x3S2, "apply",
                        lambda *a: calls.append(a[1]) or real(*a))
    agent = _agent(seed=1)
    graphed = GraphedImpalaStep(agent, batch_size=4)
    assert any(calls), "the captured step did not take the custom pool"
    w0 = agent.optimizer.flat_params.detach().clone()
    graphed.step(_batch(seed=10))
    assert not torch.equal(agent.optimizer.flat_params, w0)
