"""Conv stack backward with the ReLU mask and the bias column sums inside the
dgrad epilogue (conv_dgrad(mask_src=, slot=)), wgrads that leave their
finalize to ONE _conv_wgrad_finalize_all launch, and the stack as a single
autograd node (ops/conv_op._ConvStack). GPU-only.

Masked dX is held bit-equal to relu_mask_bwd(conv_dgrad(...)). Every dW and
dbias is held to the derived elementwise bound of
tests/test_gpu_conv_wgrad_exact.py against a float64 reference built from the
bit-identical masked dY:

    |got - ref| <= 2^-8 |ref| + M 2^-23 S,   S = |A|^T |dY|  (dbias: sum |dY|)

Batches 1 and 3: at N = 3 layer 3's dgrad has 243 rows (two tiles, the second
ragged) and layer 2's 300 rows in each of its four classes (three tiles, the
last ragged).
"""

import functools

import pytest
import torch

from test_gpu_conv_wgrad_exact import (
    GEOM, _assert_within, _inputs, _reference,
)

pytestmark = pytest.mark.gpu

N_CONV = 7 * 7 * 64
SLAB_R = N_CONV + 256 + 32 + 8  # the gate-GEMM slab row of an H = 32 agent


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available()
    return ops.require_ext()


def _drain(ext, layer):
    """Zero a layer's bias-grad slot set again (and its scratch, which a
    default conv_wgrad leaves zero anyway)."""
    x, dy, _ = _inputs(layer, 1, seed=999)
    ext.conv_wgrad(layer, x, dy)


def _mask_source(shape, gen):
    """A forward output: relu(randn) in bf16, about half exact zeros, a few
    of them -0.0 (which must clear like +0)."""
    y = torch.relu(torch.randn(shape, device="cuda", generator=gen)).bfloat16()
    flat = y.view(-1)
    idx = torch.nonzero(flat == 0).flatten()[:7]
    assert idx.numel() == 7
    flat[idx] = -0.0
    assert bool(torch.signbit(flat[idx].float()).all())
    return y


def _colsum_check(name, dbias, masked):
    """dbias against the float64 column sum of the masked tensor."""
    co = masked.shape[-1]
    B = masked.double().reshape(-1, co)
    M = B.shape[0]
    ref = B.sum(0)
    tol = 2.0 ** -8 * ref.abs() + M * 2.0 ** -23 * B.abs().sum(0)
    _assert_within(name, dbias, ref, tol)


# ---- 1. masked dgrad -------------------------------------------------------

# (layer, layer below = slot set the dgrad fills, another slot set for the
# reference relu_mask_bwd)
MASKED_CASES = [(2, 0, 1), (2, 1, 0), (3, 2, 3)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("layer,below,other", MASKED_CASES)
def test_masked_dgrad_bit_equal_and_bias_sums(ext, layer, below, other, batch):
    ci, co, k, s, hi, ho, _ = GEOM[layer]
    assert GEOM[below][1] == ci and GEOM[below][5] == hi
    gen = torch.Generator(device="cuda").manual_seed(100 * layer + below)
    w = (torch.randn(co, k * k * ci, device="cuda", generator=gen)
         * 0.05).bfloat16()
    x_below, _, _ = _inputs(below, batch, seed=70 + below)
    try:
        for rnd in range(2):
            dy = torch.randn(batch, ho, ho, co, device="cuda",
                             generator=gen).bfloat16()
            y_prev = _mask_source((batch, hi, hi, ci), gen)
            ref = ext.relu_mask_bwd(ext.conv_dgrad(layer, dy, w), y_prev, ci,
                                    other)
            got = ext.conv_dgrad(layer, dy, w, mask_src=y_prev, slot=below)
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
            # the wgrad of the layer below drains what the epilogue summed;
            # round 1 within the same bound shows the slots were re-zeroed
            _, dbias = ext.conv_wgrad(below, x_below, got)
            torch.cuda.synchronize()
            _colsum_check(f"dbias l{layer} under l{below} N{batch} r{rnd}",
                          dbias, got)
    finally:
        _drain(ext, other)


def test_masked_dgrad_rejects_bad_slot(ext):
    _, dy, _ = _inputs(3, 1, seed=1)
    w = torch.zeros(64, 576, device="cuda", dtype=torch.bfloat16)
    y2 = torch.ones(1, 9, 9, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.conv_dgrad(3, dy, w, mask_src=y2, slot=0)
    with pytest.raises(RuntimeError):
        ext.conv_dgrad(3, dy, w, mask_src=y2)
    with pytest.raises(RuntimeError):
        ext.conv_dgrad(3, dy, w, slot=2)


# ---- 2. deferred wgrads + one finalize -------------------------------------

def _queue_wgrad(ext, layer, batch, seed):
    """relu_mask_bwd + conv_wgrad(finalize=False); returns the reference."""
    x, dy, y = _inputs(layer, batch, seed)
    dy_m = ext.relu_mask_bwd(dy, y, GEOM[layer][1], layer)
    none = ext.conv_wgrad(layer, x, dy_m, finalize=False)
    assert none[0] is None and none[1] is None
    return _reference(layer, x, dy, y)


def _check_pair(tag, pair, reference):
    ref, tol, ref_db, tol_db = reference
    _assert_within(f"dw {tag}", pair[0], ref, tol)
    _assert_within(f"dbias {tag}", pair[1], ref_db, tol_db)


@pytest.mark.parametrize("l1", [0, 1])
def test_three_wgrads_one_finalize(ext, l1):
    layers = [l1, 2, 3]
    for rnd in range(2):  # round 1: scratch and slots came back to zero
        refs = [_queue_wgrad(ext, layer, 3, seed=200 + 10 * rnd + layer)
                for layer in (3, 2, l1)][::-1]
        pairs = ext._conv_wgrad_finalize_all(layers)
        torch.cuda.synchronize()
        assert len(pairs) == 3
        for layer, pair, reference in zip(layers, pairs, refs):
            _check_pair(f"layer {layer} round {rnd}", pair, reference)


def test_finalize_subset_leaves_other_layers_alone(ext):
    ref2 = _queue_wgrad(ext, 2, 3, seed=231)
    ref3 = _queue_wgrad(ext, 3, 3, seed=232)
    (pair3,) = ext._conv_wgrad_finalize_all([3])
    (pair2,) = ext._conv_wgrad_finalize_all([2])  # still whole after [3]
    torch.cuda.synchronize()
    _check_pair("layer 3 alone", pair3, ref3)
    _check_pair("layer 2 after [3]", pair2, ref2)
    # a default conv_wgrad of layer 2 on fresh inputs finds zeros
    x, dy, y = _inputs(2, 2, seed=233)
    pair = ext.conv_wgrad(2, x, ext.relu_mask_bwd(dy, y, 64, 2))
    torch.cuda.synchronize()
    _check_pair("layer 2 default after subset", pair, _reference(2, x, dy, y))
    with pytest.raises(RuntimeError):
        ext._conv_wgrad_finalize_all([2, 2])
    with pytest.raises(RuntimeError):
        ext._conv_wgrad_finalize_all([])


# ---- 3. whole stack --------------------------------------------------------

def _stack(C):
    from distributed_reinforcement_learning_amd.models.blocks import (
        AtariConvStack,
    )
    torch.manual_seed(300 + C)
    return AtariConvStack(C).cuda().to(torch.bfloat16)


def _flat(conv_weight_like):
    return conv_weight_like.permute(0, 2, 3, 1).reshape(
        conv_weight_like.shape[0], -1)


@functools.lru_cache(maxsize=None)
def _stack_case(C):
    """Stack, inputs, the forward output and the float64 references of all
    three layers at N = 3, from the per-layer ops: each layer's reference
    comes from its bit-identical masked dY (case 1 pins those bits for the
    fused path), so both paths answer to the same numbers."""
    from distributed_reinforcement_learning_amd import ops
    ext = ops.require_ext()
    l1 = 0 if C == 4 else 1
    stack = _stack(C)
    gen = torch.Generator(device="cuda").manual_seed(310 + C)
    x = torch.randint(0, 256, (3, 84, 84, C), dtype=torch.uint8,
                      device="cuda", generator=gen)
    dy3 = torch.randn(3, 7, 7, 64, device="cuda", generator=gen).bfloat16()
    w = {i: _flat(c.weight.detach()).contiguous()
         for i, c in ((1, stack.conv1), (2, stack.conv2), (3, stack.conv3))}
    b = {i: c.bias.detach()
         for i, c in ((1, stack.conv1), (2, stack.conv2), (3, stack.conv3))}
    y1, _ = ext.conv_fwd(l1, x, w[1], b[1], False)
    y2, _ = ext.conv_fwd(2, y1, w[2], b[2], False)
    y3, _ = ext.conv_fwd(3, y2, w[3], b[3], False)
    m3 = ext.relu_mask_bwd(dy3, y3, 64, 3)
    ext.conv_wgrad(3, y2, m3)
    m2 = ext.relu_mask_bwd(ext.conv_dgrad(3, m3, w[3]), y2, 64, 2)
    ext.conv_wgrad(2, y1, m2)
    m1 = ext.relu_mask_bwd(ext.conv_dgrad(2, m2, w[2]), y1, 32, l1)
    ext.conv_wgrad(l1, x, m1)
    torch.cuda.synchronize()
    refs = {}
    for i, layer, xin, m in ((1, l1, x, m1), (2, 2, y1, m2), (3, 3, y2, m3)):
        refs[i] = _reference(layer, xin, m, torch.ones_like(m))
    return stack, x, dy3, y3.reshape(3, -1), refs


def _run_stack(stack, x, dy3, slab, fused, zero=True):
    from distributed_reinforcement_learning_amd.ops import conv_op
    N = x.shape[0]
    if zero:
        stack.zero_grad(set_to_none=True)
    saved = conv_op.FUSED_BWD
    conv_op.FUSED_BWD = fused
    try:
        if slab:
            xh = torch.zeros(N, SLAB_R, device="cuda", dtype=torch.bfloat16)
            dxh = torch.zeros(N, SLAB_R, device="cuda", dtype=torch.bfloat16)
            dxh[:, :N_CONV] = dy3.reshape(N, -1)
            y = conv_op.atari_conv_stack(stack, x, out_slab=xh)
            assert y.stride() == (SLAB_R, 448, 64, 1)
            y.backward(dxh[:, :N_CONV].view(N, 7, 7, 64))
        else:
            y = conv_op.atari_conv_stack(stack, x)
            y.backward(dy3.reshape(N, -1))
    finally:
        conv_op.FUSED_BWD = saved
    torch.cuda.synchronize()
    return y.detach().reshape(N, -1).clone(), _grads(stack)


def _grads(stack):
    return {i: (_flat(c.weight.grad).clone(), c.bias.grad.clone())
            for i, c in ((1, stack.conv1), (2, stack.conv2), (3, stack.conv3))}


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("C", [4, 1])
def test_stack_fused_and_per_layer_paths(ext, C, slab):
    from distributed_reinforcement_learning_amd.ops import conv_op
    stack, x, dy3, y_ref, refs = _stack_case(C)
    assert conv_op.custom_stack_ok(stack, x)
    y_old, g_old = _run_stack(stack, x, dy3, slab, fused=False)
    y_new, g_new = _run_stack(stack, x, dy3, slab, fused=True)
    assert torch.equal(y_new, y_old) and torch.equal(y_new, y_ref)
    for path, grads in (("per-layer", g_old), ("fused", g_new)):
        for i in (1, 2, 3):
            _check_pair(f"{path} C{C} slab{int(slab)} conv{i}", grads[i],
                        refs[i])


# ---- 4. eager accumulation into existing .grad ----------------------------

def test_eager_backward_accumulates_twice(ext):
    """AccumulateGrad adds a returned gradient into .grad at once, so every
    dW and dbias must be final when the node's backward returns. .grad is
    bf16, so the two in-place adds round, each by at most half an ulp, which
    is u = 2^-8 of the sum: with G1, G2 the two gradients (each within tol of
    ref) the result is fl(fl(g0 + G1) + G2), and

        e1 = tol + u (|g0 + ref| + tol)
        e2 = e1 + tol + u (|g0 + 2 ref| + e1 + tol)

    bounds it against g0 + 2 ref: the sum of the two gradient bounds plus the
    two bf16 roundings of the accumulation itself."""
    from distributed_reinforcement_learning_amd.ops import conv_op

    class Net(torch.nn.Module):
        def __init__(self, stack):
            super().__init__()
            self.conv = stack

        def forward(self, x):
            return conv_op.atari_conv_stack(self.conv, x)

    stack, x, dy3, _, refs = _stack_case(4)
    net = Net(stack)
    gen = torch.Generator(device="cuda").manual_seed(400)
    for p in net.parameters():
        p.grad = (torch.randn(p.shape, device="cuda", generator=gen) * 0.25
                  ).to(p.dtype).contiguous(
                      memory_format=torch.channels_last if p.dim() == 4
                      else torch.contiguous_format)
    assert all(bool((p.grad != 0).any()) for p in net.parameters())
    g0 = {i: tuple(t.double() for t in pair)
          for i, pair in _grads(stack).items()}
    assert conv_op.FUSED_BWD
    for _ in range(2):
        net(x).backward(dy3.reshape(3, -1))
    torch.cuda.synchronize()
    got = _grads(stack)
    stack.zero_grad(set_to_none=True)
    for i in (1, 2, 3):
        ref, tol, ref_db, tol_db = refs[i]
        for name, g, start, r, t in (("dw", got[i][0], g0[i][0], ref, tol),
                                     ("dbias", got[i][1], g0[i][1], ref_db,
                                      tol_db)):
            e1 = t + 2.0 ** -8 * ((start + r).abs() + t)
            e2 = e1 + t + 2.0 ** -8 * ((start + 2 * r).abs() + e1 + t)
            _assert_within(f"accumulated {name} conv{i}", g, start + 2 * r,
                           e2)


# ---- 5. graph capture ------------------------------------------------------

def test_fused_backward_under_graph_capture(ext):
    from distributed_reinforcement_learning_amd.ops import conv_op
    stack, x, dy3, y_ref, refs = _stack_case(4)
    assert conv_op.FUSED_BWD
    params = [stack.conv1.weight, stack.conv1.bias, stack.conv2.weight,
              stack.conv2.bias, stack.conv3.weight, stack.conv3.bias]
    g_out = dy3.reshape(3, -1)

    def step():
        y = conv_op.atari_conv_stack(stack, x)
        return y, torch.autograd.grad(y, params, g_out)

    # eager first, on a side stream: warm-up for the capture and the result
    # the replays answer to
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y_eager, g_eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_cap, g_cap = step()

    def pairs(gs):
        return {i: (_flat(gs[2 * i - 2]), gs[2 * i - 1]) for i in (1, 2, 3)}

    for i in (1, 2, 3):
        _check_pair(f"eager conv{i}", pairs(g_eager)[i], refs[i])
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_cap, y_eager) and torch.equal(y_cap, y_ref)
        for i in (1, 2, 3):
            _check_pair(f"replay {r} conv{i}", pairs(g_cap)[i], refs[i])
