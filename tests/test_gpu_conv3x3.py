"""The 3x3 same-padding MFMA conv family (ops/hip/conv3x3.hip) through the
extension, layer ids 4..8, at N=1 and N=3 (no row count is a multiple of the
128-row tile; at 11x11 with N=3 every row block spans two images).
GPU-only.

References are float64 on the kernel's own bf16 inputs, with the elementwise
bound of tests/test_gpu_conv_wgrad_exact.py:

    |out - ref| <= 2^-8 |ref| + n 2^-23 S

n = number of f32 additions (K + 2 for forward and dgrad, M for wgrad and
the bias gradient), S = the same computation on absolute values, |bias|,
|residual| and |addend| included.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# layer id: (ci, co, hw)
GEOM = {4: (4, 16, 84), 5: (16, 16, 42), 6: (16, 32, 42), 7: (32, 32, 21),
        8: (32, 32, 11)}
LAYERS = sorted(GEOM)
SQUARE = [l for l in LAYERS if GEOM[l][0] == GEOM[l][1]]
CHUNK = 64  # wgrad m-rows per LDS chunk


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available()
    return ops.require_ext()


# ---- float64 references ----------------------------------------------------

def _im2col(x):
    """[N,H,W,C] -> [N*H*W, 9*C] with k = (kh*3 + kw)*C + c, zero padded."""
    n, h, w, c = x.shape
    cols = F.unfold(x.permute(0, 3, 1, 2), kernel_size=3, padding=1)
    return cols.reshape(n, c, 9, h * w).permute(0, 3, 2, 1) \
        .reshape(n * h * w, 9 * c)


def _dgrad_weight(w_flat, ci, co):
    """Wd[ci][tap*CO + co] = W[co][(8 - tap)*CI + ci]."""
    return w_flat.reshape(co, 9, ci).flip(1).permute(2, 1, 0) \
        .reshape(ci, 9 * co)


def _ref_fwd(x, w, b, relu_in, res):
    """(ref, tol) of conv(relu?(x)) + b (+ res), all [N,H,W,CO] float64."""
    xd = x.double()
    if relu_in:
        xd = xd.clamp(min=0)
    A = _im2col(xd)
    wd, bd = w.double(), b.double()
    ref = A @ wd.t() + bd
    S = A.abs() @ wd.abs().t() + bd.abs()
    if res is not None:
        ref = ref + res.double().reshape(ref.shape)
        S = S + res.double().abs().reshape(ref.shape)
    n_add = A.shape[1] + 2
    shape = x.shape[:3] + (w.shape[0],)
    return ref.reshape(shape), \
        (2.0 ** -8 * ref.abs() + n_add * 2.0 ** -23 * S).reshape(shape)


def _ref_dgrad(dy, w, ci, mask_src, addend):
    co = dy.shape[-1]
    A = _im2col(dy.double())
    wd = _dgrad_weight(w.double(), ci, co)
    ref = A @ wd.t()
    S = A.abs() @ wd.abs().t()
    if mask_src is not None:
        m = (mask_src.double() > 0).double().reshape(ref.shape)
        ref, S = ref * m, S * m
    if addend is not None:
        ref = ref + addend.double().reshape(ref.shape)
        S = S + addend.double().abs().reshape(ref.shape)
    n_add = A.shape[1] + 2
    shape = dy.shape[:3] + (ci,)
    return ref.reshape(shape), \
        (2.0 ** -8 * ref.abs() + n_add * 2.0 ** -23 * S).reshape(shape)


def _ref_wgrad(x, dy, relu_in):
    """(dw [CO][K], tol, dbias [CO], tol)."""
    xd = x.double()
    if relu_in:
        xd = xd.clamp(min=0)
    A = _im2col(xd)
    B = dy.double().reshape(A.shape[0], -1)
    M = A.shape[0]
    ref = (A.t() @ B).t()
    S = (A.abs().t() @ B.abs()).t()
    tol = 2.0 ** -8 * ref.abs() + M * 2.0 ** -23 * S
    ref_db = B.sum(0)
    tol_db = 2.0 ** -8 * ref_db.abs() + M * 2.0 ** -23 * B.abs().sum(0)
    return ref, tol, ref_db, tol_db


def _assert_within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    worst = (err - tol).argmax()
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max err/tol {(err / tol.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err <= tol).all()), (
        f"{name}: {int((err > tol).sum())} of {err.numel()} elements out of "
        f"bound; worst err {err.flatten()[worst].item():.3e} vs tol "
        f"{tol.flatten()[worst].item():.3e} at flat index {int(worst)}")


def _assert_small_ints(name, ref):
    assert bool((ref == ref.round()).all()), f"{name}: non-integer reference"
    assert float(ref.abs().max()) <= 256, \
        f"{name}: |ref| max {float(ref.abs().max())} > 256"


# ---- inputs ----------------------------------------------------------------

def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device="cuda", generator=g) * scale).bfloat16()


def _tern(g, *shape, density=2.0 / 3.0):
    """values in {-1, 0, 1}; `density` = probability of a nonzero."""
    u = torch.rand(*shape, device="cuda", generator=g)
    s = torch.where(torch.rand(*shape, device="cuda", generator=g) < 0.5,
                    -1.0, 1.0)
    return torch.where(u < density, s, torch.zeros_like(s)).bfloat16()


def _shift(x, dh, dw):
    """out[n,h,w,c] = x[n,h+dh,w+dw,c], zero outside the image."""
    n, h, w, c = x.shape
    p = F.pad(x, (0, 0, 1, 1, 1, 1))
    return p[:, 1 + dh:1 + dh + h, 1 + dw:1 + dw + w, :]


# ---- tap identity ----------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("layer", SQUARE)
def test_tap_identity_exact(ext, layer, batch):
    """W[co][tap][ci] = delta(co, ci): forward is the zero-padded shift of
    the input by the tap's offset (of relu(input) under relu_in), dgrad the
    mirrored shift of dY. Bit-exact: one product by 1.0 per output."""
    ci, co, hw = GEOM[layer]
    g = _gen(100 + layer)
    x = _randn(g, batch, hw, hw, ci)
    zero_b = torch.zeros(co, device="cuda", dtype=torch.bfloat16)
    for tap in range(9):
        dh, dw = tap // 3 - 1, tap % 3 - 1
        w = torch.zeros(co, 9, ci, device="cuda", dtype=torch.bfloat16)
        w[:, tap, :] = torch.eye(co, device="cuda", dtype=torch.bfloat16)
        w = w.reshape(co, 9 * ci)
        y, _ = ext.conv_fwd(layer, x, w, zero_b, False)
        assert torch.equal(y, _shift(x, dh, dw)), f"fwd tap {tap}"
        y, _ = ext.conv_fwd(layer, x, w, zero_b, False, relu_in=True)
        assert torch.equal(y, _shift(x.clamp(min=0), dh, dw)), \
            f"fwd relu_in tap {tap}"
        dx = ext.conv_dgrad(layer, x, w)
        assert torch.equal(dx, _shift(x, -dh, -dw)), f"dgrad tap {tap}"


# ---- integer exact ---------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("layer", LAYERS)
def test_integer_inputs_bit_exact(ext, layer, batch):
    """Inputs, dY and weights in {-1,0,1}, small integer bias: every f32
    partial sum is an exact integer in any order (atomics included) and the
    results (asserted <= 256 in magnitude) are exact in bf16, so fwd with all
    option combinations, dgrad with mask and addend, wgrad and dbias must
    equal the float64 reference bit for bit."""
    ci, co, hw = GEOM[layer]
    M = batch * hw * hw
    g = _gen(200 + 10 * layer + batch)
    x = _tern(g, batch, hw, hw, ci)
    w = _tern(g, co, 9 * ci)
    b = torch.randint(-3, 4, (co,), device="cuda", generator=g).bfloat16()
    res = _tern(g, batch, hw, hw, co)
    # a sparse dY keeps the M-long wgrad sums small (about 400 nonzeros per
    # column at most)
    dy = _tern(g, batch, hw, hw, co, density=min(0.6, 400.0 / M))
    for relu_in in (False, True):
        for r in (None, res):
            y, _ = ext.conv_fwd(layer, x, w, b, False, relu_in=relu_in,
                                residual=r)
            ref, _ = _ref_fwd(x, w, b, relu_in, r)
            _assert_small_ints("fwd", ref)
            assert torch.equal(y.double(), ref), (relu_in, r is not None)
        dw, db = ext.conv_wgrad(layer, x, dy, relu_in=relu_in)
        rw, _, rb, _ = _ref_wgrad(x, dy, relu_in)
        _assert_small_ints("dw", rw)
        _assert_small_ints("dbias", rb)
        assert torch.equal(dw.double(), rw), f"dw relu_in={relu_in}"
        assert torch.equal(db.double(), rb), f"dbias relu_in={relu_in}"
    if layer > 4:
        dyd = _tern(g, batch, hw, hw, co)
        addend = _tern(g, batch, hw, hw, ci)
        for m, a in ((None, None), (x, None), (None, addend), (x, addend)):
            dx = ext.conv_dgrad(layer, dyd, w, mask_src=m, addend=a)
            ref, _ = _ref_dgrad(dyd, w, ci, m, a)
            _assert_small_ints("dgrad", ref)
            assert torch.equal(dx.double(), ref), (m is not None,
                                                   a is not None)


# ---- random normal inputs --------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("layer", LAYERS)
def test_random_inputs_within_bound(ext, layer, batch):
    ci, co, hw = GEOM[layer]
    g = _gen(300 + 10 * layer + batch)
    x = _randn(g, batch, hw, hw, ci)
    w = _randn(g, co, 9 * ci, scale=0.1)
    b = _randn(g, co, scale=0.5)
    res = _randn(g, batch, hw, hw, co)
    dy = _randn(g, batch, hw, hw, co)
    addend = _randn(g, batch, hw, hw, ci)
    tag = f"layer {layer} batch {batch}"
    for relu_in in (False, True):
        for r in (None, res):
            y, _ = ext.conv_fwd(layer, x, w, b, False, relu_in=relu_in,
                                residual=r)
            ref, tol = _ref_fwd(x, w, b, relu_in, r)
            _assert_within(f"fwd {tag} relu={relu_in} res={r is not None}",
                           y, ref, tol)
        dw, db = ext.conv_wgrad(layer, x, dy, relu_in=relu_in)
        rw, tw, rb, tb = _ref_wgrad(x, dy, relu_in)
        _assert_within(f"dw {tag} relu={relu_in}", dw, rw, tw)
        _assert_within(f"dbias {tag} relu={relu_in}", db, rb, tb)
    if layer > 4:
        for m, a in ((None, None), (x, addend)):
            dx = ext.conv_dgrad(layer, dy, w, mask_src=m, addend=a)
            ref, tol = _ref_dgrad(dy, w, ci, m, a)
            _assert_within(f"dgrad {tag} mask={m is not None}", dx, ref, tol)


# ---- wgrad paths -----------------------------------------------------------

def _m_per_split(ext, layer, batch):
    hw = GEOM[layer][2]
    split = ext._conv_wgrad_split(layer)
    return (batch * hw * hw + split - 1) // split


def _smallest_batch(ext, layer, min_rows):
    batch = 1
    while _m_per_split(ext, layer, batch) < min_rows:
        batch += 1
    return batch


def _wgrad_check(ext, layer, batch, seed, relu_in=True):
    ci, co, hw = GEOM[layer]
    g = _gen(seed)
    x = _randn(g, batch, hw, hw, ci)
    dy = _randn(g, batch, hw, hw, co)
    dw, db = ext.conv_wgrad(layer, x, dy, relu_in=relu_in)
    rw, tw, rb, tb = _ref_wgrad(x, dy, relu_in)
    tag = f"layer {layer} batch {batch} seed {seed}"
    _assert_within(f"dw {tag}", dw, rw, tw)
    _assert_within(f"dbias {tag}", db, rb, tb)


@pytest.mark.parametrize("layer", LAYERS)
def test_wgrad_batch_one_short_slices(ext, layer):
    """Batch 1: every block's M-slice is a fraction of one 64-row chunk (one
    row where the split exceeds M, with the blocks past M empty)."""
    assert _m_per_split(ext, layer, 1) < CHUNK
    _wgrad_check(ext, layer, 1, seed=400 + layer)


@pytest.mark.parametrize("layer", LAYERS)
def test_wgrad_two_chunks_ragged_second(ext, layer):
    batch = _smallest_batch(ext, layer, CHUNK + 2)
    assert CHUNK < _m_per_split(ext, layer, batch) < 2 * CHUNK
    _wgrad_check(ext, layer, batch, seed=410 + layer)


@pytest.mark.parametrize("layer", LAYERS)
def test_wgrad_three_chunks(ext, layer):
    batch = _smallest_batch(ext, layer, 2 * CHUNK + 1)
    assert 2 * CHUNK < _m_per_split(ext, layer, batch) <= 3 * CHUNK
    _wgrad_check(ext, layer, batch, seed=420 + layer)


def test_wgrad_scratch_rezeroed_across_calls_and_layers(ext):
    """All five layers share one scratch: two calls in a row on one layer
    with different inputs, then the layers interleaved (largest scratch
    footprint first), each against its own reference."""
    _wgrad_check(ext, 8, 3, seed=430)
    _wgrad_check(ext, 8, 2, seed=431)
    for i, layer in enumerate((7, 4, 6, 8, 5, 7)):
        _wgrad_check(ext, layer, 1 + (i & 1), seed=440 + i,
                     relu_in=bool(i & 1))


def test_wgrad_under_graph_capture(ext):
    """One captured conv_wgrad, replayed with rewritten inputs: within the
    bound of its own reference, and equal in that bound to the eager call."""
    layer, batch = 7, 3
    ci, co, hw = GEOM[layer]
    g = _gen(450)
    x = _randn(g, batch, hw, hw, ci)
    dy = _randn(g, batch, hw, hw, co)
    ext.conv_wgrad(layer, x, dy, relu_in=True)  # scratch allocated eagerly
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dw, db = ext.conv_wgrad(layer, x, dy, relu_in=True)
    for r in range(2):
        x.copy_(_randn(g, batch, hw, hw, ci))
        dy.copy_(_randn(g, batch, hw, hw, co))
        graph.replay()
        torch.cuda.synchronize()
        rw, tw, rb, tb = _ref_wgrad(x, dy, True)
        _assert_within(f"dw replay {r}", dw, rw, tw)
        _assert_within(f"dbias replay {r}", db, rb, tb)
        edw, edb = ext.conv_wgrad(layer, x, dy, relu_in=True)
        _assert_within(f"eager dw {r}", edw, rw, tw)
        _assert_within(f"eager dbias {r}", edb, rb, tb)


# ---- residual-block Function -----------------------------------------------

@pytest.mark.parametrize("layer", SQUARE)
def test_residual_block_function(ext, layer):
    """out = x + c2(relu(c1(relu(x)))) and its five gradients against the
    torch composite (F.conv2d + autograd) in float64.

    Composition of the bounds: the block is four roundings deep (y1, out,
    dy1, dx are each rounded once to bf16), so it is checked as a chain. Each
    stage's torch reference is evaluated on the bf16 tensors that stage of
    the custom path actually reads, and held to that stage's own bound:

      out            vs  x + conv(relu(y1), w2) + b2        n = K + 2
      dw2, db2       vs  autograd of that w.r.t. w2, b2      n = M
      dy1            vs  autograd of that w.r.t. y1          n = K + 2
      dw1, db1       vs  autograd of conv(relu(x), w1) + b1
                         w.r.t. w1, b1 with output grad dy1  n = M
      dx             vs  the same w.r.t. x, plus dout        n = K + 2

    y1 and dy1 are recomputed with the same kernels the Function calls (the
    kernels are deterministic except for the wgrad atomics, which these two
    do not use), and y1 itself is held to conv(relu(x), w1) + b1. S comes
    from the im2col references above, whose values are first checked against
    the autograd ones to 1e-9."""
    from distributed_reinforcement_learning_amd.ops.resnet_op import (
        _ResBlock3x3,
    )
    ci, co, hw = GEOM[layer]
    batch = 3
    g = _gen(500 + layer)
    x = _randn(g, batch, hw, hw, ci)
    w1 = _randn(g, co, 9 * ci, scale=0.1)
    w2 = _randn(g, co, 9 * ci, scale=0.1)
    b1 = _randn(g, co, scale=0.5)
    b2 = _randn(g, co, scale=0.5)
    dout = _randn(g, batch, hw, hw, co)

    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    out = _ResBlock3x3.apply(*leaves, layer)
    out.backward(dout)
    dx, dw1, db1, dw2, db2 = (t.grad for t in leaves)

    y1, _ = ext.conv_fwd(layer, x, w1, b1, False, relu_in=True)
    dy1 = ext.conv_dgrad(layer, dout, w2, mask_src=y1)
    torch.cuda.synchronize()

    def w4(wf):  # flat [CO][9*CI] -> torch's [CO][CI][3][3], float64 on CPU
        return wf.double().cpu().reshape(co, 3, 3, ci).permute(0, 3, 1, 2) \
            .contiguous().requires_grad_(True)

    def flat(g4):
        return g4.permute(0, 2, 3, 1).reshape(co, 9 * ci).cuda()

    def nchw(t):
        return t.double().cpu().permute(0, 3, 1, 2).contiguous()

    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous().cuda()

    def close(a, b):
        assert float((a - b).abs().max()) <= 1e-9 * (1 + float(b.abs().max()))

    # stage 1 forward
    ref, tol = _ref_fwd(x, w1, b1, True, None)
    _assert_within("y1", y1, ref, tol)
    # stage 2: out, dw2, db2, dy1
    y1d = nchw(y1).requires_grad_(True)
    w2d, b2d = w4(w2), b2.double().cpu().requires_grad_(True)
    o = nchw(x) + F.conv2d(F.relu(y1d), w2d, b2d, padding=1)
    o.backward(nchw(dout))
    ref, tol = _ref_fwd(y1, w2, b2, True, x)
    close(ref, nhwc(o.detach()))
    _assert_within("out", out.detach(), nhwc(o.detach()), tol)
    rw, tw, rb, tb = _ref_wgrad(y1, dout, True)
    close(rw, flat(w2d.grad))
    close(rb, b2d.grad.cuda())
    _assert_within("dw2", dw2, flat(w2d.grad), tw)
    _assert_within("db2", db2, b2d.grad.cuda(), tb)
    ref, tol = _ref_dgrad(dout, w2, ci, y1, None)
    close(ref, nhwc(y1d.grad))
    _assert_within("dy1", dy1, nhwc(y1d.grad), tol)
    # stage 1 backward: dw1, db1, dx
    xd = nchw(x).requires_grad_(True)
    w1d, b1d = w4(w1), b1.double().cpu().requires_grad_(True)
    F.conv2d(F.relu(xd), w1d, b1d, padding=1).backward(nchw(dy1))
    rw, tw, rb, tb = _ref_wgrad(x, dy1, True)
    close(rw, flat(w1d.grad))
    close(rb, b1d.grad.cuda())
    _assert_within("dw1", dw1, flat(w1d.grad), tw)
    _assert_within("db1", db1, b1d.grad.cuda(), tb)
    ref, tol = _ref_dgrad(dy1, w1, ci, x, dout)
    ref_dx = nhwc(xd.grad) + dout.double()
    close(ref, ref_dx)
    _assert_within("dx", dx, ref_dx, tol)
