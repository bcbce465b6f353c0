"""Conv weight gradient against a float64 reference built from the kernel's
own rounded inputs, with a derived (not tuned) elementwise bound. GPU-only.

dW^T[k][co] = sum_m A[m][k] * dY[m][co] with A = im2col(input) and dY the
ReLU-masked output gradient, both bf16. bf16 x bf16 products are exact in
f32, so the only errors are the f32 additions (at most M of them, each
2^-24 relative on partial sums bounded by S = |A|^T |dY|) and one final
bf16 rounding (2^-9):

    |dw - ref| <= 2^-8 |ref| + M 2^-23 S        for EVERY element.

The bias gradient gets the same bound with S = sum_m |dY[m][co]|.

Batches are chosen from the M-split in effect (ext._conv_wgrad_split) so
that each path of the kernel runs: mostly-empty grids (batch 1), three
chunks per block (both LDS buffers and the steady-state iteration, last
chunk nearly empty), exactly two chunks with a ragged second one, the
re-zeroed scratch and bias slots across calls and layers, and graph
replay.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# layer: (ci, co, k, stride, hi, ho, u8) — the four wgrad instantiations
GEOM = {
    0: (4, 32, 8, 4, 84, 20, True),
    1: (1, 32, 8, 4, 84, 20, True),
    2: (32, 64, 4, 2, 20, 9, False),
    3: (64, 64, 3, 1, 9, 7, False),
}
CHUNK = 64  # m-rows per LDS chunk


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    assert ops.available()
    return ops.require_ext()


def _m_per_split(ext, layer, batch):
    ho = GEOM[layer][5]
    split = ext._conv_wgrad_split(layer)
    return (batch * ho * ho + split - 1) // split


def _smallest_batch(ext, layer, min_rows):
    batch = 1
    while _m_per_split(ext, layer, batch) < min_rows:
        batch += 1
    return batch


def _inputs(layer, batch, seed):
    ci, co, k, s, hi, ho, u8 = GEOM[layer]
    g = torch.Generator(device="cuda").manual_seed(seed)
    if u8:
        x = torch.randint(0, 256, (batch, hi, hi, ci), dtype=torch.uint8,
                          device="cuda", generator=g)
    else:
        x = (torch.randn(batch, hi, hi, ci, device="cuda", generator=g)
             * 0.5).bfloat16()
    dy = torch.randn(batch, ho, ho, co, device="cuda",
                     generator=g).bfloat16()
    # the forward output whose sign is the ReLU mask: about half positive
    y = torch.randn(batch, ho, ho, co, device="cuda", generator=g).bfloat16()
    return x, dy, y


def _reference(layer, x, dy, y):
    """float64 (ref_dw [CO][K], tol_dw, ref_db [CO], tol_db)."""
    ci, co, k, s, hi, ho, u8 = GEOM[layer]
    batch = x.shape[0]
    M = batch * ho * ho
    if u8:
        inv255 = (torch.ones((), dtype=torch.float32, device="cuda")
                  / torch.full((), 255.0, dtype=torch.float32, device="cuda"))
        xr = (x.float() * inv255).bfloat16()  # the kernel's exact expression
    else:
        xr = x
    # unfold orders rows (ci, kh, kw); the kernels use k = (kh*KW + kw)*CI + ci
    cols = F.unfold(xr.double().permute(0, 3, 1, 2), kernel_size=k, stride=s)
    A = cols.reshape(batch, ci, k * k, ho * ho).permute(0, 3, 2, 1) \
        .reshape(M, k * k * ci)
    B = torch.where(y.float() > 0, dy, torch.zeros_like(dy)) \
        .double().reshape(M, co)
    ref = (A.t() @ B).t()
    S = (A.abs().t() @ B.abs()).t()
    tol = 2.0 ** -8 * ref.abs() + M * 2.0 ** -23 * S
    ref_db = B.sum(0)
    tol_db = 2.0 ** -8 * ref_db.abs() + M * 2.0 ** -23 * B.abs().sum(0)
    return ref, tol, ref_db, tol_db


def _assert_within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    excess = err - tol
    worst = excess.argmax()
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max err/tol {(err / tol.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err <= tol).all()), (
        f"{name}: {int((err > tol).sum())} of {err.numel()} elements out of "
        f"bound; worst err {err.flatten()[worst].item():.3e} vs tol "
        f"{tol.flatten()[worst].item():.3e} at flat index {int(worst)}")


def _run_and_check(ext, layer, batch, seed):
    x, dy, y = _inputs(layer, batch, seed)
    co = GEOM[layer][1]
    dy_m = ext.relu_mask_bwd(dy, y, co, layer)
    dw, dbias = ext.conv_wgrad(layer, x, dy_m)
    torch.cuda.synchronize()
    ref, tol, ref_db, tol_db = _reference(layer, x, dy, y)
    tag = f"layer {layer} batch {batch} seed {seed}"
    _assert_within(f"dw {tag}", dw, ref, tol)
    _assert_within(f"dbias {tag}", dbias, ref_db, tol_db)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_batch_one_mostly_empty_grid(ext, layer):
    """m_per_split is 1 (2 for l2): most blocks have no rows and add
    nothing; the live ones stage one row and 63 zero rows."""
    if ext._conv_wgrad_split(layer) >= GEOM[layer][5] ** 2:
        assert _m_per_split(ext, layer, 1) == 1
    _run_and_check(ext, layer, 1, seed=10 + layer)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_three_chunks_per_block(ext, layer):
    """Smallest batch with ceil(M/split) >= 129: prologue, one steady-state
    iteration on each ping-pong buffer, and a nearly empty last chunk."""
    batch = _smallest_batch(ext, layer, 2 * CHUNK + 1)
    assert 2 * CHUNK < _m_per_split(ext, layer, batch) <= 3 * CHUNK
    _run_and_check(ext, layer, batch, seed=20 + layer)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_two_chunks_ragged_second(ext, layer):
    """Exactly two chunks per block, the second one with a few rows."""
    batch = _smallest_batch(ext, layer, CHUNK + 2)
    assert CHUNK < _m_per_split(ext, layer, batch) < 2 * CHUNK
    _run_and_check(ext, layer, batch, seed=30 + layer)


def test_rezero_across_calls_and_layers(ext):
    """The scratch and the bias slots must come back to zero after every
    call: two calls in a row on one layer with different inputs, then the
    layers interleaved, each result against its own reference."""
    _run_and_check(ext, 3, 3, seed=40)
    _run_and_check(ext, 3, 2, seed=41)
    for i, layer in enumerate((3, 2, 0, 3)):
        _run_and_check(ext, layer, 2 + (i & 1), seed=50 + i)


def test_under_graph_capture(ext):
    """relu_mask_bwd + conv_wgrad of layer 3 at batch 3 in one captured
    graph (one stream, no forks), replayed three times with the inputs
    rewritten in place: every replay within the bound of its own reference."""
    layer, batch = 3, 3
    co = GEOM[layer][1]
    x, dy, y = _inputs(layer, batch, seed=60)
    # eager call first: the persistent scratch and bias slots are
    # allocated at first use, never inside a capture
    ext.conv_wgrad(layer, x, ext.relu_mask_bwd(dy, y, co, layer))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dy_m = ext.relu_mask_bwd(dy, y, co, layer)
        dw, dbias = ext.conv_wgrad(layer, x, dy_m)
    for r in range(3):
        nx, ndy, ny = _inputs(layer, batch, seed=61 + r)
        x.copy_(nx)
        dy.copy_(ndy)
        y.copy_(ny)
        graph.replay()
        torch.cuda.synchronize()
        ref, tol, ref_db, tol_db = _reference(layer, x, dy, y)
        _assert_within(f"dw replay {r}", dw, ref, tol)
        _assert_within(f"dbias replay {r}", dbias, ref_db, tol_db)
