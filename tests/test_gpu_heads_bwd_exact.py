"""Bit-exact pins for the heads backward kernels (ops/hip/heads_bwd.hip):
drla_heads_wgrad's six weight gradients, drla_mlp_heads_bwd at shapes around
the wgrad's 64-row chunk edge, dh written with plain stores whatever the
workspace held, and the pair replayed from a captured graph.

Inputs are those of tests/_mh_exact_ref.py: every product and sum is an exact
integer, so no summation order can move a result and the only rounding is the
kernel's final f32 -> bf16 store (nearest-even, as torch rounds the
reference)."""

import numpy as np
import pytest
import torch

import _mh_exact_ref as R

pytestmark = pytest.mark.gpu

# (1, 1): one live row, one chunk, one logit. 63 / 64 / 65: around the 64-row
# chunk edge, A = 32 the maximum. (129, 18): three chunks, so both LDS buffers
# are reused and the last chunk has one row; nine 16-row dgrad tiles.
SHAPES = [(1, 1), (63, 6), (64, 18), (65, 32), (129, 18)]
NAN_SHAPE = (17, 6)
GRAPH_SHAPE = (37, 18)

W_NAMES = ("W1p", "W2p", "W3p", "W1v", "W2v", "W3v")
B_NAMES = ("b1p", "b2p", "b3p", "b1v", "b2v", "b3v")
DB_NAMES = ("db1p", "db2p", "db3p", "db1v", "db2v", "db3v")
DW_NAMES = ("dW1p", "dW2p", "dW3p", "dW1v", "dW2v", "dW3v")


def _bf(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(
        torch.bfloat16).cuda().contiguous()


def _f32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda()


def _eq(got, want, name):
    """got: device tensor (bf16 or f32); want: float64 numpy, compared in
    got's dtype (exact there, or rounded nearest-even like the kernel's own
    f32 -> bf16 conversion)."""
    w = torch.as_tensor(np.asarray(want), dtype=torch.float32).to(
        got.dtype).cuda().reshape(got.shape)
    assert torch.equal(got, w), (
        f"{name}: {(got.float() != w.float()).sum().item()} of "
        f"{got.numel()} elements differ")


def _with_dw(fx, ref):
    """The reference plus the six dW = dz^T . act in float64. Every sum must
    be below 2^24 in magnitude, so f32 holds it exactly in any order; the
    largest possible is N * 3 * 53 (dW3p: |dlogits| <= 3, |a2| <= 53, bounds
    heads_reference asserts), 20 511 at N = 129."""
    ref = dict(ref)
    dv = fx["dvalue"][:, None]
    ref["dW1p"] = ref["dz1p"].T @ ref["hb"]
    ref["dW2p"] = ref["dz2p"].T @ ref["a1p"]
    ref["dW3p"] = fx["dlogits"].T @ ref["a2p"]
    ref["dW1v"] = ref["dz1v"].T @ ref["hb"]
    ref["dW2v"] = ref["dz2v"].T @ ref["a1v"]
    ref["dW3v"] = dv.T @ ref["a2v"]
    for k in DW_NAMES:
        assert np.abs(ref[k]).max(initial=0.0) < 2 ** 24, k
        assert np.array_equal(ref[k], np.rint(ref[k])), k
    return ref


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    return ops.require_ext()


@pytest.fixture(scope="module")
def refs():
    """(N, A, seed offset) -> (fixture, reference), computed once."""
    out = {}
    keys = [(N, A, 0) for N, A in SHAPES + [NAN_SHAPE, GRAPH_SHAPE]]
    keys.append(GRAPH_SHAPE + (1,))
    for N, A, d in keys:
        fx = R.heads_fixture(N, A, R.seed_for(N, A) + d)
        out[(N, A, d)] = (fx, _with_dw(fx, R.heads_reference(fx)))
    return out


def _unpack(packed):
    return [packed.narrow(0, 0, 65536).view(256, 256),
            packed.narrow(0, 65536, 65536).view(256, 256),
            packed.narrow(0, 131072, 8192).view(256, 32),
            packed.narrow(0, 139264, 65536).view(256, 256),
            packed.narrow(0, 204800, 65536).view(256, 256),
            packed.narrow(0, 270336, 256).view(1, 256)]


def _check_bwd(res, ref):
    dz1p, dz2p, dz1v, dz2v, dh = res[:5]
    _eq(dz1p, ref["dz1p"], "dz1p")
    _eq(dz2p, ref["dz2p"], "dz2p")
    _eq(dz1v, ref["dz1v"], "dz1v")
    _eq(dz2v, ref["dz2v"], "dz2v")
    _eq(dh, ref["dh"], "dh")
    for k, v in zip(DB_NAMES, res[5:11]):
        _eq(v, ref[k], k + " (f32 sums)")


@pytest.mark.parametrize("N,A", SHAPES)
def test_wgrad_exact(ext, refs, N, A):
    """Only the wgrad launch runs: its inputs are the reference's."""
    fx, ref = refs[(N, A, 0)]
    # five [N,256] planes end to end, in the forward's [N, 5*256] shape
    stash = torch.cat([_bf(ref[k]) for k in
                       ("a1p", "a2p", "a1v", "a2v", "hb")]).view(N, 5 * 256)
    ws = torch.cat([torch.zeros(N * 256, device="cuda")] +
                   [_f32(ref[k]).reshape(-1) for k in DB_NAMES]).contiguous()
    got = ext.mlp_heads_wgrad(
        _bf(ref["dz1p"]), _bf(ref["dz2p"]), _bf(ref["dz1v"]),
        _bf(ref["dz2v"]), _bf(fx["dlogits"]), _f32(fx["dvalue"]),
        stash, ws, A)
    for k, v in zip(DW_NAMES + DB_NAMES, got):
        _eq(v, ref[k], k)


@pytest.mark.parametrize("N,A", SHAPES)
@pytest.mark.parametrize("fwd_ws", [True, False])
def test_dgrad_chain_exact(ext, refs, N, A, fwd_ws):
    """fwd_ws: the backward takes the workspace the forward zeroed; else it
    makes its own."""
    fx, ref = refs[(N, A, 0)]
    weights = [_bf(fx[k]) for k in W_NAMES]
    biases = [_bf(fx[k]) for k in B_NAMES]
    _, _, stash, ws, packed = ext.mlp_heads_fwd(
        _f32(fx["h"]), weights, biases, A, want_bwd_bufs=True)
    res = ext.mlp_heads_bwd(_bf(fx["dlogits"]), _f32(fx["dvalue"]), stash,
                            _unpack(packed), A, ws=ws if fwd_ws else None)
    _check_bwd(res, ref)


def test_dh_does_not_depend_on_workspace_contents(ext, refs):
    """dh is stored, every element once: NaNs in the dh region of the
    workspace passed in must not survive. Only the bias tail must be zero."""
    N, A = NAN_SHAPE
    fx, ref = refs[(N, A, 0)]
    weights = [_bf(fx[k]) for k in W_NAMES]
    biases = [_bf(fx[k]) for k in B_NAMES]
    _, _, stash, _, packed = ext.mlp_heads_fwd(
        _f32(fx["h"]), weights, biases, A, want_bwd_bufs=True)
    ws = torch.zeros(N * 256 + 4 * 256 + A + 1, device="cuda")
    ws[:N * 256] = float("nan")
    res = ext.mlp_heads_bwd(_bf(fx["dlogits"]), _f32(fx["dvalue"]), stash,
                            _unpack(packed), A, ws=ws)
    assert res[11].data_ptr() == ws.data_ptr()
    _check_bwd(res, ref)


def test_captured_forward_backward_replays(refs):
    """fused_mlp_heads forward + backward in one captured graph, replayed
    with two different fixtures copied into the static tensors: a workspace
    or LDS assumption that only holds on a first call shows here."""
    from distributed_reinforcement_learning_amd.models.blocks import MLPHead
    from distributed_reinforcement_learning_amd.ops.mlp_heads_op import (
        fused_mlp_heads,
    )
    N, A = GRAPH_SHAPE
    ph = MLPHead(256, [256, 256], A, None).cuda().bfloat16()
    vh = MLPHead(256, [256, 256], 1, None).cuda().bfloat16()
    params = {
        "W1p": ph.hidden[0].weight, "b1p": ph.hidden[0].bias,
        "W2p": ph.hidden[1].weight, "b2p": ph.hidden[1].bias,
        "W3p": ph.out.weight, "b3p": ph.out.bias,
        "W1v": vh.hidden[0].weight, "b1v": vh.hidden[0].bias,
        "W2v": vh.hidden[1].weight, "b2v": vh.hidden[1].bias,
        "W3v": vh.out.weight, "b3v": vh.out.bias,
    }
    h = torch.zeros(N, 256, device="cuda", requires_grad=True)
    dlog = torch.zeros(N, A, device="cuda", dtype=torch.bfloat16)
    dval = torch.zeros(N, device="cuda")

    def put(fx):
        with torch.no_grad():
            for k, p in params.items():
                p.copy_(_bf(fx[k]).reshape(p.shape))
            h.copy_(_f32(fx["h"]))
            dlog.copy_(_bf(fx["dlogits"]))
            dval.copy_(_f32(fx["dvalue"]))

    def step():
        logits, value = fused_mlp_heads(h, ph, vh)
        return torch.autograd.grad([logits, value],
                                   [h] + list(params.values()), [dlog, dval])

    put(refs[(N, A, 0)][0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        grads = step()
    for d in (1, 0):
        fx, ref = refs[(N, A, d)]
        put(fx)
        g.replay()
        torch.cuda.synchronize()
        _eq(grads[0], ref["dh"], f"dh (fixture {d})")
        for k, got in zip(params, grads[1:]):
            _eq(got, ref["d" + k], f"d{k} (fixture {d})")
