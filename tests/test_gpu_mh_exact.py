"""Bit-exact pins for drla_mlp_heads_fwd/_bwd and drla_embed_mlp_fwd/_bwd on
inputs whose every product and sum is exact in bf16 and f32
(tests/_mh_exact_ref.py), so neither the MFMA accumulation order nor the
atomic arrival order can move a result: any difference is a wrong operand."""

import numpy as np
import pytest
import torch

import _mh_exact_ref as R

pytestmark = pytest.mark.gpu


def _bf(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(
        torch.bfloat16).cuda().contiguous()


def _f32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda()


def _eq(got, want, name):
    """got: device tensor (bf16 or f32); want: float64 numpy, compared in
    got's dtype (the references are exact there, or rounded like the
    kernel's own f32 -> bf16 conversion: nearest-even)."""
    w = torch.as_tensor(np.asarray(want), dtype=torch.float32).to(
        got.dtype).cuda().reshape(got.shape)
    assert torch.equal(got, w), (
        f"{name}: {(got.float() != w.float()).sum().item()} of "
        f"{got.numel()} elements differ")


@pytest.fixture(scope="module")
def ext():
    from distributed_reinforcement_learning_amd import ops
    return ops.require_ext()


@pytest.fixture(scope="module")
def heads_refs():
    out = {}
    for N, A in R.SHAPES:
        fx = R.heads_fixture(N, A, R.seed_for(N, A))
        out[(N, A)] = (fx, R.heads_reference(fx))
    return out


@pytest.mark.parametrize("N,A", R.SHAPES)
@pytest.mark.parametrize("bwd_bufs", [False, True])
def test_heads_exact(ext, heads_refs, N, A, bwd_bufs):
    """bwd_bufs: the backward consumes the W^T pack and the zeroed workspace
    the forward kernel wrote (the captured step's path) instead of the pack
    kernel's and a fill's."""
    fx, ref = heads_refs[(N, A)]
    names = ("W1p", "W2p", "W3p", "W1v", "W2v", "W3v")
    weights = [_bf(fx[k]) for k in names]
    biases = [_bf(fx[k]) for k in ("b1p", "b2p", "b3p", "b1v", "b2v", "b3v")]
    res = ext.mlp_heads_fwd(_f32(fx["h"]), weights, biases, A,
                            want_bwd_bufs=bwd_bufs)
    logits, value, stash = res[:3]
    _eq(logits, ref["logits"], "logits")
    _eq(value, ref["value"], "value")
    planes = stash.view(5, N, 256)
    for i, k in enumerate(("a1p", "a2p", "a1v", "a2v", "hb")):
        _eq(planes[i], ref[k], "stash " + k)

    if bwd_bufs:
        ws, packed = res[3], res[4]
        assert torch.equal(packed, ext.mlp_heads_pack_wt(weights, A))
    else:
        ws, packed = None, ext.mlp_heads_pack_wt(weights, A)
    wT = [packed.narrow(0, 0, 65536).view(256, 256),
          packed.narrow(0, 65536, 65536).view(256, 256),
          packed.narrow(0, 131072, 8192).view(256, 32),
          packed.narrow(0, 139264, 65536).view(256, 256),
          packed.narrow(0, 204800, 65536).view(256, 256),
          packed.narrow(0, 270336, 256).view(1, 256)]
    dlogits = _bf(fx["dlogits"])
    dvalue = _f32(fx["dvalue"])
    (dz1p, dz2p, dz1v, dz2v, dh, db1p, db2p, db3p, db1v, db2v, db3v,
     ws) = ext.mlp_heads_bwd(dlogits, dvalue, stash, wT, A, ws=ws)
    _eq(dz1p, ref["dz1p"], "dz1p")
    _eq(dz2p, ref["dz2p"], "dz2p")
    _eq(dz1v, ref["dz1v"], "dz1v")
    _eq(dz2v, ref["dz2v"], "dz2v")
    _eq(dh, ref["dh"], "dh")
    f32_bias = dict(db1p=db1p, db2p=db2p, db3p=db3p, db1v=db1v, db2v=db2v,
                    db3v=db3v)
    for k, v in f32_bias.items():
        _eq(v, ref[k], k + " (f32 partials)")
    # the bf16 bias grads the step consumes (converted by the wgrad launch)
    wg = ext.mlp_heads_wgrad(dz1p, dz2p, dz1v, dz2v, dlogits, dvalue, stash,
                             ws, A)
    for k, v in zip(("db1p", "db2p", "db3p", "db1v", "db2v", "db3v"),
                    wg[6:]):
        _eq(v, ref[k], k + " (bf16)")


EMB_COL, H_SLAB, PAD = 64, 32, 8


def _embed_run(ext, fx, slab_mode, fuse):
    N = len(fx["idx"])
    A = fx["table"].shape[0]
    idx = torch.as_tensor(fx["idx"], dtype=torch.int64).cuda()
    table, b1, w2, b2 = (_bf(fx[k]) for k in ("table", "b1", "W2", "b2"))
    dy = _bf(fx["dy"])
    if slab_mode:
        Rw = EMB_COL + 256 + H_SLAB + PAD
        slab = torch.zeros(N, Rw, device="cuda", dtype=torch.bfloat16)
        h = torch.zeros(N, H_SLAB, device="cuda")
        out, a1 = ext.embed_mlp_fwd(idx, table, b1, w2, b2, xh_slab=slab,
                                    emb_col=EMB_COL, h=h)
        # dy as the step passes it: a column slice of a wider gradient
        wide = torch.zeros(N, Rw, device="cuda", dtype=torch.bfloat16)
        wide[:, EMB_COL:EMB_COL + 256] = dy
        dy = wide[:, EMB_COL:EMB_COL + 256]
    else:
        out, a1 = ext.embed_mlp_fwd(idx, table, b1, w2, b2)
    dz2, dtable, db1, db2 = ext.embed_mlp_bwd(dy, out, a1, w2, idx, A,
                                              fuse_scatter=fuse)
    return out, a1, dz2, dtable, db1, db2


@pytest.fixture(scope="module")
def embed_refs():
    out = {}
    for N, A in R.SHAPES:
        fx = R.embed_fixture(N, A, R.seed_for(N, A) + 7)
        out[(N, A, "rand")] = (fx, R.embed_reference(fx))
        # one table row per batch row (a permutation): the table grad then
        # IS da1, row for row, which no launcher returns directly
        perm = np.random.default_rng(N).permutation(N)
        fx = R.embed_fixture(N, N, R.seed_for(N, A) + 8, idx=perm)
        out[(N, A, "perm")] = (fx, R.embed_reference(fx))
    return out


@pytest.mark.parametrize("N,A", R.SHAPES)
@pytest.mark.parametrize("slab_mode", [False, True])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("kind", ["rand", "perm"])
def test_embed_exact(ext, embed_refs, N, A, slab_mode, fuse, kind):
    """fuse False: da1 goes to global memory and a separate scatter sums it;
    fuse True: the scatter runs in the dgrad kernel's epilogue."""
    fx, ref = embed_refs[(N, A, kind)]
    out, a1, dz2, dtable, db1, db2 = _embed_run(ext, fx, slab_mode, fuse)
    _eq(out.contiguous(), ref["out"], "out")
    _eq(a1, ref["a1"], "a1stash")
    _eq(dz2, ref["dz2"], "dz2")
    _eq(db1, ref["db1"], "db1")
    _eq(db2, ref["db2"], "db2")
    _eq(dtable, ref["dtable"], "dtable")
    if kind == "perm":
        da1 = np.zeros_like(ref["da1"])
        da1[fx["idx"]] = ref["da1"]
        _eq(dtable, da1, "da1 (through the one-to-one scatter)")
