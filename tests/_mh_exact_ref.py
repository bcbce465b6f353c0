"""Exact references for the four kernels built on the heads/embed dense pass
(ops/hip/mlp_heads.hip): drla_mlp_heads_fwd/_bwd, drla_embed_mlp_fwd/_bwd.

The tolerance tests of those kernels allow several percent of mean error, so
a wrong fragment index in the weight loads can hide in them. Here every
product and every sum is exact in bf16 and f32, so the result does not
depend on summation order and the kernels must match bit for bit:

* each 256x256 weight is a sum of four signed permutation matrices with
  disjoint supports (entries in {-1, 0, 1}, four nonzeros per row and per
  column), so a dot product has four nonzero terms;
* W3p [A,256] has four nonzeros per row and at most one per column, W3v
  [1,256] four nonzeros; biases are in {-1, 0, 1};
* h, dlogits, dvalue, the embedding table and dy are integers in [-3, 3].

Worst case forward: |a1| <= 4*3+1 = 13, |a2| <= 4*13+1 = 53, |logit| <=
4*53+1 = 213; backward: |dz2| <= 3, |dz1| <= 12, |dh| <= 2*48. Integers up
to 256 are exact in bf16 (8 significant bits). The references below are
float64 numpy and ASSERT those facts on what they compute: every
intermediate an integer of magnitude <= 256, every bias-grad / table-grad
sum below 2^24 (exact in f32 in any order).
"""

import numpy as np

HID = 256


def _check_int(x, bound=256):
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x, np.rint(x)), "non-integer intermediate"
    assert np.abs(x).max(initial=0.0) <= bound, (
        f"|intermediate| {np.abs(x).max()} > {bound}")
    return x


def _check_sum(x):
    return _check_int(x, bound=2 ** 24 - 1)


def signed_perm_sum(rng, n=HID, terms=4):
    """[n,n] sum of `terms` signed permutation matrices with disjoint
    supports: row i has its nonzeros in columns (p[i] + s_k) mod n."""
    p = rng.permutation(n)
    shifts = rng.choice(n, size=terms, replace=False)
    w = np.zeros((n, n), dtype=np.float64)
    for s in shifts:
        w[np.arange(n), (p + s) % n] = rng.choice([-1.0, 1.0], size=n)
    assert (np.count_nonzero(w, axis=0) == terms).all()
    assert (np.count_nonzero(w, axis=1) == terms).all()
    return w


def sparse_rows(rng, rows, n=HID, per_row=4):
    """[rows,n], `per_row` nonzeros (+-1) per row, at most one per column."""
    cols = rng.permutation(n)[:rows * per_row].reshape(rows, per_row)
    w = np.zeros((rows, n), dtype=np.float64)
    for r in range(rows):
        w[r, cols[r]] = rng.choice([-1.0, 1.0], size=per_row)
    return w


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def heads_fixture(N, A, seed):
    rng = np.random.default_rng(seed)
    fx = {
        "W1p": signed_perm_sum(rng), "W2p": signed_perm_sum(rng),
        "W3p": sparse_rows(rng, A),
        "W1v": signed_perm_sum(rng), "W2v": signed_perm_sum(rng),
        "W3v": sparse_rows(rng, 1),
        "b1p": _ints(rng, HID, -1, 1), "b2p": _ints(rng, HID, -1, 1),
        "b3p": _ints(rng, A, -1, 1),
        "b1v": _ints(rng, HID, -1, 1), "b2v": _ints(rng, HID, -1, 1),
        "b3v": _ints(rng, 1, -1, 1),
        "h": _ints(rng, (N, HID)),
        "dlogits": _ints(rng, (N, A)),
        "dvalue": _ints(rng, N),
    }
    return fx


def heads_reference(fx):
    """float64 forward + backward of both heads; dict of expected outputs."""
    relu = lambda x: np.maximum(x, 0.0)
    h = _check_int(fx["h"])
    out = {}
    acts = {}
    for c in ("p", "v"):
        a1 = _check_int(relu(h @ fx["W1" + c].T + fx["b1" + c]))
        a2 = _check_int(relu(a1 @ fx["W2" + c].T + fx["b2" + c]))
        y = _check_int(a2 @ fx["W3" + c].T + fx["b3" + c])
        acts[c] = (a1, a2)
        out["a1" + c], out["a2" + c] = a1, a2
        if c == "p":
            out["logits"] = y
        else:
            out["value"] = y[:, 0]
    out["hb"] = h
    dh = 0.0
    for c in ("p", "v"):
        a1, a2 = acts[c]
        dy = fx["dlogits"] if c == "p" else fx["dvalue"][:, None]
        dz2 = _check_int((dy @ fx["W3" + c]) * (a2 > 0))
        dz1 = _check_int((dz2 @ fx["W2" + c]) * (a1 > 0))
        dh = dh + _check_int(dz1 @ fx["W1" + c])
        out["dz2" + c], out["dz1" + c] = dz2, dz1
        out["db3" + c] = _check_sum(dy.sum(0))
        out["db2" + c] = _check_sum(dz2.sum(0))
        out["db1" + c] = _check_sum(dz1.sum(0))
    out["dh"] = _check_int(dh)
    return out


def embed_fixture(N, A, seed, idx=None):
    rng = np.random.default_rng(seed)
    fx = {
        "table": _ints(rng, (A, HID)),
        "b1": _ints(rng, HID, -1, 1),
        "W2": signed_perm_sum(rng),
        "b2": _ints(rng, HID, -1, 1),
        "dy": _ints(rng, (N, HID)),
        "idx": rng.integers(0, A, size=N),
    }
    if idx is not None:
        fx["idx"] = np.asarray(idx, dtype=np.int64)
    return fx


def embed_reference(fx):
    relu = lambda x: np.maximum(x, 0.0)
    idx = fx["idx"]
    a1 = _check_int(relu(fx["table"][idx] + fx["b1"]))
    y = _check_int(relu(a1 @ fx["W2"].T + fx["b2"]))
    dz2 = _check_int(fx["dy"] * (y > 0))
    da1 = _check_int((dz2 @ fx["W2"]) * (a1 > 0))
    dtable = np.zeros_like(fx["table"])
    np.add.at(dtable, idx, da1)
    return {
        "a1": a1, "out": y, "dz2": dz2, "da1": da1,
        "db2": _check_sum(dz2.sum(0)), "db1": _check_sum(da1.sum(0)),
        "dtable": _check_sum(dtable),
    }


# (N, A) of the GPU tests: 17 = one row tile + 1 row, 37 = two tiles + 5,
# 16 = exactly one tile; A = 6 / 18 leave the layer-3 sixteen-row operand
# partial (6, and 16 + 2)
SHAPES = [(17, 6), (37, 18), (16, 18)]


def seed_for(N, A):
    return 1000 * N + A
