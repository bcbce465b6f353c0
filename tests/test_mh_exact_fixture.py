"""The exact heads/embed fixtures (tests/_mh_exact_ref.py) must satisfy their
own exactness bounds with no GPU in sight: the float64 references assert
that every intermediate is an integer of magnitude <= 256 (exact in bf16)
and every bias-grad / table-grad sum is below 2^24 (exact in f32)."""

import numpy as np
import pytest

import _mh_exact_ref as R


def test_weight_structure():
    rng = np.random.default_rng(0)
    w = R.signed_perm_sum(rng)
    assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
    assert (np.count_nonzero(w, axis=0) == 4).all()
    assert (np.count_nonzero(w, axis=1) == 4).all()
    w3 = R.sparse_rows(rng, 18)
    assert (np.count_nonzero(w3, axis=1) == 4).all()
    assert (np.count_nonzero(w3, axis=0) <= 1).all()


@pytest.mark.parametrize("N,A", R.SHAPES)
def test_heads_reference_is_exact(N, A):
    fx = R.heads_fixture(N, A, R.seed_for(N, A))
    ref = R.heads_reference(fx)  # asserts the bounds itself
    assert ref["logits"].shape == (N, A) and ref["value"].shape == (N,)
    assert ref["dh"].shape == (N, 256)
    # the fixture is not degenerate: both ReLU branches occur, grads flow
    for k in ("a1p", "a2p", "a1v", "a2v"):
        assert (ref[k] > 0).any() and (ref[k] == 0).any()
    assert np.abs(ref["dh"]).max() > 0
    # bf16 represents every non-sum output exactly
    for k in ("logits", "value", "a2p", "dz1p", "dz1v"):
        assert np.abs(ref[k]).max() <= 256


@pytest.mark.parametrize("N,A", R.SHAPES)
def test_embed_reference_is_exact(N, A):
    fx = R.embed_fixture(N, A, R.seed_for(N, A) + 7)
    ref = R.embed_reference(fx)
    assert (ref["out"] > 0).any() and (ref["out"] == 0).any()
    assert np.abs(ref["da1"]).max() > 0
    perm = np.random.default_rng(N).permutation(N)
    fx = R.embed_fixture(N, N, R.seed_for(N, A) + 8, idx=perm)
    ref = R.embed_reference(fx)
    assert np.array_equal(ref["dtable"][perm], ref["da1"])
