"""References shared by the prioritized-replay (PER) tests.

Two facts make exact (bit-equal) PER tests possible:

* Priorities ``k/8`` with integer ``k`` in 1..64 keep every leaf, delta and
  partial sum of a segment tree a multiple of 1/8 far below 2^24/8 (at
  capacity 100 000 the root is at most 6.4 M eighths), so every float32 add
  is exact in any order and a float32 tree equals the float64 ``SumTree``.
* The root-to-leaf descent only compares and subtracts, so a float32 numpy
  transcription models ``drla_per_sample`` bit for bit on ANY tree.
"""

import numpy as np


def dyadic_priorities(rng, n):
    """n priorities k/8, k uniform in [1, 64] (float64, exact in float32)."""
    return rng.integers(1, 65, size=n).astype(np.float64) / 8.0


def descent_f32(tree_np, s_np, cap, n_entries):
    """float32 transcription of drla_per_sample (per_tree.hip): at each
    interior node go left when ``rem <= tree[left]``, else subtract (rounded
    to float32) and go right; clamp the leaf into the populated range
    ``cap - 2 + max(n_entries, 1)``. Returns int64 tree indices."""
    tree = np.asarray(tree_np, dtype=np.float32)
    rem = np.array(s_np, dtype=np.float32, copy=True).reshape(-1)
    tree_len = 2 * int(cap) - 1
    assert tree.shape == (tree_len,)
    idx = np.zeros(rem.shape[0], dtype=np.int64)
    while True:
        left = 2 * idx + 1
        interior = left < tree_len
        if not interior.any():
            break
        li = left[interior]
        ls = tree[li]
        r = rem[interior]
        go_left = r <= ls
        rem[interior] = np.where(go_left, r, (r - ls).astype(np.float32))
        idx[interior] = np.where(go_left, li, li + 1)
    last = int(cap) - 2 + max(int(n_entries), 1)
    return np.minimum(idx, last)
