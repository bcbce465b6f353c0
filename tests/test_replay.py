import numpy as np
import pytest

from distributed_reinforcement_learning_amd.replay import (
    LocalBuffer, Memory, SumTree,
)


class NaiveSumTree:
    """O(n) reference for the vectorized SumTree."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.p = np.zeros(capacity)
        self.write = 0

    def add(self, p):
        self.p[self.write] = p
        self.write = (self.write + 1) % self.capacity

    def retrieve(self, s):
        cum = np.cumsum(self.p)
        # mirror tree descent: first leaf whose inclusive prefix >= s
        # (right-branch taken when s > left-subtree sum)
        for i, c in enumerate(cum):
            if s <= c:
                return i
        return len(self.p) - 1


def test_sum_tree_total_and_update():
    t = SumTree(8)
    idxs = [t.add(p, f"d{i}") for i, p in enumerate([1, 2, 3, 4])]
    assert t.total() == 10
    t.update(idxs[0], 5)
    assert t.total() == 14
    # batched update with duplicate index: later wins
    t.update_batch(np.array([idxs[1], idxs[1]]), np.array([7.0, 9.0]))
    assert t.total() == pytest.approx(5 + 9 + 3 + 4)


def test_sum_tree_retrieve_matches_naive():
    rng = np.random.default_rng(0)
    cap = 16
    t = SumTree(cap)
    naive = NaiveSumTree(cap)
    ps = rng.random(cap) + 0.01
    for i, p in enumerate(ps):
        t.add(p, i)
        naive.add(p)
    queries = rng.random(100) * t.total()
    got = t.retrieve_batch(queries) - (cap - 1)
    want = np.array([naive.retrieve(q) for q in queries])
    np.testing.assert_array_equal(got, want)


def test_sum_tree_ring_overwrite():
    t = SumTree(4)
    for i in range(6):
        t.add(1.0, i)
    # capacity 4: entries 2..5 remain
    datas = sorted(d for d in t.data)
    assert datas == [2, 3, 4, 5]
    assert t.n_entries == 4


def test_memory_priority_exponent_and_weights():
    m = Memory(64, seed=0)
    errors = np.array([0.0, 1.0, 10.0])
    for e in errors:
        m.add(e, f"s{e}")
    expected_p = (np.abs(errors) + Memory.e) ** Memory.a
    assert m.tree.total() == pytest.approx(expected_p.sum())
    batch, idxs, w = m.sample(3)
    assert len(batch) == 3 and len(idxs) == 3
    assert w.max() == pytest.approx(1.0)
    assert m.beta == pytest.approx(0.401)


def test_memory_sampling_tracks_priorities():
    """High-priority items must be sampled ~proportionally more."""
    m = Memory(128, seed=1)
    m.add(0.01, "low")
    m.add(100.0, "high")
    counts = {"low": 0, "high": 0}
    for _ in range(300):
        batch, _, _ = m.sample(2)
        for b in batch:
            counts[b] += 1
    assert counts["high"] > counts["low"] * 5


def test_memory_update_changes_distribution():
    m = Memory(8, seed=2)
    m.add(1.0, "a")
    m.add(1.0, "b")
    _, idxs, _ = m.sample(2)
    m.update(idxs[0], 1000.0)
    # (1000 + e)^0.6 ~ 63.1 plus the untouched leaf
    total = m.tree.total()
    assert total == pytest.approx((1000.0 + Memory.e) ** Memory.a
                                  + (1.0 + Memory.e) ** Memory.a)


def test_local_buffer_sample():
    lb = LocalBuffer(10, seed=0)
    for i in range(15):
        lb.append(i, i + 1, 0, 1, 0.5, False)
    assert len(lb) == 10
    s = lb.sample(4)
    assert len(s["state"]) == 4
    # holds only the last 10
    assert all(st >= 5 for st in s["state"])


def test_memory_state_dict_roundtrip():
    m = Memory(16, seed=3)
    for i in range(10):
        m.add(float(i), i)
    sd = m.state_dict()
    m2 = Memory(16)
    m2.load_state_dict(sd)
    assert m2.tree.total() == pytest.approx(m.tree.total())
    assert m2.tree.n_entries == m.tree.n_entries


def test_refresh_master_after_out_of_band_param_rewrite():
    """bf16 model copy + fp32 master: an out-of-band parameter rewrite
    (rank-0 broadcast, restore) must be followed by refresh_master(), or
    the next update runs on the stale master and silently reverts the
    rewrite (the world>1 divergence bug fixed in r2 — setup_all_reduce
    and load_weights now call it)."""
    import torch
    from distributed_reinforcement_learning_amd.ops.optim import FusedRMSProp

    p = torch.nn.Parameter(torch.randn(64).bfloat16())
    opt = FusedRMSProp([p], lr=0.0, clip_norm=None)  # lr=0: pure sync test
    assert opt.mixed
    # simulate a broadcast: overwrite the bf16 copy out-of-band
    with torch.no_grad():
        new = torch.randn(64).bfloat16()
        opt.flat_params[:64].copy_(new)
    opt.refresh_master()
    opt.flat_grads.zero_()
    opt.step(lr=0.0)  # lr 0: step must be a no-op on the params
    assert torch.equal(p.detach(), new), \
        "stale master reverted the out-of-band rewrite"


# -- PER reference self-check, capacity-1 tree, capacity guard ---------------


def _dyadic_tree(cap, fill, seed):
    from _per_ref import dyadic_priorities
    rng = np.random.default_rng(seed)
    t = SumTree(cap)
    t.add_batch(dyadic_priorities(rng, fill), [None] * fill)
    return t


@pytest.mark.parametrize("cap", [2, 3, 5, 13, 100, 1000])
@pytest.mark.parametrize("full", [False, True], ids=["partial", "full"])
def test_descent_f32_matches_sum_tree_on_dyadic_trees(cap, full):
    """The GPU tests' float32 descent reference agrees with the float64
    SumTree on every multiple of 1/16 in [0, total] and past the end, at
    non-power-of-two capacities, partly filled and full."""
    from _per_ref import descent_f32
    fill = cap if full else max(cap // 3, 1)
    t = _dyadic_tree(cap, fill, seed=cap)
    total = t.total()
    assert total == t.tree[cap - 1:].sum()  # dyadic: exact
    assert total * 16 == int(total * 16)
    s = np.arange(0, int(total * 16) + 1, dtype=np.float64) / 16.0
    s = np.concatenate([s, [total + 1 / 16, 1.5 * total]])
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    want = t.retrieve_batch(s)
    got = descent_f32(t.tree.astype(np.float32), s.astype(np.float32), cap,
                      t.n_entries)
    np.testing.assert_array_equal(got, want)
    # and both agree with the O(n) definition: the first leaf, in
    # left-to-right order, whose inclusive prefix sum reaches s, clamped to
    # the last written leaf. Left to right the deepest level comes first:
    # leaves [2^d - 1, 2cap - 2], then the shallower [cap - 1, 2^d - 2].
    deep = (1 << int(np.log2(2 * cap - 1))) - 1
    order = np.concatenate([np.arange(deep, 2 * cap - 1),
                            np.arange(cap - 1, deep)])
    cum = np.cumsum(t.tree[order])
    pos = np.minimum(np.searchsorted(cum, s, side="left"), cap - 1)
    naive = np.minimum(order[pos], cap - 2 + fill)
    np.testing.assert_array_equal(want, naive)


def test_sum_tree_capacity_one():
    t = SumTree(1)
    t.add(3.5, "a")
    assert t.total() == 3.5
    t.update(0, 1.25)
    assert t.total() == 1.25
    assert t.tree.tolist() == [1.25]
    assert int(t.retrieve_batch(np.array([0.5]))[0]) == 0


def test_gpu_memory_refuses_capacity_past_float32_exactness(monkeypatch):
    """n_entries travels as float32: capacities >= 2**24 are refused, and
    refused before anything is allocated."""
    import torch
    from distributed_reinforcement_learning_amd.replay.gpu_memory import (
        GpuMemory,
    )

    def _no_alloc(*a, **k):
        raise AssertionError("allocated before the capacity check")

    monkeypatch.setattr(torch, "zeros", _no_alloc)
    monkeypatch.setattr(torch, "tensor", _no_alloc)
    with pytest.raises(ValueError):
        GpuMemory(2 ** 24, fields={}, device="cpu")
