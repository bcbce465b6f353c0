"""drla_dqn_loss_fwd/bwd vs a float64 implementation of the formula in the
header of ops/hip/dqn_loss.hip, across a block boundary, with argmax ties,
clamped actions, zero weights and a non-unit upstream gradient. GPU-only.

    a* = first argmax_a Qm(s',a);  y = r + disc * Qt(s',a*)
    td = y - Qm(s,a);  loss = mean_b w_b td_b^2
    dQm(s,a) = g * w * (-2 td) / B at column a, 0 elsewhere

Tolerances (u = 2^-24, float32 unit roundoff; M = |r| + |disc Qt| + |Qm|):

* td: three roundings (product, sum, difference), each at most u times a
  quantity bounded by M  ->  |td - ref| <= 4 u M.
* loss: a float32 sum of B non-negative terms in any order is within
  (B - 1) u of the exact sum, and each term w td^2 / B carries its own
  roundings -> |loss - ref| <= (B + 8) u sum(w td^2) / B. The "+ 8" covers
  three roundings in the term and twice td's RELATIVE error, so it needs
  td accurate relative to itself (<= 3 u): the shape sweep draws rows with
  no cancellation in td (r and disc Qt of one sign, Qm of the other, so
  |td| = M). test_mixed_sign_rows covers cancelling rows with the error
  of td carried through explicitly.
* grads: td's 3 u plus three roundings -> 8 u relative; bf16 output adds
  one bf16 rounding (2^-9 relative) -> 2^-8.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
G = 2.5   # upstream gradient


def _reference(mq, nm, nt, a, r, disc, w, g=G):
    """float64 numpy; every argument already float64 / int64."""
    B, A = mq.shape
    rows = np.arange(B)
    astar = nm.argmax(axis=1)               # first occurrence
    col = np.clip(a, 0, A - 1)              # drla_clamp_idx
    y = r + disc * nt[rows, astar]
    td = y - mq[rows, col]
    wtd2 = w * td * td
    dq = np.zeros((B, A))
    dq[rows, col] = g * w * (-2.0 * td) / B
    m_scale = np.abs(r) + np.abs(disc * nt[rows, astar]) \
        + np.abs(mq[rows, col])
    return dict(td=td, loss=wtd2.mean(), sum_wtd2=wtd2.sum(), dq=dq,
                col=col, M=m_scale)


def _run(mq, nm, nt, a, r, disc, w, bf16=False):
    """Runs fused_dqn_loss fwd + bwd with upstream gradient G. Inputs are
    numpy; returns (loss, td, grad) as float64 numpy, the grad's dtype, and
    the reference fed exactly what the kernel saw."""
    from distributed_reinforcement_learning_amd.ops.dqn_op import (
        fused_dqn_loss,
    )
    f32 = dict(dtype=torch.float32, device=DEV)
    q = torch.as_tensor(mq, **f32)
    if bf16:
        q = q.bfloat16()
    q.requires_grad_(True)
    t = [torch.as_tensor(v, **f32) for v in (nm, nt)]
    act = torch.as_tensor(a, dtype=torch.int64, device=DEV)
    rdw = [torch.as_tensor(v, **f32) for v in (r, disc, w)]
    loss, td = fused_dqn_loss(q, t[0], t[1], act, *rdw)
    (G * loss).backward()
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and td.dtype == torch.float32
    ref = _reference(
        q.detach().double().cpu().numpy(),
        *[v.double().cpu().numpy() for v in t],
        np.asarray(a, dtype=np.int64),
        *[v.double().cpu().numpy() for v in rdw])
    return (float(loss.detach().double()),
            td.detach().double().cpu().numpy(),
            q.grad.double().cpu().numpy(), q.grad.dtype, ref)


def _check(loss, td, grad, ref, B, grad_rtol, td_rel=None):
    assert (np.abs(td - ref["td"]) <= 4 * U * ref["M"]).all()
    if td_rel is not None:
        assert (np.abs(td - ref["td"]) <= td_rel * np.abs(ref["td"])).all()
    assert abs(loss - ref["loss"]) <= (B + 8) * U * ref["sum_wtd2"] / B
    rows = np.arange(B)
    on = grad[rows, ref["col"]]
    want = ref["dq"][rows, ref["col"]]
    assert (np.abs(on - want) <= grad_rtol * np.abs(want)).all()
    off = grad.copy()
    off[rows, ref["col"]] = 0.0
    assert (off == 0.0).all()


def _one_signed_rows(rng, B, A):
    """Random float32 rows with |td| = M: r and Qt share a per-row sign,
    Qm takes the other; next_main is unconstrained."""
    sign = np.where(rng.random(B) < 0.5, -1.0, 1.0)
    mq = -sign[:, None] * (np.abs(rng.standard_normal((B, A))) + 0.05)
    nt = sign[:, None] * np.abs(rng.standard_normal((B, A)))
    nm = rng.standard_normal((B, A))
    r = sign * np.abs(rng.standard_normal(B)).clip(0, 1)
    disc = np.where(rng.random(B) < 0.2, 0.0, 0.99)
    w = rng.random(B) + 0.1
    a = rng.integers(0, A, B)
    f = np.float32
    return (mq.astype(f), nm.astype(f), nt.astype(f), a, r.astype(f),
            disc.astype(f), w.astype(f))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("A", [2, 18])
@pytest.mark.parametrize("B", [1, 255, 257, 600])
def test_shapes_across_a_block_boundary(B, A, bf16):
    """B = 257 is the smallest batch whose loss is summed by atomicAdd
    from two blocks."""
    rng = np.random.default_rng(100 * B + A)
    loss, td, grad, gdtype, ref = _run(*_one_signed_rows(rng, B, A),
                                       bf16=bf16)
    assert gdtype == (torch.bfloat16 if bf16 else torch.float32)
    assert (np.abs(ref["td"]) == ref["M"]).all()    # no cancellation
    _check(loss, td, grad, ref, B, 2.0 ** -8 if bf16 else 8 * U,
           td_rel=4 * U)


def test_mixed_sign_rows():
    """Rows where td cancels: its absolute error (4 u M) is then large
    relative to td, so carry e = 4 u M through loss and gradient instead
    of assuming a relative error: |td'^2 - td^2| <= 2 |td| e + e^2, and
    each of the three roundings in a term, and the sum, act on terms whose
    total is at most sum(w (|td| + e)^2) / B."""
    B, A = 600, 6
    rng = np.random.default_rng(9)
    f = np.float32
    args = (rng.standard_normal((B, A)).astype(f),
            rng.standard_normal((B, A)).astype(f),
            rng.standard_normal((B, A)).astype(f),
            rng.integers(0, A, B),
            rng.standard_normal(B).clip(-1, 1).astype(f),
            np.where(rng.random(B) < 0.2, 0.0, 0.99).astype(f),
            (rng.random(B) + 0.1).astype(f))
    loss, td, grad, _, ref = _run(*args)
    w = args[6].astype(np.float64)
    e = 4 * U * ref["M"]
    assert (np.abs(td - ref["td"]) <= e).all()
    a_td = np.abs(ref["td"])
    bound = (w * (2 * a_td * e + e * e)).sum() / B \
        + (B + 2) * U * (w * (a_td + e) ** 2).sum() / B
    assert abs(loss - ref["loss"]) <= bound
    rows = np.arange(B)
    on = grad[rows, ref["col"]]
    want = ref["dq"][rows, ref["col"]]
    # g w (-2 td') / B: td's absolute error scaled, plus three roundings
    gbound = G * w * 2 * e / B + 4 * U * G * w * 2 * (a_td + e) / B
    assert (np.abs(on - want) <= gbound).all()
    grad[rows, ref["col"]] = 0.0
    assert (grad == 0.0).all()


def test_argmax_ties_take_the_first_column():
    A = 5
    nm = np.array([
        [1.0, 3.0, 3.0, 0.0, -1.0],     # max at 1, 2
        [2.0, 0.0, 2.0, 1.0, 2.0],      # max at 0, 2, 4
        [0.5, 0.5, 0.5, 0.5, 0.5],      # all equal
        [-4.0, -2.0, -3.0, -2.0, -2.0],  # negative max at 1, 3, 4
        [0.0, -0.0, 0.0, -1.0, -2.0],   # +0 == -0 ties
        [0.0, 1.0, 2.0, 3.0, 3.0],      # max at the last two
    ], dtype=np.float32)
    B = nm.shape[0]
    # a different target value at every column: td names the column used
    nt = np.tile(np.array([1.0, 2.0, 4.0, 8.0, 16.0], dtype=np.float32),
                 (B, 1))
    mq = np.zeros((B, A), dtype=np.float32)
    r = np.zeros(B, dtype=np.float32)
    disc = np.ones(B, dtype=np.float32)
    w = np.ones(B, dtype=np.float32)
    a = np.zeros(B, dtype=np.int64)
    loss, td, grad, _, ref = _run(mq, nm, nt, a, r, disc, w)
    assert td.tolist() == [2.0, 1.0, 1.0, 2.0, 1.0, 8.0]
    assert td.tolist() == ref["td"].tolist()
    _check(loss, td, grad, ref, B, 8 * U)


def test_edges_terminal_zero_weight_and_clamped_actions():
    A, B = 6, 300                      # two blocks
    rng = np.random.default_rng(4)
    mq, nm, nt, a, r, disc, w = _one_signed_rows(rng, B, A)
    # all-dyadic payload so every expected value below is exact in float32
    mq = np.round(mq * 8) / 8
    nt = np.round(nt * 8) / 8
    r = np.round(r * 8) / 8
    disc = np.where(np.arange(B) % 3 == 0, 0.0, 0.5).astype(np.float32)
    w = np.where(np.arange(B) % 5 == 0, 0.0, np.round(w * 4) / 4 + 0.25) \
        .astype(np.float32)
    a = a.copy()
    a[0:6] = [-1, A, A + 7, -1, A, A + 7]
    a[290:296] = [-1, A, A + 7, -1, A, A + 7]     # second block too
    loss, td, grad, _, ref = _run(mq.astype(np.float32), nm,
                                  nt.astype(np.float32), a,
                                  r.astype(np.float32), disc, w)
    assert ref["col"][0:6].tolist() == [0, A - 1, A - 1, 0, A - 1, A - 1]
    # td is exact here (eighths times halves), so the clamp column and
    # the terminal rows show up as equality
    np.testing.assert_array_equal(td, ref["td"])
    term = disc == 0.0
    rows = np.arange(B)
    np.testing.assert_array_equal(
        td[term], (r.astype(np.float64) - mq[rows, ref["col"]])[term])
    _check(loss, td, grad, ref, B, 8 * U)
    # zero-weight rows: no gradient at all, no share of the loss
    assert (grad[w == 0.0] == 0.0).all()
    assert (grad[rows, ref["col"]][(w != 0.0) & (td != 0.0)] != 0.0).all()
    keep = w != 0.0
    kept = (w[keep].astype(np.float64) * ref["td"][keep] ** 2).sum() / B
    assert abs(loss - kept) <= (B + 8) * U * kept
