"""Shared by test_r2d2_nstep.py (CPU) and test_gpu_r2d2_nstep.py (GPU): a
naive float64 loop over the contract of the n-step R2D2 TD tail, the error
bound a float32 evaluation of it must meet, and a float32 numpy
transcription of drla_r2d2_nstep_loss_fwd (ops/hip/r2d2_loss.hip).

The contract, per (b, t < T1 = W-1):

    k = min(n, T1 - t);  disc_u = done_u ? 0 : gamma
    Gam_0 = 1, Gam_{j+1} = Gam_j disc_{t+j}
    G  = sum_{j<k} Gam_j clip(r_{t+j})
    a* = first argmax_a Qm[b,t+k,a];  x = Qt[b,t+k,a*]
    z  = G + Gam_k hinv(x);  td = h(z) - Qm[b,t,clamp(act_t)]
    loss = mean_b w_b mean_t td^2
    prio = |mean_t td|  or  eta max_t|td| + (1-eta) mean_t|td|

The bound (u = 2^-24, float32 unit roundoff; eps = 1e-3; first order in u,
with 1 % added for the O(u^2/eps) terms). Every float32 operation is taken
to round within u relative, sqrt and division within 2u (one ulp), so the
bound holds whether or not they are correctly rounded; a contraction to FMA
only removes roundings. Inputs are float32 values, fed to the reference
unchanged, so they carry no error; abs_one / none clipping is exact.

* hinv(x) = sign(x) (t^2 - 1), t = (R - 1) / (2 eps), R = sqrt(1 + s),
  s = 4 eps a, a = |x| + 1 + eps. a carries two roundings and eps's own
  representation error, <= 3u a. s adds eps's error and a product: <= 5u s.
  1 + s rounds once more: error <= 5u s + u R^2. The square root halves
  the relative error and adds 2u: |dR| <= (5u s + u R^2) / (2R) + 2u R
  <= 5u R, since s < R^2. R - 1 is exact for R <= 2 (Sterbenz) and rounds
  within u (R - 1) beyond. The division by 2 eps is where it cancels:
  the ABSOLUTE error of R, about u, is divided by 2 eps = 1/500:
      |dt| <= (5u R + u (R - 1)) / (2 eps) + 3u t <= 3u R / eps + 3u t
  (3u t: eps's error and the one-ulp division). t^2 - 1 adds two roundings,
  each <= u t^2:
      e_boot = |d hinv| <= 2 t |dt| + 2u t^2 <= 6u t R / eps + 8u t^2.
* Gam_j is a product of j float32 factors: relative error <= j u <= k u.
* G: each term Gam_j r carries Gam's k u and one product rounding, and each
  of the k - 1 additions rounds within u of a partial sum that is at most
  S = sum_j |Gam_j r_{t+j}|:  |dG| <= 2k u S.
* z = G + Gam_k boot: Gam_k's k u, one product, one addition:
      e_z <= (2k + 2) u M + Gam_k e_boot,   M = S + |Gam_k hinv(x)|.
  When a done zeroes Gam_k the bootstrap term is gone altogether.
* h(z) = sign(z)(Q - 1) + eps z, Q = sqrt(|z| + 1). h' = 1/(2Q) + eps
  decreases in |z|, so the error carried in is at most
  h'(max(|z| - e_z, 0)) e_z. Its own roundings: |z| + 1 (u Q^2, halved by
  the root to u Q / 2), the root (2u Q), Q - 1 (u Q), eps z (2u eps |z|)
  and the final sum (u |h| <= u (Q + eps |z|)): <= 5u (Q + eps |z|).
* td = h(z) - sav rounds once: u (|h(z)| + |sav|).

      e_td = 1.01 [ h'(.) e_z + 5u (Q + eps|z|) + u (|h(z)| + |sav|) ]

With N(0, 2^2) Q values this is a few thousand u, dominated by
3u R / eps from the cancellation in hinv (h' ~ 1/(2t) undoes the factor
2t); a bound of a few u on td cannot hold.

Per-sequence sums are LDS tree reductions of depth <= 10 (W <= 1024), so a
sum of T1 terms is within 10u of the sum of their magnitudes; the loss adds
three roundings per block term and B - 1 atomic additions in any order.
Carrying e = e_td as tests/test_gpu_dqn_loss.py::test_mixed_sign_rows does:

  loss:  sum_bt w_b (2|td| e + e^2) / (T1 B)
         + (10 + B + 3) u sum_bt w_b (|td| + e)^2 / (T1 B)
         (one more u for the rounding of td^2 itself)
  |mean td|:  mean_t e + (10 + 2) u mean_t (|td| + e)
  eta mix:    eta max_t e + (1 - eta) mean_t e
              + (10 + 6) u [eta max_t + (1 - eta) mean_t](|td| + e)
              (1 - eta, two products, the division by T1, the final sum)
  grad at the action column, g w (-2 td) / T1 / B, four roundings:
         c e + 5u c (|td| + e),  c = 2 g w / (T1 B);
         a bf16 output adds one bf16 rounding, 2^-8 c (|td| + e).
"""

import numpy as np

U = 2.0 ** -24
EPS = 1e-3
TREE_DEPTH = 10


def h64(x):
    return np.sign(x) * (np.sqrt(np.abs(x) + 1.0) - 1.0) + EPS * x


def hinv64(x):
    t = (np.sqrt(1.0 + 4.0 * EPS * (np.abs(x) + 1.0 + EPS)) - 1.0) \
        / (2.0 * EPS)
    return np.sign(x) * (t * t - 1.0)


def clip64(r, mode):
    if mode == "abs_one":
        return min(1.0, max(-1.0, r))
    if mode == "soft_asymmetric":
        sq = np.tanh(r / 5.0)
        return (0.3 * sq if r < 0.0 else sq) * 5.0
    assert mode == "none"
    return r


def naive(mq, tq, act, r, done, w, gamma, n, eta=None, g=1.0,
          clip="abs_one"):
    """Triple loop in float64. mq/tq [B,W,A], act/r/done [B,W], w [B] are
    numpy arrays holding the values the kernel saw; gamma and eta likewise
    (pass the float32-rounded numbers). Returns td, its bound e, loss,
    prio, dq, the action columns and M."""
    mq = np.asarray(mq, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    B, W, A = mq.shape
    T1 = W - 1
    td = np.zeros((B, T1))
    e = np.zeros((B, T1))
    M = np.zeros((B, T1))
    col = np.clip(np.asarray(act, dtype=np.int64), 0, A - 1)
    for b in range(B):
        for t in range(T1):
            k = min(n, T1 - t)
            G, Gam, S = 0.0, 1.0, 0.0
            for j in range(k):
                c = clip64(r[b, t + j], clip)
                G += Gam * c
                S += abs(Gam * c)
                Gam *= 0.0 if done[b, t + j] else gamma
            astar = int(np.argmax(mq[b, t + k]))     # first occurrence
            x = tq[b, t + k, astar]
            boot = hinv64(x)
            z = G + Gam * boot
            sav = mq[b, t, col[b, t]]
            y = h64(z)
            td[b, t] = y - sav
            # the bound of the module docstring
            R = np.sqrt(1.0 + 4.0 * EPS * (abs(x) + 1.0 + EPS))
            tt = (R - 1.0) / (2.0 * EPS)
            e_boot = 6 * U * tt * R / EPS + 8 * U * tt * tt
            M[b, t] = S + abs(Gam * boot)
            e_z = (2 * k + 2) * U * M[b, t] + Gam * e_boot
            hp = 0.5 / np.sqrt(max(abs(z) - e_z, 0.0) + 1.0) + EPS
            Q = np.sqrt(abs(z) + 1.0)
            e[b, t] = 1.01 * (hp * e_z + 5 * U * (Q + EPS * abs(z))
                              + U * (abs(y) + abs(sav)))
    loss = float((w * (td * td).mean(axis=1)).mean())
    a = np.abs(td)
    if eta is None:
        prio = np.abs(td.mean(axis=1))
    else:
        prio = eta * a.max(axis=1) + (1.0 - eta) * a.mean(axis=1)
    dq = np.zeros((B, W, A))
    bi, ti = np.meshgrid(np.arange(B), np.arange(T1), indexing="ij")
    dq[bi, ti, col[:, :T1]] = g * w[:, None] * (-2.0 * td) / (T1 * B)
    return dict(td=td, e=e, loss=loss, prio=prio, dq=dq, col=col, M=M)


def loss_bound(ref, w):
    td, e = ref["td"], ref["e"]
    B, T1 = td.shape
    w = np.asarray(w, dtype=np.float64)[:, None]
    a = np.abs(td)
    return ((w * (2 * a * e + e * e)).sum()
            + (TREE_DEPTH + B + 3) * U * (w * (a + e) ** 2).sum()) / (T1 * B)


def prio_bound(ref, eta):
    td, e = ref["td"], ref["e"]
    a = np.abs(td) + e
    if eta is None:
        return e.mean(axis=1) + (TREE_DEPTH + 2) * U * a.mean(axis=1)
    return (eta * e.max(axis=1) + (1.0 - eta) * e.mean(axis=1)
            + (TREE_DEPTH + 6) * U
            * (eta * a.max(axis=1) + (1.0 - eta) * a.mean(axis=1)))


def grad_bound(ref, w, g, bf16=False):
    """[B,T1] bound on the action-column gradients."""
    td, e = ref["td"], ref["e"]
    B, T1 = td.shape
    c = 2.0 * g * np.asarray(w, dtype=np.float64)[:, None] / (T1 * B)
    rel = 5 * U + (2.0 ** -8 if bf16 else 0.0)
    return c * e + rel * c * (np.abs(td) + e)


# -- float32 transcription of the kernel ------------------------------------

F = np.float32


def _fma(a, b, c, contract):
    """a*b + c as the kernel's source order gives it (two roundings), or
    contracted to one rounding as the compiler may."""
    if contract:
        return F(np.float64(a) * np.float64(b) + np.float64(c))
    return F(F(a * b) + c)


def _sign32(x):
    return F(int(x > 0) - int(x < 0))


def _h32(x, contract):
    eps = F(1e-3)
    root = F(F(np.sqrt(F(F(abs(x)) + F(1)))) - F(1))
    if contract:
        return _fma(eps, x, F(_sign32(x) * root), True)
    return F(F(_sign32(x) * root) + F(eps * x))


def _hinv32(x, contract):
    eps = F(1e-3)
    a = F(F(F(abs(x)) + F(1)) + eps)
    s1 = _fma(F(F(4) * eps), a, F(1), contract)
    t = F(F(F(np.sqrt(s1)) - F(1)) / F(F(2) * eps))
    if contract:
        return F(_sign32(x) * F(np.float64(t) * np.float64(t) - 1.0))
    return F(_sign32(x) * F(F(t * t) - F(1)))


def _clip32(r, mode):
    if mode == "abs_one":
        return F(min(F(1), max(F(-1), r)))
    assert mode == "none"
    return r


def kernel_f32(mq, tq, act, r, done, w, gamma, n, eta=None,
               clip="abs_one", contract=False):
    """drla_r2d2_nstep_loss_fwd in numpy float32, operation for operation:
    phase 1 per row, phase 2 per position, then the power-of-two tree.
    Returns (loss, td [B,T1], prio [B]) as float64 views of float32."""
    mq = np.asarray(mq, dtype=F)
    tq = np.asarray(tq, dtype=F)
    r = np.asarray(r, dtype=F)
    w = np.asarray(w, dtype=F)
    B, W, A = mq.shape
    T1 = W - 1
    gamma = F(gamma)
    block = 1
    while block < T1:
        block <<= 1
    td = np.zeros((B, T1), dtype=F)
    prio = np.zeros(B, dtype=F)
    loss = F(0)
    for b in range(B):
        s_r = [_clip32(r[b, u], clip) for u in range(W)]
        s_d = [F(0) if done[b, u] else gamma for u in range(W)]
        s_boot = [None] * W
        for u in range(1, W):
            astar, best = 0, mq[b, u, 0]
            for a in range(1, A):
                if mq[b, u, a] > best:
                    best, astar = mq[b, u, a], a
            s_boot[u] = _hinv32(tq[b, u, astar], contract)
        red = np.zeros((4, block), dtype=F)
        for t in range(T1):
            k = min(n, T1 - t)
            g, gam = F(0), F(1)
            j = 0
            while j < k and gam != 0:
                g = _fma(gam, s_r[t + j], g, contract)
                gam = F(gam * s_d[t + j])
                j += 1
            z = _fma(gam, s_boot[t + k], g, contract) if gam != 0 else g
            col = min(max(int(act[b, t]), 0), A - 1)
            v = F(_h32(z, contract) - mq[b, t, col])
            td[b, t] = v
            red[:, t] = (F(v * v), v, F(abs(v)), F(abs(v)))
        s = block // 2
        while s > 0:
            red[:3, :s] = red[:3, :s] + red[:3, s:2 * s]
            red[3, :s] = np.maximum(red[3, :s], red[3, s:2 * s])
            s //= 2
        loss = F(loss + F(F(F(w[b] * red[0, 0]) / F(T1)) / F(B)))
        if eta is None:
            prio[b] = F(abs(F(red[1, 0] / F(T1))))
        else:
            e32 = F(eta)
            prio[b] = F(F(e32 * red[3, 0])
                        + F(F(F(1) - e32) * F(red[2, 0] / F(T1))))
    return float(loss), td.astype(np.float64), prio.astype(np.float64)
