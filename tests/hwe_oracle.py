"""Numpy restatement of the Hardy-Weinberg score test given ancestry (include/nadm.h, nadm_snp_hwe) from UNPACKED genotypes, in two
dtypes, and the data the tests share: an edge-case matrix and a planted panel.

    pi_ij  = sum_k q_ik p_jk
    m_ij   = 1 if g_ij != 3 and pimin <= pi_ij <= 1 - pimin, else 0
    r = clip(pi, eps, 1 - eps);  u = clip(1 - pi, eps, 1 - eps)            (u from the UNCLIPPED pi)
    t_ij   = r / u if g = 0;  -1 if g = 1;  u / r if g = 2
    U_j = sum_i m t    Hexp_j = sum_i m 2 pi (1 - pi)    n_j = sum_i m    Hobs_j = sum_i m [g == 1]    T_abs_j = sum_i m |t|
    Z = U / sqrt(n)    F = U / n    Fhet = 1 - Hobs / Hexp    p = erfc(|Z| / sqrt 2)

The inputs are the float32 Q and P the library gets; the bounds of the mask and of the clip are the float32 numbers the library
compares against (pimin, 1 - pimin, eps, 1 - eps, each rounded to float32).  ``sums`` (float64) is the truth.  ``sums32`` is the
yardstick for the tolerances: float32 pi with k in order (a multiplication and an addition per k, each rounded), float32 divisions,
float32 sums in sample order over slices of at most 4096 samples, the slices added in float64.  Both assert OF THEIR INPUTS that no
pi lies within 1e-5 of a bound of the mask, so that the mask cannot come out differently in float32 and float64; the one exception
is a pi that IS 0 or 1 exactly (a P row of zeros or ones against a dyadic Q row that sums to 1 is that in float32 as well).
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kinship_oracle as KO  # noqa: E402

EPS = 1e-6
SLICE = 4096
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _bounds(pimin, eps):
    lo, hi = float(np.float32(pimin)), float(np.float32(1.0) - np.float32(pimin))
    e, ome = float(np.float32(eps)), float(np.float32(1.0) - np.float32(eps))
    return lo, hi, e, ome


def _mask(G, pi64, lo, hi):
    near = (np.abs(pi64 - lo) < 1e-5) | (np.abs(pi64 - hi) < 1e-5)
    exact = (pi64 == 0.0) | (pi64 == 1.0)
    assert not (near & ~exact).any(), "a pi within 1e-5 of pimin or 1 - pimin: the mask could flip between float32 and float64"
    return (G != 3) & (pi64 >= lo) & (pi64 <= hi)


def terms(G, P, Q, pimin=0.0, eps=EPS):
    """Per (sample, SNP) in float64: t, h = 2 pi (1 - pi) (both 0 where masked) and m (bool), for genotypes G [N, M] (0, 1, 2; 3 =
    missing), P [M, K], Q [N, K]."""
    G = np.asarray(G)
    lo, hi, e, ome = _bounds(pimin, eps)
    pi = np.asarray(Q, dtype=np.float32).astype(np.float64) @ np.asarray(P, dtype=np.float32).astype(np.float64).T
    m = _mask(G, pi, lo, hi)
    r, u = np.clip(pi, e, ome), np.clip(1.0 - pi, e, ome)
    t = np.where(G == 0, r / u, np.where(G == 2, u / r, -1.0))
    return np.where(m, t, 0.0), np.where(m, 2.0 * pi * (1.0 - pi), 0.0), m


def from_terms(tm, G, rows=None):
    """(U, Hexp, n, Hobs, T_abs) of the samples ``rows`` (default: all; any order, repeats count) from a ``terms`` result."""
    t, h, m = tm
    G = np.asarray(G)
    if rows is None:
        w = np.ones(t.shape[0])
    else:
        w = np.bincount(np.asarray(rows), minlength=t.shape[0]).astype(np.float64)
    wi = w.astype(np.int64)
    return w @ t, w @ h, wi @ m.astype(np.int64), wi @ (m & (G == 1)).astype(np.int64), w @ np.abs(t)


def sums(G, P, Q, pimin=0.0, eps=EPS):
    """The truth, float64: (U, Hexp, n, Hobs, T_abs) per SNP over all samples of G."""
    return from_terms(terms(G, P, Q, pimin, eps), G)


def sums32(G, P, Q, pimin=0.0, eps=EPS):
    """The float32 yardstick (module docstring): (U, Hexp, n, Hobs, T_abs) per SNP over the samples of G IN THEIR ORDER."""
    G = np.asarray(G)
    P32, Q32 = np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    lo, hi, e, ome = _bounds(pimin, eps)
    N, M = G.shape
    U, H, T = np.zeros(M), np.zeros(M), np.zeros(M)
    n, ho = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    one, two = np.float32(1.0), np.float32(2.0)
    for s in range(0, N, SLICE):
        g, q = G[s:s + SLICE], Q32[s:s + SLICE]
        pi = np.zeros(g.shape, dtype=np.float32)
        for k in range(P32.shape[1]):
            pi = pi + q[:, k:k + 1] * P32[None, :, k]
        assert pi.dtype == np.float32
        m = _mask(g, q.astype(np.float64) @ P32.astype(np.float64).T, lo, hi)
        assert np.array_equal(m, (g != 3) & (pi >= np.float32(lo)) & (pi <= np.float32(hi)))
        r = np.clip(pi, np.float32(e), np.float32(ome))
        u = np.clip(one - pi, np.float32(e), np.float32(ome))
        t = np.where(m, np.where(g == 0, r / u, np.where(g == 2, u / r, -one)), np.float32(0.0)).astype(np.float32)
        h = np.where(m, (two * pi) * (one - pi), np.float32(0.0)).astype(np.float32)
        U += np.cumsum(t, axis=0, dtype=np.float32)[-1].astype(np.float64)          # cumsum: in sample order, every step rounded
        H += np.cumsum(h, axis=0, dtype=np.float32)[-1].astype(np.float64)
        T += np.cumsum(np.abs(t), axis=0, dtype=np.float32)[-1].astype(np.float64)
        n += m.sum(axis=0)
        ho += (m & (g == 1)).sum(axis=0)
    return U, H, n, ho, T


def stats(U, Hexp, n, Hobs):
    """(Z, F, Fhet, p) in float64; NaN where n = 0 (Fhet: where Hexp = 0)."""
    U, Hexp = np.asarray(U, dtype=np.float64), np.asarray(Hexp, dtype=np.float64)
    nf = np.asarray(n).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where(nf > 0, U / np.sqrt(nf), np.nan)
        F = np.where(nf > 0, U / nf, np.nan)
        Fhet = np.where(Hexp > 0, 1.0 - np.asarray(Hobs).astype(np.float64) / Hexp, np.nan)
    p = np.where(np.isnan(Z), np.nan, _erfc(np.abs(np.nan_to_num(Z)) / math.sqrt(2.0)))
    return Z, F, Fhet, p


# ------------------------------------------------------------------------------------------------ the edge-case matrix
def make_edge_case(N, M, K, seed=0):
    """``kinship_oracle.make_edge_case`` (dyadic Q whose rows sum to exactly 1, P row 0 exactly 0 and row 1 exactly 1, the one-hot Q
    row 2, sample 4 all missing, sample 5 with 7 calls, two SNPs nobody observes with M - 1 among them, 5 % missing calls, pi away
    from the bounds of pimin 0 and 0.05) with about 2 % of the OBSERVED calls overwritten by a random code, so that impossible
    calls meet the eps clip; three are planted: g = 2 and g = 1 where pi = 0 (samples 0 and 3 at SNP 0), g = 0 where pi = 1 (sample
    1 at SNP 1).  -> G uint8 [N, M], P float32 [M, K], Q float32 [N, K], dead."""
    G, P, Q, dead = KO.make_edge_case(N, M, K, seed=seed)
    rng = np.random.default_rng(77 + 1000 * M + 10 * K + seed)
    hit = (rng.random(G.shape) < 0.02) & (G != 3)
    G[hit] = rng.integers(0, 3, size=int(hit.sum())).astype(np.uint8)
    G[0, 0], G[3, 0], G[1, 1] = 2, 1, 0
    assert (G[4] == 3).all() and (G[5] != 3).sum() == 7 and (G[:, dead] == 3).all()
    return G, P, Q, dead


# ------------------------------------------------------------------------------------------------ the planted panel
PLANT_N, PLANT_M, PLANT_K, PLANT_EVERY = 300, 3000, 3, 30


def make_planted(seed=0):
    """N = 300, M = 3000, K = 3: a_j ~ U(0.05, 0.95), P = clip(a_j + N(0, 0.2), 0.02, 0.98), Q ~ Dirichlet(0.3), g ~ Binomial(2, pi);
    at every 30th SNP 30 % of the heterozygotes are recalled as 0 or 2 at random; then 5 % of the calls are set to missing.
    -> G uint8 [N, M], P float32 [M, K], Q float32 [N, K] (the TRUE ones, rounded), planted bool [M]."""
    rng = np.random.default_rng(seed)
    N, M, K = PLANT_N, PLANT_M, PLANT_K
    a = rng.uniform(0.05, 0.95, size=M)
    P = np.clip(a[:, None] + rng.normal(0.0, 0.2, size=(M, K)), 0.02, 0.98)
    Q = rng.dirichlet(np.full(K, 0.3), size=N)
    G = rng.binomial(2, np.clip(Q @ P.T, 0.0, 1.0)).astype(np.uint8)
    planted = np.zeros(M, dtype=bool)
    planted[::PLANT_EVERY] = True
    sub = G[:, planted]
    drop = (sub == 1) & (rng.random(sub.shape) < 0.3)
    sub[drop] = 2 * rng.integers(0, 2, size=int(drop.sum())).astype(np.uint8)
    G[:, planted] = sub
    G[rng.random(G.shape) < 0.05] = 3
    return G, P.astype(np.float32), Q.astype(np.float32), planted


def sample_frequency(G):
    """The K = 1 fit: P [M, 1] = sum g / (2 n) over the observed calls (0.5 where there are none), Q [N, 1] = 1."""
    G = np.asarray(G)
    obs = G != 3
    n = obs.sum(axis=0)
    s = np.where(obs, G, 0).sum(axis=0)
    P = np.where(n > 0, s / np.maximum(2.0 * n, 1.0), 0.5)
    return P.astype(np.float32)[:, None], np.ones((G.shape[0], 1), dtype=np.float32)
