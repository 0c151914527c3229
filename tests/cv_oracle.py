"""Numpy restatement of cross-validation over held-out calls (include/nadm.h: the fold of a call, nadm_cv_mask, nadm_cv_deviance;
cv.cv_error), from UNPACKED genotypes (and, for the masked copy, from the packed bytes):

    mix32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16                    (uint32, wrapping)
    row_key(seed, i) = mix32( mix32( (uint32)i ^ (uint32)(seed >> 32) ) + (uint32)seed + 0x9E3779B9 )
    fold(seed, i, j) = ( (uint64) mix32( row_key(seed, i) ^ (uint32)j ) * folds ) >> 32
    pi = sum_k q_ik p_jk;  r = clip(pi, eps, 1 - eps);  u = clip(1 - pi, eps, 1 - eps)                           (u from the UNCLIPPED pi)
    d  = -2 [ g ln r + (2 - g) ln u ] - 4 ln 2 [g == 1]        dev_j = sum d, nheld_j = count over the observed calls of the fold

The fold function is written in uint64 arithmetic with explicit masks (no reliance on wrap-around).  ``deviance`` (float64) is the
truth; ``deviance32`` is the yardstick for the tolerances: float32 pi with k in order (a multiplication and an addition per k, each
rounded), float32 log2, s = (g log2 r + (2 - g) log2 u) + 2 [g == 1] in float32, float32 sums in sample order over slices of at
most 4096 rows, the slices added in float64, dev = 2 ln 2 (0 - sum).  The inputs are the float32 Q and P the library gets; the
bounds of the clip are the float32 numbers the library compares against.  ``block_em`` is the FRAPPE / ADMIXTURE block EM over the
observed calls in float64, with the formulas of nadm_project_q and nadm_project_p.
"""
import math

import numpy as np

EPS = 1e-6
QMIN = 1e-6
PMIN = 1e-6
SLICE = 4096
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the fold of a call
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def row_key(seed, i):
    seed = int(seed)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    i = np.asarray(i, dtype=np.uint64) & _M32
    return mix32((mix32(i ^ hi) + lo + np.uint64(0x9E3779B9)) & _M32)


def folds_of(seed, rows, M, folds):
    """uint8 [len(rows), M]: the fold of SNP j < M of the matrix rows ``rows`` (indices in the whole matrix)."""
    key = row_key(seed, np.asarray(rows))
    j = np.arange(int(M), dtype=np.uint64)
    return ((mix32(key[:, None] ^ j[None, :]) * np.uint64(int(folds))) >> np.uint64(32)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the masked copy
def mask_genotypes(G, F, fold):
    """Unpacked: the observed calls of the fold become 3."""
    out = np.array(G, dtype=np.uint8, copy=True)
    out[(out != 3) & (np.asarray(F) == fold)] = 3
    return out


def mask_packed(xp, M, seed, folds, fold, row0=0):
    """The bytes of nadm_cv_mask from the packed bytes ``xp`` uint8 [rows, ld] (SNP j in byte j / 4, bits 2 (j % 4) ..): every field
    j < M that is not 3 and whose fold is ``fold`` becomes 3; every other bit stays."""
    xp = np.asarray(xp, dtype=np.uint8)
    rows, ld = xp.shape
    codes = np.stack([(xp >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(rows, 4 * ld)
    F = folds_of(seed, row0 + np.arange(rows), M, folds)
    hit = np.zeros(codes.shape, dtype=bool)
    hit[:, :M] = (codes[:, :M] != 3) & (F == fold)
    codes = np.where(hit, 3, codes).astype(np.uint8).reshape(rows, ld, 4)
    return (codes[:, :, 0] | (codes[:, :, 1] << 2) | (codes[:, :, 2] << 4) | (codes[:, :, 3] << 6)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the held-out deviance
def _bounds(eps):
    return float(np.float32(eps)), float(np.float32(1.0) - np.float32(eps))


def terms(G, P, Q, eps=EPS):
    """d float64 [N, M] of every call (0 where the call is missing)."""
    G = np.asarray(G)
    e, ome = _bounds(eps)
    pi = np.asarray(Q, dtype=np.float32).astype(np.float64) @ np.asarray(P, dtype=np.float32).astype(np.float64).T
    r, u = np.clip(pi, e, ome), np.clip(1.0 - pi, e, ome)
    g = np.where(G == 3, 0, G).astype(np.float64)
    d = -2.0 * (g * np.log(r) + (2.0 - g) * np.log(u)) - 4.0 * math.log(2.0) * (G == 1)
    return np.where(G == 3, 0.0, d)


def from_terms(d, G, F, fold, period=None):
    """(dev, nheld, sum |d|) per SNP over the held-out calls.  ``period``: G and d hold ``period`` rows and row i of F belongs to row
    i % period of them (a matrix made of repeats of its first rows)."""
    G, F = np.asarray(G), np.asarray(F)
    if period is None:
        held = ((G != 3) & (F == fold)).astype(np.int64)
    else:
        reps = -(-F.shape[0] // period)
        pad = np.full((reps * period - F.shape[0], F.shape[1]), 255, dtype=np.uint8)
        held = (np.concatenate([F, pad]) == fold).reshape(reps, period, -1).sum(axis=0) * (G != 3)
    return (held * d).sum(axis=0), held.sum(axis=0), (held * np.abs(d)).sum(axis=0)


def deviance(G, P, Q, F, fold, eps=EPS):
    """The truth, float64: (dev, nheld, sum |d|) per SNP."""
    return from_terms(terms(G, P, Q, eps), G, F, fold)


def deviance32(G, P, Q, F, fold, eps=EPS):
    """The float32 yardstick (module docstring): (dev, nheld) per SNP over the rows of G IN THEIR ORDER."""
    G, F = np.asarray(G), np.asarray(F)
    P32, Q32 = np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    e, ome = (np.float32(x) for x in _bounds(eps))
    N, M = G.shape
    S, n = np.zeros(M), np.zeros(M, dtype=np.int64)
    one, two, zero = np.float32(1.0), np.float32(2.0), np.float32(0.0)
    for s0 in range(0, N, SLICE):
        g_raw, q, f = G[s0:s0 + SLICE], Q32[s0:s0 + SLICE], F[s0:s0 + SLICE]
        pi = np.zeros(g_raw.shape, dtype=np.float32)
        for k in range(P32.shape[1]):
            pi = pi + q[:, k:k + 1] * P32[None, :, k]
        assert pi.dtype == np.float32
        held = (g_raw != 3) & (f == fold)
        g = np.where(g_raw == 3, 0, g_raw).astype(np.float32)
        r, u = np.clip(pi, e, ome), np.clip(one - pi, e, ome)
        t = (g * np.log2(r) + (two - g) * np.log2(u)) + np.where(g_raw == 1, two, zero)
        assert t.dtype == np.float32
        t = np.where(held, t, zero)
        S += np.cumsum(t, axis=0, dtype=np.float32)[-1].astype(np.float64)          # cumsum: in sample order, every step rounded
        n += held.sum(axis=0)
    return 2.0 * math.log(2.0) * (0.0 - S), n


# ------------------------------------------------------------------------------------------------ the block EM, float64
def block_em(G, P, Q, rounds, eps=EPS, qmin=QMIN, pmin=PMIN):
    """``rounds`` rounds of (Q step with P fixed, P step with the new Q) over the observed calls of G -> (P, Q), float64:
        r = clip(q . p, eps, 1 - eps)
        Q step: a_k = sum_j [ p_jk g / r + (1 - p_jk) (2 - g) / (1 - r) ];  q' = max(q a / (2 n), qmin), renormalised;  n = 0: q stays
        P step: u = clip(1 - q . p, eps, 1 - eps);  B = sum_i q g / r, C = sum_i q (2 - g) / u;  num = p B, den = num + (1 - p) C;
                p' = clip(num / den, pmin, 1 - pmin) where den > 0, else p stays"""
    G = np.asarray(G)
    obs = G != 3
    g = np.where(obs, G, 0).astype(np.float64)
    h = np.where(obs, 2.0 - g, 0.0)
    n_i = obs.sum(axis=1)
    P, Q = np.asarray(P, dtype=np.float64).copy(), np.asarray(Q, dtype=np.float64).copy()
    for _ in range(int(rounds)):
        r = np.clip(Q @ P.T, eps, 1.0 - eps)
        t1, t0 = g / r, h / (1.0 - r)
        a = t1 @ P + t0 @ (1.0 - P)
        has = n_i > 0
        q1 = np.maximum(Q[has] * a[has] / (2.0 * n_i[has, None]), qmin)
        Q[has] = q1 / q1.sum(axis=1, keepdims=True)
        rr = Q @ P.T
        r, u = np.clip(rr, eps, 1.0 - eps), np.clip(1.0 - rr, eps, 1.0 - eps)
        B, C = (g / r).T @ Q, (h / u).T @ Q
        num = P * B
        den = num + (1.0 - P) * C
        ok = den > 0.0
        P[ok] = np.clip(num[ok] / den[ok], pmin, 1.0 - pmin)
    return P, Q


def cv_error(G, Ps, Qs, folds, rounds, seed, eps=EPS):
    """Per head: (error, per-fold errors, held-out calls) of the float64 procedure: per fold the fold's calls hidden, ``rounds``
    rounds of block EM from (Ps[h], Qs[h]), the deviance of the hidden calls at the refit."""
    G = np.asarray(G)
    F = folds_of(seed, np.arange(G.shape[0]), G.shape[1], folds)
    out = []
    for P, Q in zip(Ps, Qs):
        dev, held = np.zeros(folds), np.zeros(folds, dtype=np.int64)
        for f in range(folds):
            Pf, Qf = block_em(mask_genotypes(G, F, f), P, Q, rounds, eps)
            d, n, _ = deviance(G, Pf.astype(np.float32), Qf.astype(np.float32), F, f, eps)
            dev[f], held[f] = d.sum(), n.sum()
        out.append((float(dev.sum() / held.sum()), dev / held, int(held.sum())))
    return out


# ------------------------------------------------------------------------------------------------ the panel of the end-to-end test
def make_panel(seed=3, N=300, M=3000, K=3):
    """a ~ U(0.05, 0.95), P = clip(a + N(0, 0.2), 0.02, 0.98), Q ~ Dirichlet(0.3), g ~ Binomial(2, Q P^T), 5 % missing."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, 0.95, size=M)
    P = np.clip(a[:, None] + rng.normal(0.0, 0.2, size=(M, K)), 0.02, 0.98)
    Q = rng.dirichlet(np.full(K, 0.3), size=N)
    G = rng.binomial(2, np.clip(Q @ P.T, 0.0, 1.0)).astype(np.uint8)
    G[rng.random(G.shape) < 0.05] = 3
    return G, P.astype(np.float32), Q.astype(np.float32)
