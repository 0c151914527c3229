"""Numpy restatement of the bootstrap for Q (include/nadm.h: nadm_project_q_w and the bootstrap draw; bootstrap.bootstrap_q), from
UNPACKED genotypes:

    weighted Q step: with w_j = how often SNP j was drawn, over the observed calls
        r = clip(q . p, eps, 1 - eps);  a_k = sum_j w_j [ p_jk g / r + (1 - p_jk) (2 - g) / (1 - r) ];  n = sum_j w_j
        ll = sum_j w_j [ g log r + (2 - g) log(1 - r) ];  q' = max(q a / (2 n), qmin), renormalised;  n = 0: q stays, ll = 0
    the draw:  key = row_key(seed, rep);  c_t = ((uint64) mix32(key ^ t) * nb) >> 32 for t = 0 .. nb - 1;  cnt_c = #{t : c_t = c};
               w_j = cnt_{j / block},  nb = ceil(M / block)                      (mix32 and row_key: cv_oracle, uint64 with masks)
    the procedure: the centre = ``rounds`` rounds of block EM from the given (P, Q); replicate r = ``rounds`` rounds of the block EM
               with the weighted Q step and the UNWEIGHTED P step from the centre; se = std of the replicates' Q (n - 1),
               bias = their mean - the centre's Q

``em_step_w(..., dtype=np.float64)`` is the truth of the GPU tests of one step; ``dtype=np.float32`` is the same arithmetic in float32
with the sums taken in 256-SNP chunks and the chunk partials added in float64, as project_oracle.em_step does: the yardstick of the
log-likelihood tolerance.  ``block_em_w`` / ``bootstrap_q`` take the same ``dtype``: in float32 every round's Q and P are rounded to
float32 (what the library stores between launches) and the P step's sums are float32 too.
"""
import numpy as np

import cv_oracle as CO
from project_oracle import CHUNK, EPS, QMIN

PMIN = 1e-6


# ------------------------------------------------------------------------------------------------ the weighted Q step
def em_step_w(Gm, P, Q, w, eps=EPS, qmin=QMIN, dtype=np.float64, loglik=True):
    """Gm uint8 [b, M] codes (3 = missing), P [M, K], Q [b, K], w [M] integer weights -> (Q_out [b, K], ll [b] float64 at the INPUT
    Q, n [b] = sum of w over the observed calls).  ``loglik=False`` skips the logarithms (ll = 0)."""
    T = np.dtype(dtype).type
    Gm = np.asarray(Gm)
    w = np.asarray(w).astype(np.int64)
    b, M = Gm.shape
    K = P.shape[1]
    Pd, Qd = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    step = M if dtype == np.float64 else CHUNK
    a = np.zeros((b, K), dtype=np.float64)
    ll = np.zeros(b, dtype=np.float64)
    n = np.zeros(b, dtype=np.int64)
    for j0 in range(0, M, step):
        g_raw = Gm[:, j0:j0 + step]
        wj = w[j0:j0 + step]
        wf = wj.astype(dtype)[None, :]
        obs = g_raw != 3
        g = np.where(obs, g_raw, 0).astype(dtype)
        p = Pd[j0:j0 + step]
        r = np.clip(Qd @ p.T, T(eps), T(1) - T(eps)).astype(dtype)
        t1 = (wf * np.where(obs, g / r, T(0))).astype(dtype)
        t0 = (wf * np.where(obs, (T(2) - g) / (T(1) - r), T(0))).astype(dtype)
        a += (t1 @ p + t0 @ (T(1) - p)).astype(dtype)
        if loglik:
            term = (g * np.log(r) + (T(2) - g) * np.log(T(1) - r)).astype(dtype)
            ll += (wf * np.where(obs, term, T(0))).sum(axis=1, dtype=dtype)
        n += (obs * wj[None, :]).sum(axis=1)
    out = np.asarray(Q, dtype=np.float64).copy()
    has = n > 0
    q1 = np.maximum(np.asarray(Q, dtype=np.float64)[has] * a[has] / (2.0 * n[has, None]), qmin)
    out[has] = q1 / q1.sum(axis=1, keepdims=True)
    ll[~has] = 0.0
    return out.astype(dtype), ll, n


# ------------------------------------------------------------------------------------------------ the draw
def n_blocks(M, block):
    return -(-int(M) // int(block))


def draws(M, block, seed, rep):
    """The block every draw t = 0 .. nb - 1 of replicate ``rep`` picks: int64 [nb]."""
    nb = n_blocks(M, block)
    key = CO.row_key(seed, rep)
    t = np.arange(nb, dtype=np.uint64)
    return ((CO.mix32(key ^ t) * np.uint64(nb)) >> np.uint64(32)).astype(np.int64)


def block_counts(M, block, seed, rep):
    return np.bincount(draws(M, block, seed, rep), minlength=n_blocks(M, block))


def block_weights(M, block, seed, rep):
    """int64 [M]: w_j = the count of block j // block."""
    return block_counts(M, block, seed, rep)[np.arange(int(M)) // int(block)]


# ------------------------------------------------------------------------------------------------ the weighted block EM and the procedure
def _p_step(g, h, P, Q, eps, pmin, dtype):
    T = np.dtype(dtype).type
    Pd, Qd = P.astype(dtype), Q.astype(dtype)
    rr = Qd @ Pd.T
    r, u = np.clip(rr, T(eps), T(1) - T(eps)), np.clip(T(1) - rr, T(eps), T(1) - T(eps))
    B, C = ((g.astype(dtype) / r).T @ Qd).astype(np.float64), ((h.astype(dtype) / u).T @ Qd).astype(np.float64)
    P64 = Pd.astype(np.float64)
    num = P64 * B
    den = num + (1.0 - P64) * C
    out = P64.copy()
    ok = den > 0.0
    out[ok] = np.clip(num[ok] / den[ok], pmin, 1.0 - pmin)
    return out.astype(dtype)


def block_em_w(G, P, Q, w, rounds, eps=EPS, qmin=QMIN, pmin=PMIN, dtype=np.float64):
    """``rounds`` rounds of (weighted Q step with P fixed, UNWEIGHTED P step with the new Q) -> (P, Q) in ``dtype``.  ``w = None``:
    every weight 1, the block EM of cv_oracle.block_em."""
    G = np.asarray(G)
    w = np.ones(G.shape[1], dtype=np.int64) if w is None else np.asarray(w)
    obs = G != 3
    g = np.where(obs, G, 0).astype(np.float64)
    h = np.where(obs, 2.0 - g, 0.0)
    P, Q = np.asarray(P, dtype=dtype).copy(), np.asarray(Q, dtype=dtype).copy()
    for _ in range(int(rounds)):
        Q = em_step_w(G, P, Q, w, eps, qmin, dtype, loglik=False)[0]
        P = _p_step(g, h, P, Q, eps, pmin, dtype)
    return P, Q


def bootstrap_q(G, P, Q, B, block, rounds, seed, dtype=np.float64):
    """(q_centre, se, bias) of one head, float64 [N, K]: the procedure of the module docstring with every fit run for exactly
    ``rounds`` rounds (tol = 0)."""
    G = np.asarray(G)
    M = G.shape[1]
    Pc, Qc = block_em_w(G, P, Q, None, rounds, dtype=dtype)
    reps = np.stack([block_em_w(G, Pc, Qc, block_weights(M, block, seed, r), rounds, dtype=dtype)[1].astype(np.float64) for r in range(int(B))])
    Qc = Qc.astype(np.float64)
    return Qc, reps.std(axis=0, ddof=1), reps.mean(axis=0) - Qc


# ------------------------------------------------------------------------------------------------ the planted panel of the calibration
def planted_truth(seed=7, N=60, M=1536, K=3):
    """(P [M, K], Q [N, K]) float64: a ~ U(0.05, 0.95), P = clip(a + N(0, 0.2), 0.02, 0.98); Q ~ Dirichlet(0.5) with the first six
    samples near-pure (0.98 of component i % K, the rest shared)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, 0.95, size=M)
    P = np.clip(a[:, None] + rng.normal(0.0, 0.2, size=(M, K)), 0.02, 0.98)
    Q = rng.dirichlet(np.full(K, 0.5), size=N)
    for i in range(6):
        Q[i] = 0.02 / (K - 1)
        Q[i, i % K] = 0.98
    return P, Q


def planted_panel(P, Q, seed, missing=0.05):
    """One panel drawn from the truth: g ~ Binomial(2, Q P^T), ``missing`` of the calls missing."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, np.clip(Q @ P.T, 0.0, 1.0)).astype(np.uint8)
    G[rng.random(G.shape) < missing] = 3
    return G
