"""Numpy restatement of the standard errors of P (include/nadm.h, nadm_snp_info; neural_admixture_amd/pse.py) from UNPACKED genotypes,
in two dtypes, and the simulation that measures their calibration.

    pi_ij  = sum_k q_ik p_jk
    m_ij   = 1 if g_ij != 3, else 0
    r = clip(pi, eps, 1 - eps);  u = clip(1 - pi, eps, 1 - eps)            (u from the UNCLIPPED pi)
    w_ij   = m_ij 2 / (r u)                                                (the expected information of pi in one binomial(2, pi) call)
    I_j[a][b] = sum_i w_ij q_ia q_ib   for a <= b < K, a-major             n_j = sum_i m_ij
    SE_jk  = sqrt((I_j^-1)_kk) over the SNP's free components              n_eff_jk = p_jk (1 - p_jk) / SE_jk^2

The inputs are the float32 Q and P the library gets; the bounds of the clip are the float32 numbers the library compares against.
``info`` (float64) is the truth.  ``info32`` is the yardstick for the tolerances: float32 pi with k in order (a multiplication and
an addition per k, each rounded), a float32 product r u and a float32 division, float32 products w q_a and (w q_a) q_b, float32
sums in sample order over slices of at most 4096 samples, the slices added in float64 and doubled there.  ``se`` inverts the free
block of every SNP with ``numpy.linalg.inv``.  The edge-case matrix, the planted panel and the packed rows are hwe_oracle's.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hwe_oracle as HO  # noqa: E402

EPS = 1e-6
BOUND = 1e-4
SLICE = 4096


def n_pairs(K):
    return K * (K + 1) // 2


def pairs(K):
    """The pairs a <= b of 0..K-1, a-major: the column order of the information."""
    return [(a, b) for a in range(K) for b in range(a, K)]


def _bounds(eps):
    return float(np.float32(eps)), float(np.float32(1.0) - np.float32(eps))


def weights(G, P, Q, eps=EPS):
    """Per (sample, SNP) in float64: w = 2 / (r u) where the call is observed, else 0; and m (bool)."""
    G = np.asarray(G)
    e, ome = _bounds(eps)
    pi = np.asarray(Q, dtype=np.float32).astype(np.float64) @ np.asarray(P, dtype=np.float32).astype(np.float64).T
    m = G != 3
    r, u = np.clip(pi, e, ome), np.clip(1.0 - pi, e, ome)
    return np.where(m, 2.0 / (r * u), 0.0), m


def from_weights(wm, Q, rows=None):
    """(info float64 [M, K (K + 1) / 2], n int64 [M]) of the samples ``rows`` (default: all; any order, repeats count) from a
    ``weights`` result and the samples' Q."""
    w, m = wm
    Q64 = np.asarray(Q, dtype=np.float32).astype(np.float64)
    cnt = np.ones(w.shape[0]) if rows is None else np.bincount(np.asarray(rows), minlength=w.shape[0]).astype(np.float64)
    QQ = np.stack([Q64[:, a] * Q64[:, b] for a, b in pairs(Q64.shape[1])], axis=1)           # [N, T]
    return (w * cnt[:, None]).T @ QQ, cnt.astype(np.int64) @ m.astype(np.int64)


def info(G, P, Q, eps=EPS):
    """The truth, float64: (info, n) per SNP over all samples of G."""
    return from_weights(weights(G, P, Q, eps), Q)


def info32(G, P, Q, eps=EPS):
    """The float32 yardstick (module docstring): (info, n) per SNP over the samples of G IN THEIR ORDER."""
    G = np.asarray(G)
    P32, Q32 = np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    e, ome = (np.float32(x) for x in _bounds(eps))
    N, M = G.shape
    K = P32.shape[1]
    out = np.zeros((M, n_pairs(K)))
    n = np.zeros(M, dtype=np.int64)
    one = np.float32(1.0)
    for s in range(0, N, SLICE):
        g, q = G[s:s + SLICE], Q32[s:s + SLICE]
        pi = np.zeros(g.shape, dtype=np.float32)
        for k in range(K):
            pi = pi + q[:, k:k + 1] * P32[None, :, k]
        m = g != 3
        r, u = np.clip(pi, e, ome), np.clip(one - pi, e, ome)
        w = np.where(m, one / (r * u), np.float32(0.0)).astype(np.float32)
        assert pi.dtype == np.float32 and w.dtype == np.float32
        for t, (a, b) in enumerate(pairs(K)):
            term = (w * q[:, a:a + 1]) * q[:, b:b + 1]
            assert term.dtype == np.float32
            out[:, t] += np.cumsum(term, axis=0, dtype=np.float32)[-1].astype(np.float64)     # cumsum: in sample order, every step rounded
        n += m.sum(axis=0)
    return 2.0 * out, n


def full(info_row, K):
    """One SNP's information as the symmetric K x K matrix."""
    A = np.zeros((K, K))
    for t, (a, b) in enumerate(pairs(K)):
        A[a, b] = A[b, a] = info_row[t]
    return A


def se(I, P, n, bound=BOUND):
    """Per SNP, with ``numpy.linalg.inv`` of the free block: (se, n_eff, fixed, unseen, cond).  se and n_eff float64 [M, K], NaN at a
    fixed (p <= bound or p >= 1 - bound) or unseen (I[k][k] == 0) component and at every entry of a SNP with n = 0 or whose free
    block is not positive definite; cond [M] the 2-norm condition number of the free block (inf where there is none to invert)."""
    I, P64, n = np.asarray(I, dtype=np.float64), np.asarray(P).astype(np.float64), np.asarray(n)
    M, K = P64.shape
    diag = I[:, [t for t, (a, b) in enumerate(pairs(K)) if a == b]]
    fixed = (P64 <= bound) | (P64 >= 1.0 - bound)
    unseen = diag == 0
    out = np.full((M, K), np.nan)
    cond = np.full(M, np.inf)
    for j in range(M):
        f = np.flatnonzero(~(fixed[j] | unseen[j]))
        if n[j] == 0 or len(f) == 0:
            continue
        A = full(I[j], K)[np.ix_(f, f)]
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        cond[j] = np.linalg.cond(A)
        v = np.diag(np.linalg.inv(A))
        if (v > 0).all():
            out[j, f] = np.sqrt(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_eff = P64 * (1.0 - P64) / (out * out)
    return out, n_eff, fixed, unseen, cond


# ------------------------------------------------------------------------------------------------ calibration
def em_p(G, P0, Q, iters, eps=EPS):
    """Masked EM for P with Q fixed, float64, ``iters`` steps from P0: the update of nadm_project_p,
    p <- A / (A + B),  A = p sum_i g q / pi,  B = (1 - p) sum_i (2 - g) q / (1 - pi)  over the observed calls."""
    Q64, P = np.asarray(Q, dtype=np.float64), np.asarray(P0, dtype=np.float64).copy()
    m = G != 3
    g1 = np.where(m, G, 0).astype(np.float64)
    g0 = np.where(m, 2 - G.astype(np.int64), 0).astype(np.float64)
    last = np.inf
    for _ in range(iters):
        pi = np.clip(Q64 @ P.T, eps, 1.0 - eps)
        A = P * ((g1 / pi).T @ Q64)
        B = (1.0 - P) * ((g0 / (1.0 - pi)).T @ Q64)
        with np.errstate(invalid="ignore"):
            new = np.where(A + B > 0, A / np.maximum(A + B, 1e-300), P)
        last = float(np.abs(new - P).max())
        P = new
    return P, last


def calibration(N=300, M=600, K=3, panels=40, iters=60, seed=0, missing=0.05):
    """The restated procedure on simulated data: TRUE Q and P by the recipe of ``hwe_oracle.make_planted`` (a_j ~ U(0.05, 0.95),
    P = clip(a_j + N(0, 0.2), 0.02, 0.98), Q ~ Dirichlet(0.3)), then ``panels`` independent draws of the genotypes (g ~ Binomial(2,
    pi), ``missing`` of the calls hidden); per panel P is refitted by masked EM at the true Q, started at the truth, and its SE taken
    from ``info`` at the FITTED P and ``se``.  Interior entries: true p in [0.1, 0.9] and a finite SE in every panel.  ->
    dict(ratio: the median over interior entries of [median SE over panels] / [sd of the fitted p over panels], ratio_5_95,
    coverage: the share of |z| < 1.96 with z = (fitted - true) / SE, z_sd, interior: their number, em_step: the last EM step)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, 0.95, size=M)
    P = np.clip(a[:, None] + rng.normal(0.0, 0.2, size=(M, K)), 0.02, 0.98).astype(np.float32)
    Q = rng.dirichlet(np.full(K, 0.3), size=N).astype(np.float32)
    pi = np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0.0, 1.0)
    # the panels side by side: P given Q is a separate problem per SNP, so that `panels` panels of M SNPs are one of panels x M
    G = rng.binomial(2, np.tile(pi, (1, panels))).astype(np.uint8)
    G[rng.random(G.shape) < missing] = 3
    fit, step = em_p(G, np.tile(P.astype(np.float64), (panels, 1)), Q, iters)
    I, n = info(G, fit, Q)                                   # (info takes the float32 roundings of the fit, as the library would)
    s, _, _, _, _ = se(I, fit.astype(np.float32), n)
    fit, s = fit.reshape(panels, M, K), s.reshape(panels, M, K)
    truth = P.astype(np.float64)
    interior = (truth >= 0.1) & (truth <= 0.9) & np.isfinite(s).all(axis=0)
    spread = fit.std(axis=0, ddof=1)
    ratio = (np.median(s, axis=0) / spread)[interior]
    z = ((fit - truth[None]) / s)[:, interior]
    return dict(ratio=float(np.median(ratio)), ratio_5_95=(float(np.quantile(ratio, 0.05)), float(np.quantile(ratio, 0.95))),
                coverage=float((np.abs(z) < 1.96).mean()), z_sd=float(z.std()), interior=int(interior.sum()), em_step=step)


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(calibration(), f"{time.time() - t0:.1f} s")
