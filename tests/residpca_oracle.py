"""Float64 numpy restatement of the residual PCA given Q and P (neural_admixture_amd/residpca.py; include/nadm.h, nadm_resid_project /
nadm_resid_project_t), written from the formulas there, and the data its tests share.  A plain module, imported the way the other
``*_oracle`` modules are.

G is uint8 [N, M] with the codes 0, 1, 2 observed and 3 missing.  P and Q are taken as the fp32 numbers the device holds and
everything after that is float64: pi = Q P^T, m = observed and pimin <= pi <= 1 - pimin (both bounds the fp32 numbers the kernels
hold), r = clip(pi, eps, 1 - eps), u = clip(1 - pi, eps, 1 - eps) from the UNCLIPPED pi, a = m (g - 2 pi) / sqrt(2 r u).

The mask is an fp32 comparison on the device and a float64 one here: ``resid`` asserts that no observed call has pi within ``near``
of either bound, so that the decision cannot differ between the two sides (the fp32 pi carries an absolute error below K 2^-24);
``near=None`` (the default of ``dense`` and ``rsvd``) is for float64-only work, where there is no second side."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitcheck_oracle as FO  # noqa: E402
import pca_oracle as PO  # noqa: E402

EPS = 1e-6
PIMIN = 0.01
NEAR = 2.0 ** -10            # the products' panels: no observed call this close to a bound of the mask
NEAR_FIT = 2.0 ** -20        # the fitted panels (frequencies down to 1e-6) where a GPU result is compared: 16 x the fp32 error of pi at K = 3


def _bounds(pimin):
    lo = np.float32(pimin)
    return float(lo), float(np.float32(1.0) - lo)


def resid(G, P, Q, pimin=PIMIN, eps=EPS, near=NEAR):
    """(a float64 [N, M], m bool [N, M]): the standardised residuals and the calls that enter them."""
    G = np.asarray(G)
    P64, Q64 = np.asarray(P, dtype=np.float32).astype(np.float64), np.asarray(Q, dtype=np.float32).astype(np.float64)
    lo, hi = FO._clips(eps)
    plo, phi = _bounds(pimin)
    o = G != 3
    pi = Q64 @ P64.T
    if near is not None:
        close = o & ((np.abs(pi - plo) <= near) | (np.abs(pi - phi) <= near))
        assert not close.any(), f"{int(close.sum())} observed calls have pi within {near:g} of pimin or 1 - pimin: choose other inputs"
    m = o & (pi >= plo) & (pi <= phi)
    r, u = np.clip(pi, lo, hi), np.clip(1.0 - pi, lo, hi)
    g = np.where(o, G, 0).astype(np.float64)
    return np.where(m, (g - 2.0 * pi) / np.sqrt(2.0 * r * u), 0.0), m


def project(G, P, Q, W, pimin=PIMIN, eps=EPS, near=NEAR):
    """(Y, its sum of magnitudes sum_j |a||w|, ss, nobs) of the forward product, float64 / int64."""
    a, m = resid(G, P, Q, pimin, eps, near)
    W = np.asarray(W, dtype=np.float64)
    return a @ W, np.abs(a) @ np.abs(W), (a * a).sum(axis=1), m.sum(axis=1)


def project_t(G, P, Q, Yin, pimin=PIMIN, eps=EPS, near=NEAR):
    """(O, its sum of magnitudes, nobs_snp) of the transposed product."""
    a, m = resid(G, P, Q, pimin, eps, near)
    Y = np.asarray(Yin, dtype=np.float64)
    return a.T @ Y, np.abs(a).T @ np.abs(Y), m.sum(axis=0)


def edge(total, n_eff, m_eff):
    return (total / n_eff) * (1.0 + np.sqrt(n_eff / m_eff)) ** 2


def summary(a, m):
    """(M_eff, N_eff, total, edge) of a residual matrix and its mask."""
    m_eff, n_eff = int((m.sum(axis=0) > 0).sum()), int((m.sum(axis=1) > 0).sum())
    total = float((a * a).sum() / m_eff)
    return m_eff, n_eff, total, float(edge(total, n_eff, m_eff))


def dense(G, P, Q, pimin=PIMIN, eps=EPS, near=None):
    """eigh of A A^T / M_eff: (eigenvalues descending, eigenvectors oriented, M_eff, N_eff, total, edge)."""
    a, m = resid(G, P, Q, pimin, eps, near)
    m_eff, n_eff, total, ed = summary(a, m)
    lam, U = np.linalg.eigh(a @ a.T / m_eff)
    return lam[::-1].copy(), PO.orient(U[:, ::-1]), m_eff, n_eff, total, ed


def rsvd(G, P, Q, pcs=10, oversample=10, iters=10, pimin=PIMIN, seed=42, dtype=np.float64, eps=EPS, near=None):
    """The subspace iteration of residpca.resid_pca with the same Omega: a dict with eigenvalues [pcs], eigenvectors [N, pcs], M_eff,
    N_eff, total, edge and ratio.  ``dtype``: what the two products are computed in (operands and matmul); the rest is float64."""
    a, m = resid(G, P, Q, pimin, eps, near)
    m_eff, n_eff, total, ed = summary(a, m)
    ad = a.astype(dtype)
    L = pcs + oversample

    def orth(Y):
        return np.linalg.qr(Y, mode="reduced")[0]

    def times(W):
        return (ad @ W.astype(dtype)).astype(np.float64)

    def t_times(Qh):
        return (ad.T @ Qh.astype(dtype)).astype(np.float64)

    Y = times(PO.omega(G.shape[1], L, seed))
    for _ in range(iters):
        Y = times(t_times(orth(Y)))
    Qh = orth(Y)
    Bt = t_times(Qh)
    lam, W = np.linalg.eigh(Bt.T @ Bt / m_eff)
    order = np.argsort(lam)[::-1][:pcs]
    values = np.maximum(lam[order], 0.0)
    return dict(eigenvalues=values, eigenvectors=PO.orient(Qh @ W[:, order]), M_eff=m_eff, N_eff=n_eff, total=total, edge=ed,
                ratio=values / ed)


# ---- data -----------------------------------------------------------------------------------------------------------------------
LOW, HIGH = 21, 1001         # the planted SNPs of product_panel: every p_jk = 0.001 / 0.999, masked by pimin = 0.01 (HIGH only where M > 1001)
ALL_MISSING_ROW, ALL_MISSING_SNP = 4, 3


@functools.lru_cache(maxsize=None)
def product_panel(M, K, N=200):
    """fitcheck_oracle.make_panel(N, M, K) -- P uniform in [0.05, 0.95], sample 1 and SNP 3 all missing -- with row 4 all missing too
    (tests/packed_rows.py plants it in every list) and the SNPs LOW and HIGH planted: every p_jk = 0.001 and 0.999, so that pimin =
    0.01 masks every call there.  -> (G uint8 [N, M], P float32 [M, K], Q float32 [N, K]); cached: leave them unchanged."""
    G, P, Q = FO.make_panel(N, M, K, seed=5)
    G, P = G.copy(), P.copy()
    G[ALL_MISSING_ROW] = 3
    P[LOW] = 0.001
    if M > HIGH:
        P[HIGH] = 0.999
    return G, P, Q


def masked_snps(M):
    """The SNPs of product_panel(M, .) no call of which enters: nobody observed them, or pimin masks them."""
    return [j for j in (ALL_MISSING_SNP, LOW, HIGH) if j < M]


@functools.lru_cache(maxsize=None)
def merged(seed=0, N=96, M=6000):
    return FO.panel_merged(seed, N=N, M=M, rounds=100)


@functools.lru_cache(maxsize=None)
def admixed(seed=0, N=96, M=6000):
    return FO.panel_admixed(seed, N=N, M=M, rounds=100)
