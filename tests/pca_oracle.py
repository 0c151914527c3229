"""Float64 numpy restatement of the standardised PCA (neural_admixture_amd/pca.py; include/nadm.h, nadm_obs_project /
nadm_obs_project_t) and the data its tests share.  A plain module, imported the way the other ``*_oracle`` modules are.

G is uint8 [N, M] with the codes 0, 1, 2 observed and 3 missing.  f_j = S_j / (2 n_j) over the observed calls, c_j = 2 f_j,
s_j = 1 / sqrt(2 f_j (1 - f_j)), or 0 for a SNP nobody observed, a monomorphic one and one with min(f, 1 - f) < maf;
Z_ij = o_ij (g_ij - c_j) s_j; M_eff = #{s_j > 0}; the GRM is Z Z^T / M_eff."""
import functools

import numpy as np


def standardise(G, maf=0.0):
    """(f, c, s, M_eff) in float64."""
    G = np.asarray(G)
    o = G != 3
    n = o.sum(axis=0).astype(np.float64)
    S = np.where(o, G, 0).sum(axis=0).astype(np.float64)
    f = np.zeros(G.shape[1])
    f[n > 0] = S[n > 0] / (2.0 * n[n > 0])
    use = (n > 0) & (S > 0) & (S < 2.0 * n) & (np.minimum(f, 1.0 - f) >= maf)
    s = np.zeros(G.shape[1])
    s[use] = 1.0 / np.sqrt(2.0 * f[use] * (1.0 - f[use]))
    return f, 2.0 * f, s, int(use.sum())


def Z(G, maf=0.0):
    _, c, s, _ = standardise(G, maf)
    G = np.asarray(G)
    return np.where(G != 3, (G.astype(np.float64) - c) * s, 0.0)


def orient(U):
    """Columns at unit norm, the entry of largest magnitude positive."""
    U = U / np.linalg.norm(U, axis=0, keepdims=True)
    big = U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])]
    return U * np.where(big < 0, -1.0, 1.0)


def grm(G, maf=0.0):
    z = Z(G, maf)
    return z @ z.T / standardise(G, maf)[3]


def grm_eigh(G, maf=0.0):
    """(eigenvalues descending, eigenvectors oriented) of the dense GRM."""
    lam, U = np.linalg.eigh(grm(G, maf))
    return lam[::-1].copy(), orient(U[:, ::-1])


def omega(M, L, seed):
    return np.random.default_rng(seed).standard_normal(size=(M, L), dtype=np.float32).astype(np.float64)


def rsvd(G, pcs=10, oversample=10, iters=10, maf=0.0, seed=42, dtype=np.float64):
    """The randomised subspace iteration of pca.pca with the same Omega: (eigenvalues [pcs], eigenvectors [N, pcs], M_eff, explained).
    ``dtype``: what the two products Z W and Z^T Q are computed in (operands and matmul); everything else is float64 like there."""
    z = Z(G, maf)
    m_eff = standardise(G, maf)[3]
    zd = z.astype(dtype)
    L = pcs + oversample

    def z_times(W):
        return (zd @ W.astype(dtype)).astype(np.float64)

    def zt_times(Q):
        return (zd.T @ Q.astype(dtype)).astype(np.float64)

    def orth(Y):
        return np.linalg.qr(Y, mode="reduced")[0]

    Y = z_times(omega(G.shape[1], L, seed))
    for _ in range(iters):
        Y = z_times(zt_times(orth(Y)))
    Q = orth(Y)
    Bt = zt_times(Q)
    lam, W = np.linalg.eigh(Bt.T @ Bt / m_eff)
    order = np.argsort(lam)[::-1][:pcs]
    values = np.maximum(lam[order], 0.0)
    return values, orient(Q @ W[:, order]), m_eff, values / ((z ** 2).sum() / m_eff)


def pc_errors(values, vectors, values_ref, vectors_ref, k):
    """Per PC 0..k-1 against a reference: (relative eigenvalue error, 1 - |cos|).  For unit vectors 1 - |cos| = min |u -+ v|^2 / 2,
    which is how it is computed: 1 - u.v itself drowns an angle below 1e-8 in the rounding of the dot product."""
    ev = np.abs(values[:k] - values_ref[:k]) / np.abs(values_ref[:k])
    u, v = vectors[:, :k], vectors_ref[:, :k]
    ang = np.minimum(((u - v) ** 2).sum(axis=0), ((u + v) ** 2).sum(axis=0)) / 2.0
    return ev, ang


# ---- data -----------------------------------------------------------------------------------------------------------------------
STRUCTURED = 3               # PCs that separate the planted panel's four populations


@functools.lru_cache(maxsize=None)
def planted_panel(N=200, M=3001, pops=4, fst=0.1, missing=0.05, seed=7):
    """Balding-Nichols panel of ``pops`` equal populations: ancestral frequency U(0.05, 0.95), population frequencies
    Beta(p (1 - F) / F, (1 - p) (1 - F) / F), genotypes Binomial(2, .), ``missing`` of the calls set to 3.  Planted: SNPs 5 and M - 2
    monomorphic (all 0 / all 2 among the observed), SNP 11 observed by nobody.  uint8 [N, M]; cached: leave it unchanged."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=M)
    a = p * (1.0 - fst) / fst
    b = (1.0 - p) * (1.0 - fst) / fst
    fp = rng.beta(a, b, size=(pops, M))
    pop = np.arange(N) * pops // N
    G = rng.binomial(2, fp[pop]).astype(np.uint8)
    G[:, 5] = 0
    G[:, M - 2] = 2
    G[rng.random((N, M)) < missing] = 3
    G[:, 11] = 3
    return G


@functools.lru_cache(maxsize=None)
def product_panel(N=200, M=3001, seed=19):
    """Codes for the product tests: uniform calls with 10 % missing; row 4 all missing (packed_rows.case_rows plants it in every
    list), row 2 a single observed call, SNPs 9 and 1025 observed by nobody.  uint8 [N, M]; cached: leave it unchanged."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(N, M)).astype(np.uint8)
    G[rng.random((N, M)) < 0.10] = 3
    G[4] = 3
    G[2] = 3
    G[2, 77] = 1
    G[:, 9] = 3
    G[:, 1025] = 3
    return G


def project(Gr, W1, W2):
    """Y = (g o) W1 + o W2 in float64 and the sum of magnitudes sum_j |g o||W1| + o |W2| per output."""
    o = (Gr != 3).astype(np.float64)
    a = np.where(Gr != 3, Gr, 0).astype(np.float64)
    W1, W2 = W1.astype(np.float64), W2.astype(np.float64)
    return a @ W1 + o @ W2, a @ np.abs(W1) + o @ np.abs(W2)


def project_t(Gr, Yin):
    """(O1, O2, sum of magnitudes of O1, of O2) in float64."""
    o = (Gr != 3).astype(np.float64)
    a = np.where(Gr != 3, Gr, 0).astype(np.float64)
    Y = Yin.astype(np.float64)
    return a.T @ Y, o.T @ Y, a.T @ np.abs(Y), o.T @ np.abs(Y)
