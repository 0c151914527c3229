"""Float64 numpy restatement of the admixture-aware kinship estimator (REAP; include/nadm.h, nadm_kinship) from UNPACKED genotypes,
and the data the tests share: a seed-fixed pedigree and an edge-case matrix.

    pi_ij  = sum_k q_ik p_jk
    m_ij   = 1 if g_ij != 3 and pimin <= pi_ij <= 1 - pimin, else 0
    d_ij   = m_ij (g_ij - 2 pi_ij)        s_ij = m_ij sqrt(max(pi_ij (1 - pi_ij), 0))
    num_ab = sum_j d_aj d_bj    den_ab = sum_j s_aj s_bj    n_ab = sum_j m_aj m_bj    abs_ab = sum_j |d_aj| |d_bj|
    phi_ab = num_ab / (4 den_ab)  (NaN where den_ab = 0)

The inputs are the float32 Q and P the library gets, widened; the two bounds of the mask are the float32 numbers the library compares
against (pimin and 1 - pimin, both rounded to float32).  ``terms`` asserts OF ITS INPUTS that no pi lies within 1e-5 of either bound,
so that the mask cannot come out differently in float32 and float64; the one exception is a pi that IS 0 or 1 exactly (a P row of
zeros or ones against a Q row whose entries are dyadic and sum to 1 is that in float32 as well).
"""
import numpy as np


def terms(G, P, Q, pimin=0.0):
    """Per (sample, SNP): d, s (float64) and m (bool) for genotypes G [N, M] (0, 1, 2; 3 = missing), P [M, K], Q [N, K]."""
    G = np.asarray(G)
    pi = np.asarray(Q, dtype=np.float32).astype(np.float64) @ np.asarray(P, dtype=np.float32).astype(np.float64).T
    lo = float(np.float32(pimin))
    hi = float(np.float32(1.0) - np.float32(pimin))
    near = (np.abs(pi - lo) < 1e-5) | (np.abs(pi - hi) < 1e-5)
    exact = (pi == 0.0) | (pi == 1.0)
    assert not (near & ~exact).any(), "a pi within 1e-5 of pimin or 1 - pimin: the mask could flip between float32 and float64"
    m = (G != 3) & (pi >= lo) & (pi <= hi)
    d = np.where(m, G.astype(np.float64) - 2.0 * pi, 0.0)
    s = np.where(m, np.sqrt(np.maximum(pi * (1.0 - pi), 0.0)), 0.0)
    return d, s, m


def from_terms(tA, tB):
    """(num, den, n, abs) of the samples of tA against the samples of tB (each a ``terms`` result, possibly row-gathered)."""
    dA, sA, mA = tA
    dB, sB, mB = tB
    num = dA @ dB.T
    den = sA @ sB.T
    n = (mA.astype(np.float64) @ mB.astype(np.float64).T).astype(np.int64)
    ab = np.abs(dA) @ np.abs(dB).T
    return num, den, n, ab


def gather(t, idx):
    return tuple(a[idx] for a in t)


def phi_of(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num / (4.0 * den), np.nan)


def kinship(G, P, Q, pimin=0.0):
    """All pairs of the samples of G: (phi, num, den, n, abs), float64 / int64 [N, N]."""
    t = terms(G, P, Q, pimin)
    num, den, n, ab = from_terms(t, t)
    return phi_of(num, den), num, den, n, ab


# ------------------------------------------------------------------------------------------------ the pedigree
PED_M, PED_K, PED_FOUNDERS = 3001, 3, 12
PED_PARENT_CHILD = [(0, 12), (0, 13), (1, 12), (1, 13)]
PED_SIBS = [(12, 13)]
PED_DUPLICATE = [(2, 14)]


def make_pedigree(seed=0, missing=0.05):
    """12 founders, two children (12, 13) of founders 0 and 1, a duplicate (14) of founder 2.  P = clip(a_j + N(0, 0.15), 0.02, 0.98),
    a_j ~ U(0.05, 0.95); a founder's q ~ Dirichlet(0.7) and each of its two haplotypes draws, per SNP, an ancestry from q and then an
    allele from that ancestry's p; a child takes one random haplotype allele from each parent per SNP, its q is the parents' mean.
    -> G uint8 [15, M] with ``missing`` of the calls set to 3 at random, P float32 [M, K], Q float32 [15, K] (the TRUE ones)."""
    rng = np.random.default_rng(seed)
    M, K, F = PED_M, PED_K, PED_FOUNDERS
    a = rng.uniform(0.05, 0.95, size=M)
    P = np.clip(a[:, None] + rng.normal(0.0, 0.15, size=(M, K)), 0.02, 0.98)
    q = rng.dirichlet(np.full(K, 0.7), size=F)
    hap = np.empty((F, 2, M), dtype=np.uint8)
    for f in range(F):
        for h in range(2):
            z = (rng.random(M)[:, None] > np.cumsum(q[f])[None, :-1]).sum(axis=1)          # ancestry of the haplotype at each SNP
            hap[f, h] = rng.random(M) < P[np.arange(M), z]
    rows, qs = [hap[f, 0] + hap[f, 1] for f in range(F)], [q[f] for f in range(F)]
    for _ in range(2):
        pick0, pick1 = rng.integers(0, 2, size=M), rng.integers(0, 2, size=M)
        rows.append(hap[0, pick0, np.arange(M)] + hap[1, pick1, np.arange(M)])
        qs.append(0.5 * (q[0] + q[1]))
    rows.append(rows[2].copy())
    qs.append(q[2])
    G = np.stack(rows).astype(np.uint8)
    G[rng.random(G.shape) < missing] = 3
    return G, P.astype(np.float32), np.stack(qs).astype(np.float32)


def band(phi):
    """Degree band of a kinship coefficient: 0 = duplicate, 1 = first, 2 = second, 3 = third degree, 4 = unrelated."""
    return int(sum(phi < e for e in (2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5, 2.0 ** -4.5)))


# ------------------------------------------------------------------------------------------------ the edge-case matrix
def make_edge_case(N, M, K, pimins=(0.0, 0.05), seed=0, missing=0.05):
    """N >= 8 samples with 5 % missing calls and the planted cases: P row 0 exactly 0 and row 1 exactly 1, Q row 2 one-hot, sample 4
    all missing, sample 5 with 7 calls, the SNPs ``dead`` (two of them, M - 1 among them) that nobody observes.  Q is dyadic
    (multiples of 2^-10, every row sums to exactly 1), so that pi against the P row of ones is exactly 1 in float32 and float64;
    P rows with a pi within 2e-5 of a bound of one of ``pimins`` are drawn again.  -> G uint8 [N, M], P float32 [M, K],
    Q float32 [N, K], dead."""
    rng = np.random.default_rng(1000 * M + 10 * K + seed)
    Q = rng.dirichlet(np.full(K, 0.6), size=N)
    Q = np.floor(Q * 1024.0) / 1024.0
    Q[np.arange(N), Q.argmax(axis=1)] += 1.0 - Q.sum(axis=1)             # exact: everything is a multiple of 2^-10
    Q[2] = 0.0
    Q[2, K - 1] = 1.0
    Q = Q.astype(np.float32)
    assert (Q.astype(np.float64).sum(axis=1) == 1.0).all() and (Q >= 0).all()
    P = rng.uniform(0.03, 0.97, size=(M, K)).astype(np.float32)
    Q64 = Q.astype(np.float64)
    for _ in range(50):
        pi = Q64 @ P.astype(np.float64).T
        bad = np.zeros(M, dtype=bool)
        for pm in pimins:
            lo, hi = float(np.float32(pm)), float(np.float32(1.0) - np.float32(pm))
            bad |= ((np.abs(pi - lo) < 2e-5) | (np.abs(pi - hi) < 2e-5)).any(axis=0)
        if not bad.any():
            break
        P[bad] = rng.uniform(0.03, 0.97, size=(int(bad.sum()), K)).astype(np.float32)
    else:
        raise AssertionError("could not keep pi away from the mask's bounds")
    P[0] = 0.0
    P[1] = 1.0
    pi = Q64 @ P.astype(np.float64).T
    G = rng.binomial(2, np.clip(pi, 0.0, 1.0)).astype(np.uint8)
    G[rng.random(G.shape) < missing] = 3
    G[4] = 3
    dead = np.asarray([min(100, M - 2), M - 1])
    calls = rng.choice(np.setdiff1d(np.arange(M), dead), size=7, replace=False)
    keep = G[5, calls].copy()
    keep[keep == 3] = 1
    G[5] = 3
    G[5, calls] = keep
    G[:, dead] = 3
    return G, P, Q, dead
