"""float64 numpy restatement of the model-fit check (include/nadm.h, nadm_em_sums and nadm_resid_cor), written from the formulas there,
the panels its tests share, and the simulated panels the statistic is calibrated on.

``resid_cor_block`` reads the fp32 ``B`` and ``C`` it is given (on the GPU tests: the ones the device wrote), so that the sums are not
a source of difference; ``em_sums`` is its own float64 form of them.  The fallback branch of the refit is decided in float64 here and
in fp32 on the device: ``resid_cor_block`` asserts that no (b, j, k) of its inputs lies within 2^-10 relative of the threshold, so
that the branch cannot differ between the two sides (the fp32 values that decide it carry a relative error below 2^-18: a few
roundings of 2^-24, amplified by at most 8 in the subtraction B - beta when the refit is kept)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EPS = 1e-6
MIN_SHARE = 0.125            # NADM_LOO_MIN_SHARE
NEAR = 2.0 ** -10


def _clips(eps):
    """The device's clip bounds: eps and 1 - eps as the fp32 numbers the kernels hold."""
    e = np.float32(eps)
    return float(e), float(np.float32(1.0) - e)


def _terms(Gm, P, Q, eps):
    """o, g [b, M] and the clipped terms t1 = o g / r, t0 = o (2 - g) / u [b, M] of every call, float64."""
    lo, hi = _clips(eps)
    Gm = np.asarray(Gm)
    o = Gm != 3
    g = np.where(o, Gm, 0).astype(np.float64)
    rr = np.asarray(Q, dtype=np.float64) @ np.asarray(P, dtype=np.float64).T
    r = np.clip(rr, lo, hi)
    u = np.clip(1.0 - rr, lo, hi)                               # 1 - r from the UNCLIPPED product
    return o, g, np.where(o, g / r, 0.0), np.where(o, (2.0 - g) / u, 0.0)


def em_sums(Gm, P, Q, eps=EPS):
    """B, C float64 [M, K] over the rows of Gm [b, M] (3 = missing), P [M, K], Q [b, K].  Every term is >= 0, so B and C are their
    own sums of magnitudes."""
    o, g, t1, t0 = _terms(Gm, P, Q, eps)
    Qd = np.asarray(Q, dtype=np.float64)
    return t1.T @ Qd, t0.T @ Qd


def loo_freq(g_b, o_b, q_b, P, B, C, eps=EPS, check_near=True):
    """f^{-b} [M, K] for one left-out sample: codes g_b [M] (0 where missing), o_b bool [M], q_b [K]; P, B, C [M, K] float64."""
    lo, hi = _clips(eps)
    rr = P @ q_b
    r, u = np.clip(rr, lo, hi), np.clip(1.0 - rr, lo, hi)
    t1 = np.where(o_b, g_b / r, 0.0)
    t0 = np.where(o_b, (2.0 - g_b) / u, 0.0)
    nb = np.maximum(B - np.outer(t1, q_b), 0.0)
    nc = np.maximum(C - np.outer(t0, q_b), 0.0)
    numn = P * nb
    denn = numn + (1.0 - P) * nc
    den = P * B + (1.0 - P) * C
    take = (denn >= MIN_SHARE * den) & (den > 0) & (denn > 0)
    if check_near:                                              # only where b is observed does the branch enter anything
        thr = MIN_SHARE * den
        near = o_b[:, None] & (den > 0) & (np.abs(denn - thr) <= NEAR * thr)
        assert not near.any(), f"{int(near.sum())} (j, k) within 2^-10 of the fallback threshold: choose other inputs"
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(take, numn / np.where(take, denn, 1.0), P), take


def resid_cor_block(GA, GB, P, QA, QB, B, C, eps=EPS, check_near=True):
    """The rows GA [ba, M] against the LEFT-OUT rows GB [bb, M]: a dict with S, Ta, Tb float64 [ba, bb], n int64 [ba, bb] and the
    sums of magnitudes the tolerances are made of: absS = sum |d_a d_b|, linS = sum o_a o_b (|d_a| + |d_b|), linTa = sum o_a o_b |d_a|,
    linTb = sum o_a o_b |d_b|; ``fallbacks``: how many (b, j, k) with b observed fell back to p."""
    P, B, C = (np.asarray(x, dtype=np.float64) for x in (P, B, C))
    QA, QB = np.asarray(QA, dtype=np.float64), np.asarray(QB, dtype=np.float64)
    GA, GB = np.asarray(GA), np.asarray(GB)
    oA = (GA != 3)
    gA = np.where(oA, GA, 0).astype(np.float64)
    oAf = oA.astype(np.float64)
    ba, bb = GA.shape[0], GB.shape[0]
    out = {k: np.zeros((ba, bb)) for k in ("S", "Ta", "Tb", "absS", "linS", "linTa", "linTb")}
    out["n"] = np.zeros((ba, bb), dtype=np.int64)
    fallbacks = 0
    for b in range(bb):
        o_b = GB[b] != 3
        g_b = np.where(o_b, GB[b], 0).astype(np.float64)
        f, take = loo_freq(g_b, o_b, QB[b], P, B, C, eps, check_near)
        fallbacks += int((~take & o_b[:, None]).sum())
        ob = o_b.astype(np.float64)
        dA = oAf * (gA - 2.0 * (QA @ f.T))
        db = ob * (g_b - 2.0 * (f @ QB[b]))
        out["S"][:, b] = dA @ db
        out["Ta"][:, b] = (dA * dA) @ ob
        out["Tb"][:, b] = oAf @ (db * db)
        out["n"][:, b] = (oA.astype(np.int64) @ o_b.astype(np.int64))
        out["absS"][:, b] = np.abs(dA) @ np.abs(db)
        out["linTa"][:, b] = np.abs(dA) @ ob
        out["linTb"][:, b] = oAf @ np.abs(db)
    out["linS"] = out["linTa"] + out["linTb"]
    out["fallbacks"] = fallbacks
    return out


def cor_of(S, Ta, Tb):
    den = Ta * Tb
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, S / np.sqrt(np.where(den != 0, den, 1.0)), np.nan)


def resid_cor(Gm, P, Q, eps=EPS, B=None, C=None, check_near=False):
    """The symmetrised statistic over all samples of Gm: (cor [N, N] with a NaN diagonal, n [N, N]); B, C default to em_sums."""
    if B is None:
        B, C = em_sums(Gm, P, Q, eps)
    r = resid_cor_block(Gm, Gm, P, Q, Q, B, C, eps, check_near)
    c = cor_of(r["S"], r["Ta"], r["Tb"])
    cor = (c + c.T) * 0.5
    np.fill_diagonal(cor, np.nan)
    return cor, r["n"]


def naive_cor(Gm, P, Q):
    """The plain residual correlation, every residual against the fitted frequencies themselves."""
    Gm = np.asarray(Gm)
    o = (Gm != 3).astype(np.float64)
    d = o * (np.where(Gm != 3, Gm, 0) - 2.0 * (np.asarray(Q, dtype=np.float64) @ np.asarray(P, dtype=np.float64).T))
    S = d @ d.T
    T = (d * d) @ o.T
    c = cor_of(S, T, T.T)
    np.fill_diagonal(c, np.nan)
    return c


# ------------------------------------------------------------------------------------------------ the panel of the GPU tests
def make_panel(N, M, K, seed=0, missing=0.05):
    """Genotypes drawn from the model: P uniform in [0.05, 0.95], Q Dirichlet(1/2), ``missing`` of the calls missing, and the planted
    cases: sample 1 (N > 3) all missing, SNP 3 (M > 5) all missing, and (K > 1, N > 3) the LAST component carried by sample 2 alone,
    which carries nothing else.  -> (Gm uint8 [N, M], P float32 [M, K], Q float32 [N, K])."""
    rng = np.random.default_rng(1000 * seed + 7 * N + 3 * M + K)
    P = rng.uniform(0.05, 0.95, size=(M, K)).astype(np.float32)
    Q = rng.dirichlet(np.full(K, 0.5), size=N)
    if K > 1 and N > 3:
        Q[:, K - 1] = 0.0
        Q /= Q.sum(axis=1, keepdims=True)
        Q[2] = 0.0
        Q[2, K - 1] = 1.0
    Q = Q.astype(np.float32)
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0.0, 1.0)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < missing] = 3
    if N > 3:
        Gm[1] = 3
    if M > 5:
        Gm[:, 3] = 3
    return Gm, P, Q


# ------------------------------------------------------------------------------------------------ calibration panels
def _balding_nichols(rng, M, pops, fst, hi=0.95):
    anc = rng.uniform(0.05, hi, size=M)
    a = anc * (1.0 - fst) / fst
    b = (1.0 - anc) * (1.0 - fst) / fst
    return np.clip(rng.beta(a[:, None], b[:, None], size=(M, pops)), 0.01, 0.99)


def block_em(Gm, P, Q, rounds, eps=EPS, qmin=1e-6, pmin=1e-6):
    """``rounds`` rounds of the float64 block EM over the observed calls (a Q step with P fixed, then a P step with the new Q): the
    steps of tests/project_oracle.py (em_step) and tests/project_p_oracle.py (p_step) without the log-likelihood."""
    Gm = np.asarray(Gm)
    o = Gm != 3
    g = np.where(o, Gm, 0).astype(np.float64)
    h = np.where(o, 2.0 - g, 0.0)
    n2 = 2.0 * o.sum(axis=1, keepdims=True)
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)

    def terms():
        rr = Q @ P.T
        return g / np.clip(rr, eps, 1.0 - eps), h / np.clip(1.0 - rr, eps, 1.0 - eps)
    for _ in range(rounds):
        t1, t0 = terms()
        Qn = np.maximum(Q * (t1 @ P + t0 @ (1.0 - P)) / np.where(n2 > 0, n2, 1.0), qmin)
        Q = np.where(n2 > 0, Qn / Qn.sum(axis=1, keepdims=True), Q)     # a sample without a call keeps its row
        t1, t0 = terms()
        num = P * (t1.T @ Q)
        den = num + (1.0 - P) * (t0.T @ Q)
        P = np.where(den > 0, np.clip(num / np.where(den > 0, den, 1.0), pmin, 1.0 - pmin), P)
    return P, Q


def panel_admixed(seed, N=96, M=6000, K=3, fst=0.1, missing=0.05, admixed=0.3, rounds=200):
    """Panel 1: K populations (Balding-Nichols, Fst 0.1), about 30 % admixed samples (Dirichlet(1)), the others unadmixed; 5 % of the
    calls missing; a joint block-EM fit of ``rounds`` rounds from the truth.  -> (Gm, P fit, Q fit, pop [N]: the population of an
    unadmixed sample, -1 for an admixed one)."""
    rng = np.random.default_rng(seed)
    F = _balding_nichols(rng, M, K, fst)
    pop = rng.integers(0, K, size=N)
    Q = np.eye(K)[pop]
    adm = rng.random(N) < admixed
    Q[adm] = rng.dirichlet(np.ones(K), size=int(adm.sum()))
    pop = np.where(adm, -1, pop)
    Gm = rng.binomial(2, Q @ F.T).astype(np.uint8)
    Gm[rng.random(Gm.shape) < missing] = 3
    P, Qf = block_em(Gm, F, np.clip(Q, 1e-3, None) / np.clip(Q, 1e-3, None).sum(axis=1, keepdims=True), rounds)
    return Gm, P, Qf, pop


def panel_merged(seed, N=96, M=6000, fst=0.1, missing=0.05, rounds=200, hi=0.95):
    """Panel 2: four unadmixed populations fitted with K = 3: the fit starts with the last two sharing the third component (its
    frequencies their mean); ``hi``: the upper end of the ancestral frequencies (below 0.5 the panel is in minor-allele coding).
    -> (Gm, P fit, Q fit, pop [N] in 0..3)."""
    rng = np.random.default_rng(seed)
    F = _balding_nichols(rng, M, 4, fst, hi)
    pop = np.arange(N) % 4
    Gm = rng.binomial(2, F[:, pop].T).astype(np.uint8)
    Gm[rng.random(Gm.shape) < missing] = 3
    P0 = np.stack([F[:, 0], F[:, 1], 0.5 * (F[:, 2] + F[:, 3])], axis=1)
    Q0 = np.full((N, 3), 1e-3)
    Q0[np.arange(N), np.minimum(pop, 2)] = 1.0
    P, Qf = block_em(Gm, P0, Q0 / Q0.sum(axis=1, keepdims=True), rounds)
    return Gm, P, Qf, pop


def pair_means(cor, pop, x, y):
    """(mean, standard deviation, pairs) of cor over the pairs of a sample of population x and one of population y (x == y: a < b)."""
    ix, iy = np.flatnonzero(pop == x), np.flatnonzero(pop == y)
    blk = cor[np.ix_(ix, iy)]
    v = blk[np.triu_indices(len(ix), 1)] if x == y else blk.ravel()
    v = v[~np.isnan(v)]
    return float(v.mean()), float(v.std()), len(v)
