"""A plain numpy restatement of nadm_wld's contract (include/nadm.h) and a small forward simulator of an admixed panel.

``wld_restatement`` follows the contract step by step: the integer moments of every pair over the jointly observed rows (as float64
matrix products of 0/1/2 values, exact far below 2^53, cast to int64), the numerator and the denominator in int64, the same float64
operations in the same order, ``np.rint`` (ties to even, like llrint) to int64, integer sums per bin.  ``simulate`` draws each
haplotype as a mosaic of two sources whose segment lengths are exponential with rate n / 100 per cM."""
import numpy as np


def pack(codes: np.ndarray, ld: int, rng=None) -> np.ndarray:
    """Codes ``[rows, M]`` in 0..3 -> the packed matrix uint8 ``[rows, ld]`` (SNP j in byte j // 4, bits 2 (j % 4) ..); the fields past
    M and the pad bytes are zeros, or garbage with ``rng``."""
    rows, M = codes.shape
    assert ld % 16 == 0 and 4 * ld >= M
    full = np.zeros((rows, 4 * ld), dtype=np.uint8) if rng is None else rng.integers(0, 4, size=(rows, 4 * ld)).astype(np.uint8)
    full[:, :M] = codes
    f = full.reshape(rows, ld, 4)
    return (f[:, :, 0] | (f[:, :, 1] << 2) | (f[:, :, 2] << 4) | (f[:, :, 3] << 6)).astype(np.uint8)


def unpack(xp: np.ndarray, M: int) -> np.ndarray:
    rows, ld = xp.shape
    out = np.empty((rows, ld, 4), dtype=np.uint8)
    for i in range(4):
        out[:, :, i] = (xp >> (2 * i)) & 3
    return out.reshape(rows, 4 * ld)[:, :M]


def wld_restatement(codes: np.ndarray, m0: int, m1: int, W: int, cell, wt, nbins: int, nmin: int = 2):
    """``codes [rows, M]`` (the listed rows, in any order, duplicates included; 3 = missing) -> ``(sum int64 [C, nbins], cnt int64 [nbins])``
    over the pairs m0 <= a < b < m1, b - a <= W."""
    cell, wt = np.asarray(cell, dtype=np.int64), np.asarray(wt, dtype=np.float64)
    C = wt.shape[0]
    seg = codes[:, m0:m1]
    o = (seg != 3).astype(np.float64)
    g = np.where(seg == 3, 0, seg).astype(np.float64)
    n = (o.T @ o).astype(np.int64)                       # [a, b]
    Sa = (g.T @ o).astype(np.int64)
    Sb = (o.T @ g).astype(np.int64)
    Sab = (g.T @ g).astype(np.int64)
    m = m1 - m0
    ia, ib = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    bins = cell[m0 + ib] - cell[m0 + ia]
    take = (ib > ia) & (ib - ia <= W) & (bins < nbins) & (n >= nmin)
    ia, ib, bins = ia[take], ib[take], bins[take]
    n, Sa, Sb, Sab = n[take], Sa[take], Sb[take], Sab[take]
    num, den = n * Sab - Sa * Sb, n * (n - 1)
    v = num.astype(np.float64) / den.astype(np.float64)
    cnt = np.bincount(bins, minlength=nbins).astype(np.int64)
    out = np.zeros((C, nbins), dtype=np.int64)
    for c in range(C):
        t = ((v * wt[c, m0 + ia]) * wt[c, m0 + ib]) * 4294967296.0
        q = np.rint(t).astype(np.int64)
        # integer sums per bin through bincount: the low 24 bits and the rest apart, each sum far below 2^53 and so exact in float64
        assert len(q) < (1 << 28)
        lo, hi = q & 0xFFFFFF, q >> 24
        out[c] = (np.bincount(bins, weights=hi.astype(np.float64), minlength=nbins).astype(np.int64) << 24) + \
            np.bincount(bins, weights=lo.astype(np.float64), minlength=nbins).astype(np.int64)
    return out, cnt


def wld_restatement_ranges(codes, ranges, W, cell, wt, nbins, nmin=2):
    """One ``wld_restatement`` per chromosome range: ``(sum [chrom, C, nbins], cnt [chrom, nbins])``."""
    res = [wld_restatement(codes, m0, m1, W, cell, wt, nbins, nmin) for m0, m1 in ranges]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def simulate(seed: int, N: int, chroms: int, snps: int, spacing: float, n_gen: float, fst: float = 0.2, alpha: float = 0.5,
             miss: float = 0.05):
    """An admixed panel ``n_gen`` generations after a single pulse: ``(codes uint8 [N, chroms snps]`` with 3 = missing, ``cm``, ``chrom``,
    ``pa``, ``pb)``.  SNPs every ``spacing`` cM on each chromosome; source frequencies Balding-Nichols around an ancestral frequency
    uniform on [0.1, 0.9] with the given Fst; along a haplotype the ancestry is redrawn (source a with probability ``alpha``) at the
    points of a Poisson process of rate n_gen / 100 per cM, so its autocovariance at distance d is alpha (1 - alpha) exp(-n d / 100);
    alleles are drawn from the source's frequency; calls go missing independently with probability ``miss``."""
    rng = np.random.default_rng(seed)
    M = chroms * snps
    anc = rng.uniform(0.1, 0.9, size=M)
    s = (1.0 - fst) / fst
    pa, pb = rng.beta(anc * s, (1.0 - anc) * s), rng.beta(anc * s, (1.0 - anc) * s)
    pos = np.arange(snps) * spacing
    length = pos[-1]
    G = np.zeros((N, M), dtype=np.uint8)
    for c in range(chroms):
        sl = slice(c * snps, (c + 1) * snps)
        for hap in range(2):
            nb = rng.poisson(n_gen / 100.0 * length, size=N)
            for i in range(N):
                cuts = np.sort(rng.uniform(0.0, length, size=nb[i]))
                src = rng.random(nb[i] + 1) < alpha                          # True: source a
                from_a = src[np.searchsorted(cuts, pos, side="right")]
                G[i, sl] += (rng.random(snps) < np.where(from_a, pa[sl], pb[sl])).astype(np.uint8)
    G[rng.random((N, M)) < miss] = 3
    cm = np.tile(pos, chroms)
    chrom = np.repeat(np.arange(1, chroms + 1), snps)
    return G, cm, chrom, pa, pb
