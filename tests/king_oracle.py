"""numpy restatement of KING-robust kinship (include/nadm.h: nadm_king) in int64 / float64, and the data of tests/test_king.py.  The
counts are explicit masked sums over the SNPs both samples were called at, phi is the header's formula; ``brute`` is the same as a
double loop over pairs and a loop over SNPs, literally.  Nothing here knows how the library computes any of it."""
import functools

import numpy as np

# lower edges of the degree bands (KING's): duplicate / twin, first, second, third degree
EDGES = (2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5, 2.0 ** -4.5)


def counts(GA, GB):
    """int64 [5, ba, bb]: n, hethet, ibs0, het_a, het_b of the rows of GA uint8 [ba, M] against the rows of GB uint8 [bb, M]
    (codes 0, 1, 2; 3 = missing)."""
    GA, GB = np.asarray(GA), np.asarray(GB)

    def ind(v):
        return v.astype(np.float64)                          # 0 / 1 indicators: their products sum exactly in float64 (M < 2^53)
    oa, ob, ha, hb = ind(GA != 3), ind(GB != 3), ind(GA == 1), ind(GB == 1)
    za, zb, ta, tb = ind(GA == 0), ind(GB == 0), ind(GA == 2), ind(GB == 2)
    return np.rint(np.stack([oa @ ob.T, ha @ hb.T, za @ tb.T + ta @ zb.T, ha @ ob.T, oa @ hb.T])).astype(np.int64)


def brute(GA, GB):
    """(counts int64 [5, ba, bb], phi float64 [ba, bb]) by the definition: a loop over the pairs and over the SNPs."""
    ba, bb, M = len(GA), len(GB), GA.shape[1]
    c = np.zeros((5, ba, bb), dtype=np.int64)
    phi = np.full((ba, bb), np.nan)
    for a in range(ba):
        for b in range(bb):
            n = hethet = ibs0 = het_a = het_b = 0
            for j in range(M):
                ga, gb = int(GA[a, j]), int(GB[b, j])
                if ga == 3 or gb == 3:
                    continue
                n += 1
                hethet += ga == 1 and gb == 1
                ibs0 += (ga == 0 and gb == 2) or (ga == 2 and gb == 0)
                het_a += ga == 1
                het_b += gb == 1
            c[:, a, b] = n, hethet, ibs0, het_a, het_b
            if min(het_a, het_b) > 0:
                phi[a, b] = 0.5 - (het_a + het_b - 2 * hethet + 4 * ibs0) / (4.0 * min(het_a, het_b))
    return c, phi


def band(phi):
    """0 duplicate / twin, 1 first, 2 second, 3 third degree, 4 below (NaN: 4)."""
    for k, e in enumerate(EDGES):
        if phi >= e:
            return k
    return 4


def random_genotypes(rows, M, seed, missing=0.1):
    """Codes 0, 1, 2 from per-SNP frequencies with `missing` of the calls set to 3.  Planted where rows allow: row 1 a copy of row 0
    (a duplicate), row 2 without a heterozygous call, row 3 all missing, row 4 the 0 <-> 2 mirror of row 0 (every jointly observed
    homozygous call opposite)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=M)
    G = rng.binomial(2, f, size=(rows, M)).astype(np.uint8)
    G[rng.random((rows, M)) < missing] = 3
    if rows > 4:
        G[1] = G[0]
        G[2] = np.where(G[2] == 1, 2, G[2])
        G[3] = 3
        G[4] = np.where(G[0] == 3, 3, 2 - G[0])
    return G


def flip(G):
    """The reader's 0 <-> 2 flip: 3 stays 3."""
    G = np.asarray(G)
    return np.where(G == 3, 3, 2 - G).astype(np.uint8)


# ---- the planted panel -----------------------------------------------------------------------------------------------------------
FAMILIES, FAMILY_SIZE, UNRELATED = 12, 7, 40
PANEL_N = FAMILIES * FAMILY_SIZE + UNRELATED               # 124
# within a family: founders 0, 1, 2; full sibs 3, 4 (children of 0 and 1); half sib 5 (child of 1 and 2); 6 a duplicate of 3
FAM_DUPLICATE = [(3, 6)]
FAM_FIRST = [(0, 3), (0, 4), (0, 6), (1, 3), (1, 4), (1, 6), (1, 5), (2, 5), (3, 4), (4, 6)]
FAM_SECOND = [(3, 5), (4, 5), (5, 6)]


def _child(rng, ga, gb):
    """Mendelian transmission: one allele of each parent's genotype (codes 0, 1, 2), SNPs independent."""
    def gamete(g):
        return np.where(g == 1, rng.integers(0, 2, size=g.shape), g // 2)
    return (gamete(ga) + gamete(gb)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def make_panel(seed=0, M=12000):
    """(G uint8 [124, M], degree int8 [124, 124]) -- two populations at Fst 0.1 from a Balding-Nichols draw and one admixed class
    (every founder its own fraction in [0.3, 0.7], a genotype binomial(2, q p0 + (1 - q) p1)); twelve families of seven (four per
    class: three founders, two full sibs, a half sib, a duplicate of the first sib), then 40 unrelated samples; 5 % of the calls
    missing.  degree: 0 duplicate, 1 first, 2 second degree, 9 unrelated (the diagonal -1)."""
    rng = np.random.default_rng(seed)
    F = 0.1
    anc = rng.uniform(0.1, 0.9, size=M)
    p = np.stack([rng.beta(anc * (1 - F) / F, (1 - anc) * (1 - F) / F) for _ in range(2)])

    def founder(cls):
        q = (1.0, 0.0, rng.uniform(0.3, 0.7))[cls]
        return rng.binomial(2, q * p[0] + (1 - q) * p[1]).astype(np.uint8)
    rows = []
    degree = np.full((PANEL_N, PANEL_N), 9, dtype=np.int8)
    for fam in range(FAMILIES):
        cls = fam % 3
        f0, f1, f2 = founder(cls), founder(cls), founder(cls)
        s1, s2, hs = _child(rng, f0, f1), _child(rng, f0, f1), _child(rng, f1, f2)
        base = len(rows)
        rows += [f0, f1, f2, s1, s2, hs, s1.copy()]
        for d, pairs in ((0, FAM_DUPLICATE), (1, FAM_FIRST), (2, FAM_SECOND)):
            for a, b in pairs:
                degree[base + a, base + b] = degree[base + b, base + a] = d
    rows += [founder(u % 3) for u in range(UNRELATED)]
    G = np.stack(rows)
    G[rng.random(G.shape) < 0.05] = 3
    np.fill_diagonal(degree, -1)
    G.setflags(write=False)
    degree.setflags(write=False)
    return G, degree
