"""numpy restatement of LD pruning (include/nadm.h: nadm_snp_counts, nadm_ld_band, nadm_ld_sweep) in int64 / float64, and the data
of tests/test_ld.py.  The moments are explicit masked sums, r^2 is the header's formula with one IEEE operation per step, the sweep
is the header's double loop, literally.  Nothing here knows how the library computes any of it."""
import numpy as np


def counts(G):
    """int64 [M, 3]: observed calls, their sum, their sum of squares per SNP of the genotype matrix G uint8 [rows, M] (3 = missing)."""
    G = np.asarray(G).astype(np.int64)
    o = (G != 3).astype(np.int64)
    g = G * o
    return np.stack([o.sum(axis=0), g.sum(axis=0), (g * g).sum(axis=0)], axis=1)


def maf(cnt):
    n, S = cnt[:, 0].astype(np.int64), cnt[:, 1].astype(np.int64)
    out = np.zeros(len(n), dtype=np.float64)
    for j in range(len(n)):
        if n[j] > 0:
            out[j] = float(min(S[j], 2 * n[j] - S[j])) / (2.0 * float(n[j]))
    return out


def r2_of(mom):
    """The header's formula on int64 moments [..., 6] -> float64 [...]; exactly 0.0 where va == 0 or vb == 0."""
    mom = np.asarray(mom).astype(np.int64)
    n, Sa, Sb, Sab, Saa, Sbb = (mom[..., i] for i in range(6))
    cov, va, vb = n * Sab - Sa * Sb, n * Saa - Sa * Sa, n * Sbb - Sb * Sb
    num = cov.astype(np.float64) * cov.astype(np.float64)
    den = va.astype(np.float64) * vb.astype(np.float64)
    ok = (va != 0) & (vb != 0)
    out = np.zeros(num.shape, dtype=np.float64)
    out[ok] = num[ok] / den[ok]
    return out


def band(G, W, m0=0, m1=None):
    """(r2 float64 [m1 - m0, W], mom int64 [m1 - m0, W, 6]) of G uint8 [rows, M]: entry (j - m0, d) is the pair (j, j + 1 + d), the sums
    over the rows where both calls are observed; zeros where j + 1 + d >= M."""
    G = np.asarray(G).astype(np.int64)
    M = G.shape[1]
    m1 = M if m1 is None else m1
    o = (G != 3).astype(np.int64)
    g = G * o
    g2 = g * g
    mom = np.zeros((m1 - m0, W, 6), dtype=np.int64)
    for d in range(W):
        hi = min(m1, M - 1 - d)                              # pairs (j, j + 1 + d) with j + 1 + d < M
        if hi <= m0:
            continue
        a, b = slice(m0, hi), slice(m0 + 1 + d, hi + 1 + d)
        mom[: hi - m0, d, 0] = (o[:, a] * o[:, b]).sum(axis=0)
        mom[: hi - m0, d, 1] = (g[:, a] * o[:, b]).sum(axis=0)
        mom[: hi - m0, d, 2] = (o[:, a] * g[:, b]).sum(axis=0)
        mom[: hi - m0, d, 3] = (g[:, a] * g[:, b]).sum(axis=0)
        mom[: hi - m0, d, 4] = (g2[:, a] * o[:, b]).sum(axis=0)
        mom[: hi - m0, d, 5] = (o[:, a] * g2[:, b]).sum(axis=0)
    return r2_of(mom), mom


def sweep(r2, m0, m1, W, M, maf_, chrom, thr, kept):
    """The header's rule, in place on kept (uint8 [M])."""
    for i in range(m0, m1):
        if not kept[i]:
            continue
        for d in range(W):
            j = i + 1 + d
            if j >= M:
                break
            if chrom is not None and chrom[j] != chrom[i]:
                break
            if not kept[j]:
                continue
            if r2[i - m0, d] > thr:
                if maf_[i] < maf_[j]:
                    kept[i] = 0
                    break
                kept[j] = 0
    return kept


def prune(G, window, thr, chrom=None):
    G = np.asarray(G)
    M = G.shape[1]
    r2, _ = band(G, window - 1)
    return sweep(r2, 0, M, window - 1, M, maf(counts(G)), chrom, thr, np.ones(M, dtype=np.uint8)).astype(bool)


# ---- data -------------------------------------------------------------------------------------------------------------------------
def random_genotypes(rows, M, seed, missing=0.3):
    """Codes 0, 1, 2 from per-SNP frequencies, neighbouring SNPs correlated (every SNP copies its predecessor's call with probability
    0.5), `missing` of the calls set to 3; a monomorphic SNP, an all-missing SNP and a pair without a jointly observed row planted
    where M allows."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=M)
    G = rng.binomial(2, f, size=(rows, M)).astype(np.uint8)
    for j in range(1, M):
        copy = rng.random(rows) < 0.5
        G[copy, j] = G[copy, j - 1]
    G[rng.random((rows, M)) < missing] = 3
    if M >= 5:
        G[:, 1] = np.where(G[:, 1] == 3, 3, 1)               # monomorphic among its observed calls
        G[:, 3] = 3                                          # missing in every row
    if M >= 64 and rows >= 2:
        half = np.arange(rows) % 2 == 0
        G[half, 40] = 3
        G[~half, 42] = 3                                     # SNPs 40 and 42 share no observed row
    return G


def pack(G, ld_round=16, dirty=False, extra_rows=0):
    """Packed rows uint8 [rows + extra_rows, ld] (numpy): SNP 4c + i in bits [2i, 2i + 1] of byte c, ld = ceil(M/4) rounded up to
    `ld_round`.  dirty: every bit that holds no SNP set; the extra rows are all 0xFF (dirty) or zeros."""
    G = np.asarray(G, dtype=np.uint8)
    rows, M = G.shape
    ld = ((M + 3) // 4 + ld_round - 1) // ld_round * ld_round
    codes = np.zeros((rows, 4 * ld), dtype=np.uint8)
    codes[:, :M] = G
    if dirty:
        codes[:, M:] = 3
    c4 = codes.reshape(rows, ld, 4)
    out = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)
    if extra_rows:
        out = np.concatenate([out, np.full((extra_rows, ld), 0xFF if dirty else 0, dtype=np.uint8)], axis=0)
    return np.ascontiguousarray(out)


def unpack(packed, M):
    p = np.asarray(packed)
    out = np.stack([(p >> (2 * i)) & 3 for i in range(4)], axis=2).reshape(p.shape[0], -1)
    return out[:, :M]


def make_panel(rows=200, M=3000, seed=7):
    """A panel for pruning: runs of near-duplicated SNPs (a founder SNP and 1..5 copies with 2 % of the calls redrawn) between
    independent SNPs, 2 % missing.  The keep-list of window 50, r2 0.1 is neither everything nor nothing."""
    rng = np.random.default_rng(seed)
    G = np.empty((rows, M), dtype=np.uint8)
    j = 0
    while j < M:
        f = rng.uniform(0.1, 0.9)
        base = rng.binomial(2, f, size=rows).astype(np.uint8)
        G[:, j] = base
        j += 1
        if rng.random() < 0.4:
            for _ in range(int(rng.integers(1, 6))):
                if j >= M:
                    break
                c = base.copy()
                redo = rng.random(rows) < 0.02
                c[redo] = rng.binomial(2, f, size=int(redo.sum()))
                G[:, j] = c
                j += 1
    G[rng.random((rows, M)) < 0.02] = 3
    return G


def write_bed(prefix, G, ids=None, chroms=None):
    """G uint8 [N, M] (codes as the reader returns them for an unflipped file) -> prefix.bed / .bim / .fam.  The reader's table maps the
    PLINK fields 0, 1, 2, 3 to the codes 2, 3, 1, 0."""
    G = np.asarray(G, dtype=np.uint8)
    N, M = G.shape
    field = np.asarray([3, 2, 0, 1], dtype=np.uint8)[G]       # code -> PLINK field
    nb = (N + 3) // 4
    pad = np.zeros((4 * nb, M), dtype=np.uint8)
    pad[:N] = field
    p4 = pad.T.reshape(M, nb, 4)
    body = (p4[:, :, 0] | (p4[:, :, 1] << 2) | (p4[:, :, 2] << 4) | (p4[:, :, 3] << 6)).astype(np.uint8)
    with open(f"{prefix}.bed", "wb") as fb:
        fb.write(bytes([0x6C, 0x1B, 0x01]))
        fb.write(body.tobytes())
    ids = [f"rs{j}" for j in range(M)] if ids is None else ids
    chroms = ["1"] * M if chroms is None else chroms
    with open(f"{prefix}.bim", "w") as fb:
        for j in range(M):
            fb.write(f"{chroms[j]}\t{ids[j]}\t0\t{j + 1}\tA\tG\n")
    with open(f"{prefix}.fam", "w") as fb:
        for i in range(N):
            fb.write(f"f{i} s{i} 0 0 0 -9\n")
