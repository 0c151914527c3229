"""A plain numpy restatement of nadm_local_anc's contract (include/nadm.h) with a ``dtype`` switch, and a forward simulator of an
admixed panel that also returns the true ancestry of every haplotype at every SNP.

``local_anc(..., dtype=np.float64)`` is the yardstick.  ``dtype=np.float32`` follows the contract's arithmetic order: the same
grouping of every product and sum, y ascending in a row sum, a-major over the upper triangle, a multiply-add as one rounding (the
product of two fp32 values is exact in float64; the sum is rounded there and again to fp32, which differs from a fused multiply-add
in rare double roundings), log2 S summed in fp32 within a 256-SNP chunk of the matrix and times ln 2 in float64 across chunks.  The
reciprocal is a correctly rounded division where the hardware's is good to 1 ulp.  The state is kept as the full symmetric K x K
array, the upper triangle computed and mirrored; pad columns hold exact zeros in the library and are left out here."""
import numpy as np

from wld_oracle import pack, unpack  # noqa: F401  (the tests pack their codes with these)

CHUNK = 256


def _fma(a, b, c, dt):
    if dt == np.float64:
        return a * b + c
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _mirror(up):
    """The upper triangle of ``up [n, K, K]`` mirrored into the lower."""
    K = up.shape[1]
    iu = np.triu_indices(K, 1)
    up[:, iu[1], iu[0]] = up[:, iu[0], iu[1]]
    return up


def _rowsum(a):
    """sum over y of a[n, x, y], y ascending."""
    r = a[:, :, 0].copy()
    for y in range(1, a.shape[2]):
        r += a[:, :, y]
    return r


def _seqsum(v):
    """sum over the last axis of v[n, K], ascending."""
    s = v[:, 0].copy()
    for x in range(1, v.shape[1]):
        s += v[:, x]
    return s


def _emission(codes_j, Pj, eps, ome, dt):
    """e [n, K, K] (both triangles by the upper triangle's formula; the caller mirrors what it keeps)."""
    one = dt(1.0)
    p = np.minimum(np.maximum(Pj, eps), ome)
    c = np.minimum(np.maximum(one - Pj, eps), ome)
    n = len(codes_j)
    cj = codes_j[:, None]
    u = np.where(cj == 3, one, np.where(cj == 0, c[None, :], p[None, :])).astype(dt)
    v = np.where(cj == 3, one, np.where(cj == 2, p[None, :], c[None, :])).astype(dt)
    w = np.where(cj == 1, c[None, :], dt(0.0)).astype(dt) * np.ones((n, 1), dtype=dt)
    return _fma(u[:, :, None], v[:, None, :], (u[:, None, :] * w[:, :, None]).astype(dt), dt)


def _coef(r, dt):
    s = dt(1.0) - r
    return dt(s * s), dt(r * s), dt(dt(0.5) * dt(r * r))


def pair_index(K):
    """The a-major list of the pairs x <= y < K."""
    return [(a, d) for a in range(K) for d in range(a, K)]


def local_anc(codes, P, Q, eps, rho, seg, out_snp=None, oseg=None, dtype=np.float64):
    """``codes [n, M]`` (3 = missing), ``P [M, K]``, ``Q [n, K]``, ``rho [M]``, ``seg [n_seg + 1]``, ``out_snp [n_out]``, ``oseg [n_seg + 1]``
    -> a dict: ``ll`` float64 ``[n, n_seg]`` and, with output points, ``dosage [n, n_out, K]``, ``call`` uint8 ``[n, n_out]``, ``post
    [n, n_out]`` and ``gap [n, n_out]``, the difference of the two largest pair masses (the first two in ``dtype``)."""
    dt = np.float32 if dtype == np.float32 else np.float64
    codes = np.asarray(codes)
    n, M = codes.shape
    P, Q = np.asarray(P).astype(np.float32).astype(dt), np.asarray(Q).astype(np.float32).astype(dt)
    K = P.shape[1]
    eps = dt(np.float32(eps))
    ome = dt(np.float32(1.0) - np.float32(eps))
    rho = np.asarray(rho).astype(np.float32).astype(dt)
    seg = [int(s) for s in seg]
    n_seg = len(seg) - 1
    ln2 = np.log(2.0)
    ll = np.zeros((n, n_seg), dtype=np.float64)
    full = out_snp is not None and len(out_snp) > 0
    out = {"ll": ll}
    if full:
        out_snp = [int(j) for j in out_snp]
        n_out = len(out_snp)
        ckpt = {}
        out.update(dosage=np.zeros((n, n_out, K), dtype=dt), call=np.zeros((n, n_out), dtype=np.uint8),
                   post=np.zeros((n, n_out), dtype=dt), gap=np.zeros((n, n_out), dtype=dt))
    pairs = pair_index(K)
    pa, pd = np.array([a for a, _ in pairs]), np.array([d for _, d in pairs])
    qq = (Q[:, :, None] * Q[:, None, :]).astype(dt)
    sup = (qq > 0).astype(dt)
    with np.errstate(all="ignore"):
        for sg in range(n_seg):
            s0, s1 = seg[sg], seg[sg + 1]
            if s0 >= s1:
                continue
            opts = list(range(int(oseg[sg]), int(oseg[sg + 1]))) if full else []
            o = 0
            A = np.zeros((n, K, K), dtype=dt)
            R = np.zeros((n, K), dtype=dt)
            lsum = np.zeros(n, dtype=dt)
            for j in range(s0, s1):
                r = dt(1.0) if j == s0 else rho[j]
                c0, c1, hc2 = _coef(r, dt)
                e = _emission(codes[:, j], P[j], eps, ome, dt)
                G = _fma(c1, R, (hc2 * Q).astype(dt), dt)
                inner = _fma(Q[:, None, :], G[:, :, None], (Q[:, :, None] * G[:, None, :]).astype(dt), dt)
                val = _mirror((_fma(c0, A, inner, dt) * e).astype(dt))
                Rn = _rowsum(val)
                S = _seqsum(Rn)
                inv = (dt(1.0) / S).astype(dt)
                A = (val * inv[:, None, None]).astype(dt)
                R = (Rn * inv[:, None]).astype(dt)
                lsum += np.log2(S).astype(dt)
                if (j + 1) % CHUNK == 0 or j == s1 - 1:
                    ll[:, sg] += lsum.astype(np.float64) * ln2
                    lsum[:] = 0
                if o < len(opts) and out_snp[opts[o]] == j:
                    ckpt[opts[o]] = A.copy()
                    o += 1
            if not opts:
                continue
            first = out_snp[opts[0]]
            B = sup.copy()
            o = len(opts) - 1
            for j in range(s1 - 1, first - 1, -1):
                if o >= 0 and out_snp[opts[o]] == j:
                    g = (ckpt[opts[o]] * B).astype(dt)
                    D = _rowsum(g)
                    Z = _seqsum(D)
                    inv = (dt(1.0) / Z).astype(dt)
                    ok = (Z > 0) & np.isfinite(Z)
                    mass = np.where(pa == pd, g[:, pa, pd], g[:, pa, pd] + g[:, pa, pd]).astype(dt)
                    bi = np.argmax(np.where(np.isnan(mass), -1, mass), axis=1)
                    best = mass[np.arange(n), bi]
                    srt = np.sort(np.where(np.isnan(mass), -1, mass), axis=1)
                    second = srt[:, -2] if mass.shape[1] > 1 else np.zeros(n, dtype=dt)
                    dos = np.minimum(dt(2.0) * (D * inv[:, None]).astype(dt), dt(2.0)).astype(dt)
                    k = opts[o]
                    out["dosage"][:, k] = np.where(ok[:, None], dos, np.nan)
                    out["call"][:, k] = np.where(ok, bi, 255).astype(np.uint8)
                    out["post"][:, k] = np.where(ok, (best * inv).astype(dt), np.nan)
                    out["gap"][:, k] = np.where(ok, ((best - second) * inv).astype(dt), np.nan)
                    o -= 1
                if j <= first:
                    break
                c0, c1, hc2 = _coef(rho[j], dt)
                h = _mirror((B * _emission(codes[:, j], P[j], eps, ome, dt)).astype(dt))
                H = np.zeros((n, K), dtype=dt)
                for y in range(K):
                    H = _fma(Q[:, y][:, None], h[:, :, y], H, dt)
                Tt = np.zeros(n, dtype=dt)
                for x in range(K):
                    Tt = _fma(Q[:, x], H[:, x], Tt, dt)
                hT = (hc2 * Tt).astype(dt)
                J = _fma(c1, H, hT[:, None], dt)
                val = (sup * _fma(c0, h, (J[:, :, None] + J[:, None, :]).astype(dt), dt)).astype(dt)
                Zd = np.zeros(n, dtype=dt)
                Zo = np.zeros(n, dtype=dt)
                for a, d in pairs:
                    if a == d:
                        Zd += val[:, a, a]
                    else:
                        Zo += val[:, a, d]
                inv = (dt(1.0) / _fma(dt(2.0), Zo, Zd, dt)).astype(dt)
                B = _mirror((val * inv[:, None, None]).astype(dt))
    return out


def simulate(seed: int, N: int, chroms: int, snps: int, spacing: float, n_gen: float, K: int = 3, fst: float = 0.2, miss: float = 0.05,
             Q=None, alpha: float = 1.0):
    """An admixed panel ``n_gen`` generations after a single pulse: ``(codes uint8 [N, M]`` with 3 = missing, ``cm``, ``chrom``, ``P [M, K]``,
    ``Q [N, K]``, ``anc uint8 [N, M, K])``, M = chroms snps.  ``anc[i, j, k]`` counts the haplotypes (0, 1, 2) of sample i whose ancestry
    at SNP j is k: the true dosage.  SNPs every ``spacing`` cM; source frequencies Balding-Nichols around an ancestral frequency
    uniform on [0.1, 0.9]; ``Q`` per sample (default: Dirichlet(alpha)); along a haplotype the ancestry is redrawn from the sample's
    ``Q`` row at the points of a Poisson process of rate n_gen / 100 per cM; alleles are drawn from the ancestry's frequency; calls go
    missing independently with probability ``miss``."""
    rng = np.random.default_rng(seed)
    M = chroms * snps
    base = rng.uniform(0.1, 0.9, size=M)
    s = (1.0 - fst) / fst
    P = np.stack([rng.beta(base * s, (1.0 - base) * s) for _ in range(K)], axis=1)
    Q = rng.dirichlet(np.full(K, alpha), size=N) if Q is None else np.asarray(Q, dtype=np.float64)
    pos = np.arange(snps) * spacing
    length = pos[-1] if snps > 1 else 0.0
    G = np.zeros((N, M), dtype=np.uint8)
    anc = np.zeros((N, M, K), dtype=np.uint8)
    cols = np.arange(snps)
    for c in range(chroms):
        sl = slice(c * snps, (c + 1) * snps)
        Pc = P[sl]
        for hap in range(2):
            nb = rng.poisson(n_gen / 100.0 * length, size=N)
            for i in range(N):
                cuts = np.sort(rng.uniform(0.0, length, size=nb[i]))
                src = rng.choice(K, size=nb[i] + 1, p=Q[i])
                a = src[np.searchsorted(cuts, pos, side="right")]
                anc[i, c * snps + cols, a] += 1
                G[i, sl] += (rng.random(snps) < Pc[cols, a]).astype(np.uint8)
    G[rng.random((N, M)) < miss] = 3
    cm = np.tile(pos, chroms)
    chrom = np.repeat(np.arange(1, chroms + 1), snps)
    return G, cm, chrom, P, Q, anc
