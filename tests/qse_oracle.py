"""Float64 numpy restatement of the standard errors of Q given P (neural_admixture_amd/qse.py, include/nadm.h nadm_sample_info): the
per-sample expected information, both forms of its inverse under the constraint sum_k q_k = 1, a float32 restatement of the kernel's
arithmetic (the yardstick of tests/test_q_se.py), the masked projection EM, and the seeded calibration experiment of DESIGN.md 4.18.
G is uint8 [n, M] with codes 0, 1, 2 and 3 = missing."""
import numpy as np

EPS = 1e-6
CHUNK = 256


def pairs(K):
    return [(a, b) for a in range(K) for b in range(a, K)]


def weights(G, P, Q, eps=EPS):
    """w [n, M] float64: o 2 / (clip(pi) clip(1 - pi)), exactly 0 where the call is missing."""
    pi = np.asarray(Q, np.float64) @ np.asarray(P, np.float64).T
    r, u = np.clip(pi, eps, 1 - eps), np.clip(1 - pi, eps, 1 - eps)
    return np.where(np.asarray(G) != 3, 2.0 / (r * u), 0.0)


def info(G, P, Q, eps=EPS):
    """(info float64 [n, K (K + 1) / 2], the pairs a <= b a-major; n int32 [n]).  Every entry is one sum over the SNPs of elementwise
    products, so two equal columns of P give bit-equal entries."""
    P = np.asarray(P, np.float64)
    w = weights(G, P, Q, eps)
    out = np.stack([(w * (P[:, a] * P[:, b])[None, :]).sum(axis=1) for a, b in pairs(P.shape[1])], axis=1)
    return out, (np.asarray(G) != 3).sum(axis=1).astype(np.int32)


def info32(G, P, Q, chunks_per_range, eps=EPS):
    """The kernel's arithmetic in float32 without its fused multiply-adds: pi with k in order, an fp32 product r u and an fp32 division,
    fp32 products w p_a and (w p_a) p_b, fp32 sums in SNP order over ranges of ``chunks_per_range`` 256-SNP chunks, the ranges added
    in float64, the factor 2 last."""
    f = np.float32
    G, P, Q = np.asarray(G), np.asarray(P, f), np.asarray(Q, f)
    n, M, K = G.shape[0], P.shape[0], P.shape[1]
    pi = np.zeros((n, M), f)
    for k in range(K):
        pi = (Q[:, k, None] * P[None, :, k] + pi).astype(f)
    r = np.minimum(np.maximum(pi, f(eps)), f(1) - f(eps))
    u = np.minimum(np.maximum(f(1) - pi, f(eps)), f(1) - f(eps))
    w = np.where(G != 3, f(1) / (r * u).astype(f), f(0)).astype(f)
    span = chunks_per_range * CHUNK
    out = np.zeros((n, len(pairs(K))), np.float64)
    for i, (a, b) in enumerate(pairs(K)):
        term = ((w * P[None, :, a]).astype(f) * P[None, :, b]).astype(f)
        for lo in range(0, M, span):
            out[:, i] += np.cumsum(term[:, lo:lo + span], axis=1, dtype=f)[:, -1].astype(np.float64)
    return 2.0 * out


def full(I, K):
    """info rows -> symmetric [n, K, K]."""
    A = np.zeros((I.shape[0], K, K))
    for i, (a, b) in enumerate(pairs(K)):
        A[:, a, b] = A[:, b, a] = I[:, i]
    return A


def _chol_ok(J):
    try:
        np.linalg.cholesky(J)
        return True
    except np.linalg.LinAlgError:
        return False


def se_drop(A, c):
    """One sample, the drop-one form: J = D^T A D with component c left out; sqrt(diag(J^-1)) for a != c, NaN at c and NaN throughout
    when J is not positive definite."""
    K = A.shape[0]
    keep = [a for a in range(K) if a != c]
    J = (A[np.ix_(keep, keep)] - A[c, keep][None, :]) - (A[keep, c][:, None] - A[c, c])
    out = np.full(K, np.nan)
    if K > 1 and _chol_ok(J):
        try:
            with np.errstate(invalid="ignore"):
                out[keep] = np.sqrt(np.diag(np.linalg.inv(J)))
        except np.linalg.LinAlgError:                               # (a pivot that rounded to +0: singular all the same)
            pass
    return out


def se_schur(A):
    """One sample, the constrained form: Cov = A^-1 - A^-1 1 1^T A^-1 / (1^T A^-1 1)."""
    K = A.shape[0]
    if not _chol_ok(A):
        return np.full(K, np.nan)
    Ai = np.linalg.inv(A)
    v = Ai.sum(axis=1)
    return np.sqrt(np.maximum(np.diag(Ai - np.outer(v, v) / v.sum()), 0.0))


def se(I, K, n, vif_cap=1e12):
    """[n, K]: the drop-one form twice (c = K - 1, then c = 0 for the last component), as qse.se_from_info; NaN throughout where n =
    0, the block is not positive definite or a component's variance inflation exceeds ``vif_cap``; K = 1: exactly 0."""
    A = full(np.asarray(I, np.float64), K)
    out = np.full((A.shape[0], K), np.nan)
    for i in range(A.shape[0]):
        if n[i] == 0:
            continue
        if K == 1:
            out[i] = 0.0
            continue
        first, last = se_drop(A[i], K - 1), se_drop(A[i], 0)
        row = np.concatenate([first[:K - 1], last[K - 1:]])
        for c, s in ((K - 1, first), (0, last)):
            keep = [a for a in range(K) if a != c]
            Jd = A[i][keep, keep] - 2 * A[i][c, keep] + A[i][c, c]
            if not np.all(s[keep] ** 2 * Jd <= vif_cap):
                row[:] = np.nan
        out[i] = row if not np.isnan(row).any() else np.nan
    return out


def se_at(G, P, Q):
    """The two together: the standard errors [n, K] of Q given P on the panel G."""
    I, n = info(G, P, Q)
    return se(I, np.shape(P)[1], n)


# ------------------------------------------------------------------------------------------------ the calibration experiment
def project_em(G, P, iters=400, qmin=1e-9, eps=EPS):
    """Masked projection EM of Q given P in float64 from the uniform start (nadm_project_q's step): G [..., n, M] -> Q [..., n, K]."""
    P = np.asarray(P, np.float64)
    K = P.shape[1]
    o = (G != 3)
    g = np.where(o, G, 0).astype(np.float64)
    h = np.where(o, 2.0 - g, 0.0)
    nobs = o.sum(axis=-1, keepdims=True).astype(np.float64)
    Q = np.full(G.shape[:-1] + (K,), 1.0 / K)
    for _ in range(iters):
        pi = Q @ P.T
        t1, t0 = g / np.clip(pi, eps, 1 - eps), h / np.clip(1 - pi, eps, 1 - eps)
        Q = Q * (t1 @ P + t0 @ (1.0 - P)) / (2.0 * nobs)
        Q = np.maximum(Q, qmin)
        Q /= Q.sum(axis=-1, keepdims=True)
    return Q


def project_fit(G, P, em_iters=10, iters=15, qmin=1e-9, eps=EPS):
    """The maximum of the masked likelihood of Q given P on the simplex, in float64: a few EM steps from the uniform start (the EM alone
    needs thousands of steps here), then Fisher scoring under the sum constraint with an active set -- a component at the floor
    ``qmin`` whose step points outwards is held there, and a step is cut where it would cross the floor.  G [..., n, M] -> Q [..., n, K]."""
    P = np.asarray(P, np.float64)
    K = P.shape[1]
    o = (G != 3)
    g = np.where(o, G, 0).astype(np.float64)
    h = np.where(o, 2.0 - g, 0.0)
    PP = np.stack([P[:, a] * P[:, b] for a, b in pairs(K)], axis=1)
    ia, ib = np.array(pairs(K)).T
    Q = project_em(G, P, iters=em_iters, qmin=qmin, eps=eps)

    def step(A, s, free):
        f = free.astype(np.float64)
        Af = A * f[..., :, None] * f[..., None, :] + (1.0 - f)[..., :, None] * np.eye(K)
        Ai = np.linalg.inv(Af)
        sf = s * f
        x, v = (Ai @ sf[..., None])[..., 0], (Ai @ f[..., None])[..., 0]
        return (x - v * ((f * x).sum(-1) / (f * v).sum(-1))[..., None]) * f

    for _ in range(iters):
        pi = Q @ P.T
        r, u = np.clip(pi, eps, 1 - eps), np.clip(1 - pi, eps, 1 - eps)
        s = (g / r - h / u) @ P
        I = (np.where(o, 2.0 / (r * u), 0.0)) @ PP
        A = np.zeros(Q.shape + (K,))
        A[..., ia, ib] = I
        A[..., ib, ia] = I
        fixed = np.zeros(Q.shape, bool)
        for _ in range(K - 1):
            d = step(A, s, ~fixed)
            more = ~fixed & (Q <= qmin * (1 + 1e-9)) & (d < 0)
            more &= (~(fixed | more)).sum(-1, keepdims=True) >= 1
            if not more.any():
                break
            fixed |= more
        d = step(A, s, ~fixed)
        with np.errstate(divide="ignore", invalid="ignore"):
            room = np.where(d < 0, (Q - qmin) / -d, np.inf).min(axis=-1, keepdims=True)
        Q = np.maximum(Q + np.minimum(1.0, room) * d, qmin)
        Q /= Q.sum(axis=-1, keepdims=True)
    return Q


def make_panel(seed, n_interior=12, n_pure=12, M=3000, K=3, fst=0.1):
    """(P [M, K], Qtrue [n, K], interior bool [n]): Balding-Nichols frequencies around ancestral ones in [0.1, 0.9]; interior samples
    with every q_k > 0.05, unadmixed ones cycling through the components."""
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.1, 0.9, M)
    s = (1 - fst) / fst
    P = np.clip(rng.beta(anc[:, None] * s, (1 - anc[:, None]) * s, (M, K)), 0.01, 0.99)
    Qi = np.empty((0, K))
    while len(Qi) < n_interior:
        d = rng.dirichlet(np.full(K, 2.0), 4 * n_interior)
        Qi = np.concatenate([Qi, d[d.min(axis=1) > 0.05]])[:n_interior]
    Qp = np.eye(K)[np.arange(n_pure) % K]
    return P, np.concatenate([Qi, Qp]), np.arange(n_interior + n_pure) < n_interior


def draw(rng, P, Q, missing=0.05, reps=None):
    """Genotypes binomial(2, Q P^T) with ``missing`` of the calls masked: uint8 [n, M], or [reps, n, M]."""
    pi = Q @ P.T
    shape = pi.shape if reps is None else (reps,) + pi.shape
    G = rng.binomial(2, np.broadcast_to(pi, shape)).astype(np.uint8)
    G[rng.random(shape) < missing] = 3
    return G


def calibration(seed, reps=60):
    """The experiment of DESIGN.md 4.18: P fixed at the truth, ``reps`` independently drawn panels, Q fitted by the projection EM, the SE
    at the fitted Q.  Returns (ratio: the median over interior samples and components of median-SE / spread-of-estimate; coverage: the
    share of |z| < 1.96 over interior samples, components and panels; pure_se, pure_spread: over the unadmixed samples' ABSENT
    components the median SE and the median spread of the (truncated) estimate)."""
    P, Qt, interior = make_panel(seed)
    rng = np.random.default_rng(seed + 1000)
    G = draw(rng, P, Qt, reps=reps)
    Qh = project_fit(G, P)
    ses = np.stack([se_at(G[r], P, Qh[r]) for r in range(reps)])
    spread = Qh.std(axis=0, ddof=1)
    ratio = float(np.median((np.median(ses, axis=0) / spread)[interior]))
    z = (Qh - Qt[None]) / ses
    coverage = float((np.abs(z[:, interior]) < 1.96).mean())
    absent = (Qt == 0) & ~interior[:, None]
    return ratio, coverage, float(np.median(np.median(ses, axis=0)[absent])), float(np.median(spread[absent]))
