"""numpy restatement of the projection step (include/nadm.h, nadm_project_q): one EM step of the binomial admixture model with P
fixed, over the OBSERVED calls only.  ``em_step(..., dtype=np.float64)`` is the reference of the GPU tests; ``dtype=np.float32``
is the same arithmetic in float32 with the sums taken in 256-SNP chunks and the chunk partials added in float64 -- what an fp32
kernel can be expected to reach, and the yardstick of the log-likelihood tolerance."""
import numpy as np

CHUNK = 256          # SNPs per chunk of the float32 restatement (= the kernel's PROJ_CHUNK, csrc/nadm_project.hip)
EPS = 1e-6
QMIN = 1e-6


def em_step(Gm, P, Q, eps=EPS, qmin=QMIN, dtype=np.float64):
    """Gm uint8 [b, M] codes (3 = missing), P [M, K], Q [b, K] -> (Q_out [b, K], ll [b] float64 at the INPUT Q, nobs [b])."""
    T = np.dtype(dtype).type
    Gm = np.asarray(Gm)
    b, M = Gm.shape
    K = P.shape[1]
    Pd, Qd = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    step = M if dtype == np.float64 else CHUNK
    a = np.zeros((b, K), dtype=np.float64)
    ll = np.zeros(b, dtype=np.float64)
    n = np.zeros(b, dtype=np.int64)
    for j0 in range(0, M, step):
        g_raw = Gm[:, j0:j0 + step]
        obs = g_raw != 3
        g = np.where(obs, g_raw, 0).astype(dtype)
        p = Pd[j0:j0 + step]
        r = np.clip(Qd @ p.T, T(eps), T(1) - T(eps)).astype(dtype)
        t1 = np.where(obs, g / r, T(0)).astype(dtype)
        t0 = np.where(obs, (T(2) - g) / (T(1) - r), T(0)).astype(dtype)
        a += (t1 @ p + t0 @ (T(1) - p)).astype(dtype)
        term = (g * np.log(r) + (T(2) - g) * np.log(T(1) - r)).astype(dtype)
        ll += np.where(obs, term, T(0)).sum(axis=1, dtype=dtype)
        n += obs.sum(axis=1)
    out = np.asarray(Q, dtype=np.float64).copy()
    has = n > 0
    q1 = np.maximum(np.asarray(Q, dtype=np.float64)[has] * a[has] / (2.0 * n[has, None]), qmin)
    out[has] = q1 / q1.sum(axis=1, keepdims=True)
    ll[~has] = 0.0
    return out.astype(dtype), ll, n


def iterate(Gm, P, Q, iters, dtype=np.float64, eps=EPS, qmin=QMIN):
    """``iters`` steps -> (Q after them, lls [iters, b]: ll at the input of every step)."""
    lls = []
    for _ in range(iters):
        Q, ll, _ = em_step(Gm, P, Q, eps, qmin, dtype)
        lls.append(ll)
    return Q, np.asarray(lls)


def make_case(N, M, K, seed=5, missing=0.05, edge=True):
    """oracle.nadm_oracle.synth_genotypes(N, M, K, seed, missing) together with the allele frequencies it was drawn from (the same
    first draw of the same stream) as P [M, K], and a Dirichlet start Q [N, K].  ``edge``: P gets rows of exact 0 and exact 1, Q row 2
    is one-hot, row 4 is all missing, row 5 keeps 7 observed calls; otherwise P is clipped to [0.02, 0.98] (no clip of r is active)."""
    from oracle import nadm_oracle as O
    Gm = O.synth_genotypes(N, M, K, seed=seed, missing=missing)
    Fq = np.clip(0.5 * np.random.default_rng(seed).beta(0.5, 0.5, size=(K, M)), 0.005, 0.5)
    rng = np.random.default_rng(seed + 1000)
    P = Fq.T.astype(np.float32).copy()
    Q = rng.dirichlet(np.ones(K), size=N).astype(np.float32)
    if edge:
        P[3::97] = 0.0
        P[7::89] = 1.0
        if N > 2:
            Q[2] = 0.0
            Q[2, K - 1] = 1.0
        if N > 5:
            Gm[4] = 3
            keep = rng.choice(M, size=7, replace=False)
            row = Gm[5].copy()
            Gm[5] = 3
            Gm[5, keep] = row[keep] % 3
    else:
        P = np.clip(P, 0.02, 0.98)
    return Gm, P, Q
