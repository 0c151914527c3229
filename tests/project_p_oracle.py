"""numpy restatement of the P step (include/nadm.h, nadm_project_p): one EM step of the binomial admixture model with Q fixed, over
the OBSERVED calls only, and of the alternating loop built from it and the Q step of tests/project_oracle.py.
``p_step(..., dtype=np.float64)`` is the reference of the GPU tests; ``dtype=np.float32`` is the same arithmetic in float32 with the
sums taken over 64-sample slices and the slices' partials added in float64 -- what an fp32 kernel can be expected to reach."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_oracle as R  # noqa: E402

SLICE = 64           # samples per fp32 partial sum of the float32 restatement (= the kernel's tile, csrc/nadm_snp_sweep.h: SWEEP_TILE)
EPS = R.EPS
PMIN = 1e-6


def p_step(Gm, P, Q, eps=EPS, pmin=PMIN, dtype=np.float64):
    """Gm uint8 [b, M] codes (3 = missing), P [M, K], Q [b, K] -> (P_out [M, K] in ``dtype``, n [M]).  den == 0 returns the entry as
    it came."""
    T = np.dtype(dtype).type
    Gm = np.asarray(Gm)
    b, M = Gm.shape
    K = P.shape[1]
    Pd, Qd = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    step = b if dtype == np.float64 else SLICE
    B = np.zeros((M, K), dtype=np.float64)
    Cc = np.zeros((M, K), dtype=np.float64)
    n = np.zeros(M, dtype=np.int64)
    for i0 in range(0, b, step):
        g_raw = Gm[i0:i0 + step]
        obs = g_raw != 3
        g = np.where(obs, g_raw, 0).astype(dtype)
        q = Qd[i0:i0 + step]
        rr = (q @ Pd.T).astype(dtype)
        r = np.clip(rr, T(eps), T(1) - T(eps)).astype(dtype)
        u = np.clip(T(1) - rr, T(eps), T(1) - T(eps)).astype(dtype)      # 1 - r from the UNCLIPPED product
        t1 = np.where(obs, g / r, T(0)).astype(dtype)
        t0 = np.where(obs, (T(2) - g) / u, T(0)).astype(dtype)
        B += (t1.T @ q).astype(dtype)
        Cc += (t0.T @ q).astype(dtype)
        n += obs.sum(axis=0)
    p64 = np.asarray(P, dtype=np.float64)
    num = p64 * B
    den = num + (1.0 - p64) * Cc
    out = p64.copy()
    has = den > 0.0
    out[has] = np.clip(num[has] / den[has], pmin, 1.0 - pmin)
    return out.astype(dtype), n


def loglik(Gm, P, Q, eps=EPS):
    """Log-likelihood of the observed calls summed over the samples, float64 (the ``ll`` of project_oracle.em_step)."""
    return float(R.em_step(Gm, P, Q, eps)[1].sum())


def alternate(Gm, P, Q, rounds, dtype=np.float64, eps=EPS, qmin=R.QMIN, pmin=PMIN):
    """``rounds`` rounds of (Q step with P fixed, P step with the new Q) -> (P, Q, lls): ``lls[0]`` at the start, then one entry per
    HALF round (float64, whatever ``dtype`` the steps run in)."""
    lls = [loglik(Gm, P, Q, eps)]
    for _ in range(rounds):
        Q = R.em_step(Gm, P, Q, eps, qmin, dtype)[0]
        lls.append(loglik(Gm, P, Q, eps))
        P = p_step(Gm, P, Q, eps, pmin, dtype)[0]
        lls.append(loglik(Gm, P, Q, eps))
    return P, Q, np.asarray(lls)


def make_edge_case(N, M, K, seed=5):
    """project_oracle.make_case with its edge cases (rows of P exactly 0 and 1, a one-hot row of Q, an all-missing sample, a 7-call
    sample) and one more: SNP ``dead`` that nobody observes.  -> (Gm, P, Q, dead)."""
    Gm, P, Q = R.make_case(N, M, K, seed=seed)
    dead = 11 if M > 11 else M - 1
    Gm[:, dead] = 3
    return Gm, P, Q, dead


def make_recovery_case(N=130, M=1027, K=3, seed=5, light=0.02, heavy=0.4):
    """Synthetic genotypes of the admixture model with frequencies F [M, K] uniform in [0.05, 0.95] and Dirichlet fractions Q [N, K],
    ``light`` of the calls missing everywhere and ``heavy`` of them at every third SNP; and the fit that reads a missing call as
    genotype 0: thirty float64 P steps on the zero-filled matrix with Q = the truth.
    -> (Gm, F float32, Q float32, P_start float32, heavy SNPs bool [M])."""
    rng = np.random.default_rng(seed)
    F = rng.uniform(0.05, 0.95, size=(M, K)).astype(np.float32)
    Q = rng.dirichlet(0.5 * np.ones(K), size=N).astype(np.float32)
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ F.T.astype(np.float64), 0.0, 1.0)).astype(np.uint8)
    hv = np.zeros(M, dtype=bool)
    hv[::3] = True
    u = rng.random((N, M))
    Gm[(u < light) | ((u < heavy) & hv[None, :])] = 3
    G0 = np.where(Gm == 3, 0, Gm).astype(np.uint8)
    P = np.full((M, K), 0.5)
    for _ in range(30):
        P = p_step(G0, P, Q)[0]
    return Gm, F, Q, P.astype(np.float32), hv


def recovery_figures(P, F, hv):
    """(mean P / F at the heavy SNPs, RMSE of P against F at the heavy SNPs, at the others)."""
    P, F = np.asarray(P, dtype=np.float64), np.asarray(F, dtype=np.float64)
    rm = lambda sel: float(np.sqrt(np.mean((P[sel] - F[sel]) ** 2)))
    return float(np.mean(P[hv] / F[hv])), rm(hv), rm(~hv)
