"""Float64 numpy restatement of the IBD-sharing sums given ancestry (PC-Relate's k2 and k0 estimators with the admixture model's
individual-specific frequencies; include/nadm.h, nadm_ibd) from UNPACKED genotypes.

    pi_ij  = sum_k q_ik p_jk                m_ij: kinship_oracle.terms' own mask (observed and pimin <= pi <= 1 - pimin)
    v_ij   = pi (1 - pi)
    gD_ij  = pi if g = 0;  0 if g = 1;  1 - pi if g = 2
    e_ij   = m (gD - v (1 + f_i))           vm_ij = m v
    u_ij   = m pi^2                         w_ij  = m (1 - pi)^2
    z0_ij  = m [g = 0]                      z2_ij = m [g = 2]
    mag_ij = m (|gD| + v (1 + |f_i|))       the un-cancelled magnitude of e
    k2num_ab = sum_j e_a e_b    k2den_ab = sum_j vm_a vm_b    ibs0_ab = sum_j (z0_a z2_b + z2_a z0_b)
    exp0_ab  = sum_j (u_a w_b + w_a u_b)    abs2_ab = sum_j mag_a mag_b
    k2 = k2num / k2den (NaN where k2den = 0);  k0 = ibs0 / exp0 if phi >= 2^-2.5 (NaN where exp0 = 0) else 1 - 4 phi + k2;  k1 = 1 - k0 - k2

The mask comes from ``kinship_oracle.terms`` (the float32 bounds the library compares against, and its guard that no pi lies within
1e-5 of a bound).  ``f`` is the float32 vector the library gets, widened; where a sample's every call is masked its f does not matter
(a NaN there is replaced before the arithmetic: numpy's where would otherwise carry 0 * NaN warnings, not values).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kinship_oracle as KO  # noqa: E402

FIRST_DEGREE = 2.0 ** -2.5


def terms(G, P, Q, f, pimin=0.0):
    """Per (sample, SNP): e, vm, u, w (float64), z0, z2 (bool) and mag (float64) for genotypes G [N, M] (0, 1, 2; 3 = missing),
    P [M, K], Q [N, K] and the inbreeding coefficients f [N]."""
    G = np.asarray(G)
    _, _, m = KO.terms(G, P, Q, pimin)
    pi = np.asarray(Q, dtype=np.float32).astype(np.float64) @ np.asarray(P, dtype=np.float32).astype(np.float64).T
    f64 = np.asarray(f, dtype=np.float32).astype(np.float64)
    f64 = np.where(m.any(axis=1), f64, 0.0)[:, None]            # (the f of a sample without a counted call multiplies nothing)
    v = pi * (1.0 - pi)
    gd = np.where(G == 0, pi, np.where(G == 2, 1.0 - pi, 0.0))
    e = np.where(m, gd - v * (1.0 + f64), 0.0)
    vm = np.where(m, v, 0.0)
    u = np.where(m, pi * pi, 0.0)
    w = np.where(m, (1.0 - pi) * (1.0 - pi), 0.0)
    z0, z2 = m & (G == 0), m & (G == 2)
    mag = np.where(m, np.abs(gd) + v * (1.0 + np.abs(f64)), 0.0)
    return e, vm, u, w, z0, z2, mag


def from_terms(tA, tB):
    """(k2num, k2den, ibs0, exp0, abs2) of the samples of tA against the samples of tB (each a ``terms`` result, possibly gathered)."""
    eA, vA, uA, wA, z0A, z2A, gA = tA
    eB, vB, uB, wB, z0B, z2B, gB = tB
    f8 = np.float64
    k2num = eA @ eB.T
    k2den = vA @ vB.T
    ibs0 = (z0A.astype(f8) @ z2B.astype(f8).T + z2A.astype(f8) @ z0B.astype(f8).T).astype(np.int64)
    exp0 = uA @ wB.T + wA @ uB.T
    abs2 = gA @ gB.T
    return k2num, k2den, ibs0, exp0, abs2


gather = KO.gather


def ibd_of(phi, k2num, k2den, ibs0, exp0):
    """(k0, k1, k2) float64, NaN rules as in the module docstring."""
    phi = np.asarray(phi, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k2 = np.where(k2den != 0, k2num / k2den, np.nan)
        k0 = np.where(phi >= FIRST_DEGREE, np.where(exp0 != 0, ibs0 / exp0, np.nan), 1.0 - 4.0 * phi + k2)
    return k0, 1.0 - k0 - k2, k2


def ibd(G, P, Q, f, phi, pimin=0.0):
    """All pairs of the samples of G: (k0, k1, k2) and the five sums."""
    t = terms(G, P, Q, f, pimin)
    s = from_terms(t, t)
    return ibd_of(phi, *s[:4]), s
