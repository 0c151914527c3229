"""The model-fit check (nadm_em_sums, nadm_resid_cor, fitcheck.em_sums / resid_cor_block / resid_cor / group_means / sample_means /
fit_check, Engine.resid_cor, the `fit` mode of the command line and `train --fit_check`).  The float64 numpy restatement, the shared
panels and the calibration panels live in tests/fitcheck_oracle.py.

TOLERANCES (u = 2^-24, the unit round-off of fp32).

nadm_em_sums against float64:  |B - B64| <= 2^-20 B64 and the same for C (every term is >= 0, so B64 is its own sum of magnitudes).
A term is fma(q, g * rcp(r), sum): r = clip(rr) with rr from K fused multiply-adds (relative error growing like sqrt(K) u for
round-offs of either sign, K u at worst), a 1-ulp reciprocal (2 u), one product (u) and the multiply-add (u); the fp32 sum runs over
at most 64 x 64 samples of a slice, whose round-offs average out over the samples.  16 u = 2^-20 covers a term (4 u + sqrt(16) u)
with a factor 2; it presumes frequencies away from 0 and 1 (the panels' P is in [0.05, 0.95]): u = 1 - rr cancels, and its relative
error is rr / (1 - rr) times that of rr.

nadm_resid_cor against the float64 oracle ON THE SAME fp32 B AND C:  n equal, and (the form the issue states)
    |S  - S64|  <= 2^-15 sum_j |d_a d_b|   + 2^-17 sum_j o_a o_b (|d_a| + |d_b|)
    |Ta - Ta64| <= 2^-15 sum_j d_a^2 o_b   + 2^-16 sum_j o_a o_b |d_a|
    |Tb - Tb64| <= 2^-15 sum_j d_b^2 o_a   + 2^-16 sum_j o_a o_b |d_b|
The first term is test_kinship's: a product (u) and the fp32 accumulation over the SNPs of a range (at most 4100 here: a random walk
of sqrt(4100) u = 64 u against 2^-15 = 512 u).  The second is the error of a residual, which does not shrink with the residual
because g - 2 pi cancels: beta and gamma are formed by the operations of the sums' terms, 8 u = 2^-21 relative (the 4 u + sqrt(16) u
above, which 2^-20 covers with a factor 2); the refit is kept only while den' >= den / 8, so a perturbation of B - beta or C - gamma
reaches f = num' / den' amplified by at most 8: |f - f64| <= 2^-18 (f <= 1); pi = sum_k q_k f_k with sum_k q_k = 1 carries that
through; d = g - 2 pi doubles it: |d - d64| <= 2^-17.  S takes it once per factor, d^2 twice (2 |d| 2^-17).  Every case prints its
largest ratio to the bound before it asserts.
OBSERVED on an MI355X: the largest error is 0.07 % .. 2 % of these bounds over BLOCKS and the two-range case (S 1.1e-2, Ta 2.1e-2, Tb
1.4e-2 of the bound at most), the sums 9e-9 .. 4.5e-7 relative against 2^-20 = 9.5e-7; see DESIGN.md section 4.15.
The branch of the refit cannot differ between the two sides: the oracle asserts that no (b, j, k) lies within 2^-10 of the threshold.

CALIBRATION of the statistic on the oracle (float64, CPU), measured with the committed seeds:
    panel 1 (seed 1): naive within-population mean -0.0398; corrected within -0.0068, between +0.0031; sd over pairs 0.01504 against
                      1 / sqrt(median n_ab) = 0.01360 (ratio 1.106)
    panel 2 (seed 1): corrected within-means -0.0002, -0.0002 (well modelled), +0.1052, +0.1057 (merged); between the merged -0.1016
"""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitcheck_oracle as FO  # noqa: E402
import ld_oracle as LO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

ROWS = 140                   # resident rows of the GPU cases: the fit the sums run over
TOL_SUMS = 2.0 ** -20
TOL_ACC, TOL_D = 2.0 ** -15, 2.0 ** -17
SUMS_CASES = [(70, 515, 3), (1, 1, 1), (130, 257, 9), (65, 1030, 16)]
# (ba, bb, M, K, lists): "perm" = two different permutations of the resident rows with the planted ones in them, "few" = short lists
# that overlap, one with a duplicate
BLOCKS = [(70, 70, 515, 3, "perm"), (1, 1, 1, 1, "perm"), (64, 65, 256, 8, "perm"), (33, 130, 257, 9, "perm"), (5, 3, 4100, 16, "few")]


# ------------------------------------------------------------------------------------------------ CPU: the oracle by hand
def test_oracle_on_a_case_worked_out_by_hand():
    """Two samples, three SNPs, K = 1, Q = 1, P = (1/2, 1/4, 1/2); g_a = 2, 1, missing; g_b = 0, 1, 2.  K = 1: rr = p.
        B = sum g / p:          4 + 0 = 4,   4 + 4 = 8,      4 (b alone)
        C = sum (2 - g) / (1 - p):  0 + 4 = 4,   4/3 + 4/3 = 8/3,   0
        den = p B + (1 - p) C = 4, 4, 2.
    Without b:  SNP 0: beta = 0, gamma = 4: num' = 2, den' = 2 >= 4/8: f = 1.     d_a = 2 - 2 = 0,   d_b = 0 - 2 = -2
                SNP 1: beta = 4, gamma = 4/3: num' = 1, den' = 1 + 1 = 2: f = 1/2.  d_a = 1 - 1 = 0,   d_b = 1 - 1 = 0
                SNP 2: beta = 4, gamma = 0: num' = den' = 0 < 2/8: f = p = 1/2.    d_a = 0 (missing), d_b = 2 - 1 = 1
      column b:  S_ab = 0, Ta_ab = 0, Tb_ab = 4 + 0 = 4 (SNP 2: a is missing), n_ab = 2;  S_bb = Ta_bb = Tb_bb = 5, n_bb = 3.
    Without a:  SNP 0: beta = 4, gamma = 0: num' = 0, den' = 0 + 2 = 2: f = 0.    d_a = 2,  d_b = 0
                SNP 1: f = 1/2 as above (b alone, g = 1).                          d_a = 0,  d_b = 0
                SNP 2: a is missing: nothing enters the pair.
      column a:  S_aa = Ta_aa = Tb_aa = 4, n_aa = 2;  S_ba = 0, Ta_ba = 0, Tb_ba = 4, n_ba = 2.
    With two samples the refit without one IS the other's genotype, so the other's residual is 0: c_ab has no value (Ta = 0).
    Three samples, one SNP, p = 1/2, g = (2, 1, 0): B = C = 6, den = 6; without the third: beta = 0, gamma = 4, num' = 3, den' = 3 +
    1 = 4, f = 3/4: d = (1/2, -1/2, -3/2); S = (-3/4, +3/4), Ta = (1/4, 1/4), Tb = 9/4: c = -1 and +1."""
    Gm = np.asarray([[2, 1, 3], [0, 1, 2]], dtype=np.uint8)
    Q = np.ones((2, 1), dtype=np.float32)
    P = np.asarray([[0.5], [0.25], [0.5]], dtype=np.float32)
    B, C = FO.em_sums(Gm, P, Q)
    assert np.allclose(B[:, 0], [4, 8, 4], rtol=1e-15) and np.allclose(C[:, 0], [4, 8 / 3, 0], rtol=1e-15)
    f_b, take_b = FO.loo_freq(np.asarray([0.0, 1.0, 2.0]), np.ones(3, dtype=bool), np.ones(1), P.astype(np.float64), B, C)
    assert np.allclose(f_b[:, 0], [1.0, 0.5, 0.5], rtol=1e-15) and take_b[:, 0].tolist() == [True, True, False]
    r = FO.resid_cor_block(Gm, Gm, P, Q, Q, B, C)
    assert np.allclose(r["S"], [[4, 0], [0, 5]], atol=1e-14) and np.allclose(r["Ta"], [[4, 0], [0, 5]], atol=1e-14)
    assert np.allclose(r["Tb"], [[4, 4], [4, 5]], atol=1e-14) and np.array_equal(r["n"], [[2, 2], [2, 3]])
    assert r["fallbacks"] == 1
    c = FO.cor_of(r["S"], r["Ta"], r["Tb"])
    assert np.isnan(c[0, 1]) and np.isnan(c[1, 0]) and c[0, 0] == 1.0 and c[1, 1] == 1.0
    cor, n = FO.resid_cor(Gm, P, Q)
    assert np.isnan(cor).all() and np.array_equal(n, [[2, 2], [2, 3]])
    G3, Q3, P3 = np.asarray([[2], [1], [0]], dtype=np.uint8), np.ones((3, 1), dtype=np.float32), np.asarray([[0.5]], dtype=np.float32)
    B3, C3 = FO.em_sums(G3, P3, Q3)
    assert B3[0, 0] == 6.0 and C3[0, 0] == 6.0
    r3 = FO.resid_cor_block(G3[:2], G3[2:], P3, Q3[:2], Q3[2:], B3, C3)
    assert np.allclose(r3["S"][:, 0], [-0.75, 0.75], atol=1e-15) and np.allclose(r3["Ta"][:, 0], [0.25, 0.25], atol=1e-15)
    assert np.allclose(r3["Tb"][:, 0], [2.25, 2.25], atol=1e-15) and np.allclose(FO.cor_of(r3["S"], r3["Ta"], r3["Tb"])[:, 0], [-1.0, 1.0], atol=1e-15)


def test_missing_calls_and_other_p_where_nobody_observes_do_not_enter_the_oracle():
    Gm, P, Q = FO.make_panel(20, 40, 3)
    B, C = FO.em_sums(Gm, P, Q)
    assert (B[3] == 0).all() and (C[3] == 0).all() and (Gm[1] == 3).all()
    r = FO.resid_cor_block(Gm, Gm, P, Q, Q, B, C)
    assert not r["n"][1].any() and not r["n"][:, 1].any() and not r["S"][1].any() and not r["Ta"][:, 1].any() and not r["Tb"][1].any()
    P2 = P.copy()
    P2[3] = 0.123
    r2 = FO.resid_cor_block(Gm, Gm, P2, Q, Q, B, C)
    assert all(np.array_equal(r[k], r2[k]) for k in ("S", "Ta", "Tb", "n"))
    assert r["fallbacks"] >= (Gm[2] != 3).sum()                 # sample 2 alone carries the last component: its own refit falls back


# ------------------------------------------------------------------------------------------------ CPU: calibration on the oracle
@functools.lru_cache(maxsize=None)
def _panel1():
    Gm, P, Q, pop = FO.panel_admixed(1)
    return Gm, P, Q, pop, FO.naive_cor(Gm, P, Q), FO.resid_cor(Gm, P, Q)


def _pooled(cor, pop, K, within):
    parts = [FO.pair_means(cor, pop, x, y) for x in range(K) for y in range(x, K) if (x == y) == within]
    return sum(m * k for m, _, k in parts) / sum(k for _, _, k in parts)


def test_calibration_panel_1_the_correction_removes_the_own_genotype_bias():
    """96 x 6000, K = 3, Fst 0.1, 5 % missing, about 30 % admixed, 200 rounds of joint block EM from the truth (seed 1).
    MEASURED: naive within-population mean -0.0398, between +0.0030; corrected within -0.0068, between +0.0031; standard deviation
    over all pairs 0.01504 against 1 / sqrt(median n_ab) = 0.01360."""
    Gm, P, Q, pop, naive, (cor, n) = _panel1()
    assert Gm.shape == (96, 6000) and 0.2 < (pop < 0).mean() < 0.4 and 0.04 < (Gm == 3).mean() < 0.06
    nw, nb = _pooled(naive, pop, 3, True), _pooled(naive, pop, 3, False)
    cw, cb = _pooled(cor, pop, 3, True), _pooled(cor, pop, 3, False)
    iu = np.triu_indices(96, 1)
    sd, want_sd = float(np.nanstd(cor[iu])), 1.0 / np.sqrt(np.median(n[iu]))
    print(f"panel 1: naive within {nw:+.4f} between {nb:+.4f}; corrected within {cw:+.4f} between {cb:+.4f}; sd {sd:.5f} against {want_sd:.5f}")
    assert nw <= -0.025
    assert abs(cw) <= 0.01 and abs(cb) <= 0.01
    assert sd <= 1.25 * want_sd
    assert np.array_equal(cor, cor.T, equal_nan=True) and np.isnan(np.diagonal(cor)).all()


def test_calibration_panel_2_merged_populations_stand_out():
    """Four unadmixed populations fitted with K = 3, the last two sharing a component (seed 1).
    MEASURED: within-means -0.0002, -0.0002, +0.1052, +0.1057; between the two merged ones -0.1016."""
    Gm, P, Q, pop = FO.panel_merged(1)
    cor, n = FO.resid_cor(Gm, P, Q)
    w = [FO.pair_means(cor, pop, x, x)[0] for x in range(4)]
    b23 = FO.pair_means(cor, pop, 2, 3)[0]
    print("panel 2: within " + " ".join(f"{v:+.4f}" for v in w) + f"; between the merged {b23:+.4f}")
    assert w[2] >= 0.05 and w[3] >= 0.05 and b23 <= -0.05
    assert abs(w[0]) <= 0.01 and abs(w[1]) <= 0.01
    from neural_admixture_amd import fitcheck
    means, counts, groups = fitcheck.group_means(cor, pop)
    assert groups == [0, 1, 2, 3] and np.allclose(np.diagonal(means), w, atol=1e-15) and abs(means[2, 3] - b23) < 1e-15
    assert counts[0, 0] == 24 * 23 // 2 and counts[2, 3] == 24 * 24


# ------------------------------------------------------------------------------------------------ CPU: host-side checks
def test_header_states_the_fallback_constant_and_the_library_exports_the_symbols():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_em_sums", "nadm_em_sums_slices", "nadm_em_sums_scratch_floats", "nadm_resid_cor", "nadm_resid_cor_ranges",
                 "nadm_resid_cor_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "#define NADM_LOO_MIN_SHARE 0.125f" in header and "den' >= NADM_LOO_MIN_SHARE * den" in header
    assert "#define NADM_RESID_COR_MAX_ROWS 4096" in header and FO.MIN_SHARE == 0.125
    build = open(os.path.join(root, "neural-admixture_amd", "csrc", "build.sh")).read()
    assert "nadm_resid_cor.hip" in build and build.count("nadm_resid_cor.o") >= 2


def test_ranges_and_scratch_are_rules_of_the_shape():
    from neural_admixture_amd._lib import lib
    rg, f = lib.nadm_resid_cor_ranges, lib.nadm_resid_cor_scratch_floats
    for kp in (4, 8, 12, 16):
        gb = 3 if kp == 16 else 4
        for ba, bb in ((1, 1), (70, 70), (33, 130), (1024, 1024), (4096, 4096), (257, 5)):
            for M in (1, 257, 4100, 500000, 600000):
                r, chunks = int(rg(ba, bb, M, kp)), (M + 255) // 256
                assert 1 <= r <= chunks and -(-chunks // r) <= 1024                 # one fp32 sum: at most 2^18 SNPs
                tiles = -(-ba // 256) * -(-bb // gb)
                assert int(f(ba, bb, M, kp)) >= r * tiles * 256 * gb * 4
        v = [int(f(1024, 1024, M, kp)) for M in (1, 257, 4100, 500000, 600000)]
        assert all(y >= x for x, y in zip(v, v[1:]))
        # bounded by ranges x ba x bb, never per chunk: a 1024 x 1024 block at 600k SNPs stays far below a GB
        assert int(f(1024, 1024, 600000, kp)) * 4 <= 64 * 1024 ** 2 and int(rg(1024, 1024, 600000, kp)) == 3
    assert int(rg(70, 70, 257, 4)) >= 2
    for bad in ((0, 5, 100, 4), (5, 0, 100, 4), (4097, 5, 100, 4), (5, 4097, 100, 4), (5, 5, 0, 4), (5, 5, 100, 20), (5, 5, 100, 24), (5, 5, 100, 0)):
        assert int(rg(*bad)) == 0 and int(f(*bad)) == 0
    sl, fs = lib.nadm_em_sums_slices, lib.nadm_em_sums_scratch_floats
    for b, M in ((1, 1), (70, 515), (4200, 257), (32768, 500000)):
        assert int(sl(b, M)) == int(lib.nadm_project_p_slices(b, M))
        assert int(fs(b, M, 8)) == int(lib.nadm_project_p_scratch_floats(b, M, 8)) > 0
    assert int(sl(0, 5)) == 0 and int(fs(5, 0, 4)) == 0


def _refusal_args():
    xp = torch.zeros((8, 16), dtype=torch.uint8)
    Q = torch.full((8, 24), 0.25)
    P, B, C = (torch.full((50, 24), 0.25) for _ in range(3))
    S, Ta, Tb = (torch.empty(8 * 8, dtype=torch.float64) for _ in range(3))
    n = torch.empty(8 * 8, dtype=torch.int32)
    scratch = torch.empty(1 << 16)
    keep = (xp, Q, P, B, C, S, Ta, Tb, n, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idxA=None, ba=8, idxB=None, bb=8, M=50, P=P.data_ptr(), k=3, kp=4, QA=Q.data_ptr(), QB=Q.data_ptr(),
             q_stride=24, B=B.data_ptr(), C=C.data_ptr(), eps=1e-6, S=S.data_ptr(), Ta=Ta.data_ptr(), Tb=Tb.data_ptr(), n=n.data_ptr(),
             scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(B=None), "null pointer"), (dict(C=None), "null pointer"), (dict(S=None), "null pointer"),
    (dict(Tb=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(ba=0), "empty block"), (dict(bb=-1), "empty block"), (dict(M=0), "empty block"),
    (dict(bb=4097), "must be <= NADM_RESID_COR_MAX_ROWS"), (dict(ba=5000), "must be <= NADM_RESID_COR_MAX_ROWS"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"),
    (dict(kp=20), "kp must be nadm_pad_k(k)"), (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=17, kp=24), "K must be <= 16"),
    (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(unaligned="xp"), "16-byte aligned"), (dict(unaligned="P"), "16-byte aligned"), (dict(unaligned="B"), "16-byte aligned"),
    (dict(unaligned="QB"), "16-byte aligned"), (dict(unaligned="scratch"), "16-byte aligned"), (dict(unaligned="S"), "8-byte"),
    (dict(unaligned2="n"), "4-byte"),
])
def test_resid_cor_refuses_before_any_launch(change, message):
    """Every refusal of nadm_resid_cor is decided on the host: it is reported with its message on a machine without a GPU (where a
    launch would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "unaligned2" in change:
        a[change["unaligned2"]] += 2
    else:
        a.update(change)
    status = lib.nadm_resid_cor(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_resid_cor"):
        check(status, "resid_cor")
    del keep


def test_em_sums_refuses_before_any_launch():
    from neural_admixture_amd._lib import lib
    xp, Q = torch.zeros((4, 16), dtype=torch.uint8), torch.full((4, 8), 0.25)
    P, B, C = (torch.full((50, 4), 0.25) for _ in range(3))
    scratch = torch.empty(4096)
    base = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, Q=Q.data_ptr(), q_stride=8, k=3, kp=4, P=P.data_ptr(), eps=1e-6, B=B.data_ptr(),
                C=C.data_ptr(), nobs=None, scratch=scratch.data_ptr(), stream=None)
    for change, message in ((dict(B=None), "null pointer"), (dict(b=0), "empty batch"), (dict(ld=24), "multiple of 16"),
                            (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(eps=0.7), "eps must be in"),
                            (dict(C=C.data_ptr() + 4), "16-byte aligned"), (dict(q_stride=2), "q_stride < kp")):
        assert lib.nadm_em_sums(*dict(base, **change).values()) != 0 and message in lib.nadm_last_error().decode()


def test_python_layer_refuses_in_words():
    from neural_admixture_amd import fitcheck
    xp = torch.zeros((4, 16), dtype=torch.uint8)                     # (a CPU tensor: the refusals come before it is looked at)
    with pytest.raises(RuntimeError, match="K must be <= 16 for the fit check"):
        fitcheck.resid_cor(xp, 50, np.full((50, 17), 0.5, dtype=np.float32), np.full((4, 17), 1 / 17, dtype=np.float32))
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match=r"rows must be in 1\.\.4096"):
            fitcheck.resid_cor(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None, rows=rows)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        fitcheck.resid_cor(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        fitcheck.em_sums(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None)


def test_group_means_and_sample_means_skip_nan():
    from neural_admixture_amd import fitcheck
    nan = float("nan")
    cor = np.asarray([[nan, 0.2, 0.4, -0.1],
                      [0.2, nan, nan, 0.3],
                      [0.4, nan, nan, 0.5],
                      [-0.1, 0.3, 0.5, nan]])
    means, counts, groups = fitcheck.group_means(cor, ["x", "x", "y", "y"])
    assert groups == ["x", "y"]
    assert np.allclose(means, [[0.2, (0.4 - 0.1 + 0.3) / 3], [(0.4 - 0.1 + 0.3) / 3, 0.5]], atol=1e-15)
    assert np.array_equal(counts, [[1, 3], [3, 1]])
    means, counts, groups = fitcheck.group_means(torch.from_numpy(cor), np.asarray([2, 1, 1, 3]), groups=[1, 2, 3, 4])
    assert np.isnan(means[0, 0]) and counts[0, 0] == 0 and abs(means[0, 1] - 0.3) < 1e-15 and np.isnan(means[1, 1]) and abs(means[0, 2] - 0.4) < 1e-15
    assert np.isnan(means[3]).all() and not counts[3].any() and np.array_equal(means, means.T, equal_nan=True)
    m, n = fitcheck.sample_means(cor)
    assert np.allclose(m, [0.5 / 3, 0.25, 0.45, 0.7 / 3], atol=1e-15) and np.array_equal(n, [3, 2, 2, 3])
    m, n = fitcheck.sample_means(np.full((2, 2), nan))
    assert np.isnan(m).all() and not n.any()
    with pytest.raises(RuntimeError, match="labels"):
        fitcheck.group_means(cor, ["x", "y"])
    lab, names = fitcheck.default_labels(np.asarray([[0.1, 0.9], [0.6, 0.4], [0.5, 0.5]]))
    assert lab.tolist() == ["2", "1", "1"] and names == ["1", "2"]


def test_writers_and_log_lines(tmp_path, caplog):
    from neural_admixture_amd import fitcheck
    nan = float("nan")
    cor = torch.tensor([[nan, 0.2, -0.1], [0.2, nan, 0.3], [-0.1, 0.3, nan]], dtype=torch.float64)
    labels = np.asarray(["b", "b", "a"])
    means, counts, groups = fitcheck.group_means(cor, labels)
    sm, sn = fitcheck.sample_means(cor)
    r = fitcheck.FitResult(2, cor, torch.ones((3, 3), dtype=torch.int32), groups, np.asarray([1, 1, 0]), means, counts, sm, sn, 5e-3)
    fitcheck.write_results(tmp_path, "run", [r], matrix=True)
    pop = (tmp_path / "run.2.cor_pop").read_text().splitlines()
    assert pop[0] == "a b" and pop[1].split() == ["nan", "0.10000000"] and pop[2].split() == ["0.10000000", "0.20000000"]
    smp = (tmp_path / "run.2.cor_sample").read_text().splitlines()
    assert smp == ["0.05000000 2", "0.25000000 2", "0.10000000 2"]
    back = np.loadtxt(tmp_path / "run.2.cor", dtype=np.float32, ndmin=2)
    assert np.array_equal(back, cor.numpy().astype(np.float32), equal_nan=True)
    caplog.set_level(logging.INFO)
    fitcheck.log_results([r], logging.getLogger("fit"), warn=0.15)
    msgs = [x.getMessage() for x in caplog.records]
    assert any(m.startswith("Fit check (K=2): mean residual correlation within groups 0.2000, between groups 0.1000; largest |group mean| 0.2000") for m in msgs)
    assert any("group b: mean correlation +0.2000 over 1 pairs (positive within a group: unmodelled structure or relatedness there)" in m for m in msgs)
    assert not any("groups a and b" in m for m in msgs)
    assert any("not at the fixed point of its own EM step" in m and "train --polish" in m for m in msgs)
    caplog.clear()
    fitcheck.log_results([r._replace(means=-means, em_gap=1e-5)], logging.getLogger("fit"), warn=0.05)
    msgs = [x.getMessage() for x in caplog.records]
    assert any("groups a and b: mean correlation -0.1000 over 2 pairs (negative between groups: they share a component they should not)" in m for m in msgs)
    assert not any("fixed point" in m for m in msgs)


def test_cli_fit_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing or misshapen files end the run with the offender named, before the GPU check and before a genotype
    is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["fit", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_fit_args(base[1:] + ["--k", "3"])
    assert (a.k, a.pops_path, a.subsample, a.seed, a.matrix, a.warn, a.out_name, a.threads, a.extract) == (3, None, 0, 42, False, 0.02, None, 1, None)
    a = cli.parse_fit_args(base[1:] + ["--min_k", "2", "--max_k", "4", "--pops_path", "p", "--subsample", "100", "--seed", "7", "--matrix", "--warn", "0.05",
                                      "--out_name", "o", "--threads", "4", "--extract", "f"])
    assert (a.min_k, a.max_k, a.pops_path, a.subsample, a.seed, a.matrix, a.warn, a.out_name, a.threads, a.extract) == (2, 4, "p", 100, 7, True, 0.05, "o", 4, "f")
    assert "fit" in cli._ANALYSIS_MODES

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    for ks in (["--k", "17"], ["--min_k", "15", "--max_k", "17"]):
        with pytest.raises(SystemExit, match=r"fit needs every K <= 16.*K = 17 was asked for"):
            cli.main(base + ks)
    for value in ("4097", "1", "-5"):
        with pytest.raises(SystemExit, match=r"--subsample must be in 2\.\.4096"):
            cli.main(base + ["--k", "3", "--subsample", value])
    for value in ("-0.1", "nan"):
        with pytest.raises(SystemExit, match=r"--warn must be >= 0"):
            cli.main(base + ["--k", "3", "--warn", value])
    with pytest.raises(SystemExit, match=r"nopops not found"):
        cli.main(base + ["--k", "3", "--pops_path", str(tmp_path / "nopops")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen"), "--k", "3"])
    with pytest.raises(SystemExit, match=r"fit needs the .*run\.3\.P not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    bed.write_bytes(bytes(3 + 2 * 9))                        # N = 5, M = 9
    (tmp_path / "pops").write_text("a\nb\na\nb\n")          # four labels for five samples
    with pytest.raises(SystemExit, match=r"pops lists 4 labels, the data holds 5 samples"):
        cli.main(base + ["--k", "3", "--pops_path", str(tmp_path / "pops")])
    (tmp_path / "pops").write_text("a\nb\na\nb\na\n")
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + ["--k", "3", "--pops_path", str(tmp_path / "pops")])
    # more than 4096 samples: the run ends naming --subsample; with it the GPU check is what is left
    big = tmp_path / "big.bed"
    (tmp_path / "big.fam").write_text("\n".join(["s"] * 4100) + "\n")
    big.write_bytes(bytes(3 + 1025 * 9))
    np.savetxt(tmp_path / "run.3.Q", np.full((4100, 3), 1 / 3))
    bigargs = ["fit", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(big), "--k", "3"]
    with pytest.raises(SystemExit, match=r"holds 4100: pass --subsample S with S <= 4096"):
        cli.main(bigargs)
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(bigargs + ["--subsample", "500"])
    assert not list(tmp_path.glob("*.cor_pop"))


def test_train_fit_check_refuses_sharded_and_supervised_runs(tmp_path, monkeypatch):
    """`train --fit_check`: the refusals and the wording of --p_se, before the GPU check; the keyword of train() likewise."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["train", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "x.bed"), "--k", "3", "--fit_check"]
    assert cli.parse_train_args(base[1:]).fit_check is True and cli.parse_train_args(base[1:-1]).fit_check is False
    with pytest.raises(SystemExit, match=r"--fit_check is single-GPU: run it with --num_gpus 1"):
        cli.main(base + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--fit_check ignores labels: it is not available with --pops_path"):
        cli.main(base + ["--pops_path", str(tmp_path / "pops")])
    with pytest.raises(SystemExit, match=r"--fit_check needs every K <= 16"):
        cli.main(base[:-3] + ["--min_k", "15", "--max_k", "17", "--fit_check"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(base)
    G0, V0 = torch.zeros((4, 100), dtype=torch.uint8), np.zeros((8, 100), np.float32)
    with pytest.raises(ValueError, match="fit_check needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 2, 16, True, V0, None, fit_check=True)
    with pytest.raises(ValueError, match="fit_check needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 1, 16, True, V0, ["a", "b", "c", "a"], fit_check=True)
    with pytest.raises(ValueError, match="fit_check needs every K <= 16"):
        na.train(1, 8, 1e-3, 17, 0, G0, torch.device("cpu"), 1, 16, True, V0, None, fit_check=True)


def test_sharded_and_cpu_engines_refuse_and_public_names():
    import neural_admixture_amd as na
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.resid_cor is single-GPU"):
        e.resid_cor()
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.resid_cor needs the HIP engine with its packed matrix resident"):
        e.resid_cor()
    for name in ("resid_cor", "em_sums", "fit_check", "group_means", "sample_means"):
        assert callable(getattr(na, name)) and name in na.__all__


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _panel(M, K):
    """ROWS resident rows with the planted cases of fitcheck_oracle.make_panel; the tests leave them as they are."""
    return FO.make_panel(ROWS, M, K)


def _rows(b, seed):
    """b of the resident rows, out of order: the all-missing row 1 and row 2, which alone carries the last component, among them
    (b >= 3), the last entry a duplicate of the first (b >= 4)."""
    if b < 3:
        return np.asarray([5, 9][:b], dtype=np.int32)
    perm = np.random.default_rng(seed).permutation(ROWS)
    perm = np.concatenate([[1, 2], perm[(perm != 1) & (perm != 2)]])[:b]
    perm = perm[np.random.default_rng(seed + 1).permutation(b)]
    if b >= 4:
        perm[-1] = perm[0]
    return perm.astype(np.int32)


def _lists(ba, bb, kind):
    if kind == "few":
        return np.asarray([2, 7, 1, 9, 7][:ba], dtype=np.int32), np.asarray([9, 2, 30][:bb], dtype=np.int32)
    return _rows(ba, 10 * ba + bb), _rows(bb, 10 * bb + ba + 500)


def _device_sums(M, K):
    """(xp, Pp, Qp, B, C) on the device: the sums over ALL resident rows."""
    from neural_admixture_amd import fitcheck
    from neural_admixture_amd._packed import pad_P, pad_Q
    dev = _dev()
    Gm, P, Q = _panel(M, K)
    xp = _packed(Gm).to(dev)
    Pp = pad_P(P, dev)
    Qp = pad_Q(Q, ROWS, K, int(Pp.shape[1]), dev)
    B, C = fitcheck.em_sums(xp, M, P, Q)
    return xp, Pp, Qp, B, C


def _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib):
    from neural_admixture_amd import fitcheck
    dev = xp.device
    ta, tb = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
    out = fitcheck.resid_cor_block(xp, M, Pp, K, ta, Qp[ta.long()].contiguous(), tb, Qp[tb.long()].contiguous(), B, C)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_block(got, want, what):
    """n equal; the three sums within the bounds of the module docstring; prints the largest ratio to the bound before it asserts."""
    S, Ta, Tb, n = got
    assert S.dtype == np.float64 and n.dtype == np.int32 and S.shape == want["S"].shape
    bounds = {"S": TOL_ACC * want["absS"] + TOL_D * want["linS"], "Ta": TOL_ACC * want["Ta"] + 2 * TOL_D * want["linTa"],
              "Tb": TOL_ACC * want["Tb"] + 2 * TOL_D * want["linTb"]}
    ratios = {}
    for name, val in (("S", S), ("Ta", Ta), ("Tb", Tb)):
        err = np.abs(val - want[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratios[name] = float(np.max(np.where(bounds[name] > 0, err / bounds[name], 0.0)))
    print(f"{what}: largest error / bound  S {ratios['S']:.3e}  Ta {ratios['Ta']:.3e}  Tb {ratios['Tb']:.3e}; {want['fallbacks']} fallbacks")
    assert np.array_equal(n, want["n"])
    for name, val in (("S", S), ("Ta", Ta), ("Tb", Tb)):
        assert (np.abs(val - want[name]) <= bounds[name]).all(), name
        zero = bounds[name] == 0
        assert (val[zero] == 0).all() and not np.signbit(val[zero]).any()


def _run_block(ba, bb, M, K, kind):
    Gm, P, Q = _panel(M, K)
    xp, Pp, Qp, B, C = _device_sums(M, K)
    ia, ib = _lists(ba, bb, kind)
    got = _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib)
    want = FO.resid_cor_block(Gm[ia], Gm[ib], P, Q[ia], Q[ib], B[:, :K].cpu().numpy(), C[:, :K].cpu().numpy())
    return got, want, ia, ib


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K", SUMS_CASES)
def test_em_sums_against_float64(b, M, K):
    """nadm_em_sums over a gather list out of order and with a duplicate against the float64 sums: within 2^-20 of the sum of the
    terms' magnitudes (module docstring), pad columns 0, a SNP nobody observes exactly 0."""
    from neural_admixture_amd import fitcheck
    dev = _dev()
    Gm, P, Q = _panel(M, K)
    rows = _rows(b, 77 + b)
    if b >= 4:
        assert rows[-1] == rows[0] and (np.diff(rows) < 0).any()
    Bd, Cd = fitcheck.em_sums(_packed(Gm).to(dev), M, P, Q[rows], torch.from_numpy(rows).to(dev))
    torch.cuda.synchronize()
    kp = Bd.shape[1]
    assert Bd.dtype == torch.float32 and tuple(Bd.shape) == tuple(Cd.shape) == (M, kp) and kp % 4 == 0 and kp >= K
    Bd, Cd = Bd.cpu().numpy(), Cd.cpu().numpy()
    assert not Bd[:, K:].any() and not Cd[:, K:].any()
    B64, C64 = FO.em_sums(Gm[rows], P, Q[rows])
    for name, got, want in (("B", Bd[:, :K], B64), ("C", Cd[:, :K], C64)):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.max(np.where(want > 0, np.abs(got - want) / want, 0.0)))
        print(f"em_sums b={b} M={M} K={K}: max |{name} - {name}64| / {name}64 = {r:.3e} (bound {TOL_SUMS:.3e})")
        assert (np.abs(got - want) <= TOL_SUMS * want).all()
        assert (got[want == 0] == 0).all()
    if M > 5:
        assert not Bd[3].any() and not Cd[3].any()


@pytest.mark.gpu
@pytest.mark.parametrize("ba, bb, M, K, kind", BLOCKS)
def test_block_against_the_oracle(ba, bb, M, K, kind):
    got, want, ia, ib = _run_block(ba, bb, M, K, kind)
    _check_block(got, want, f"ba={ba} bb={bb} M={M} K={K}")
    S, Ta, Tb, n = got
    if kind == "few":
        assert ia[1] == ia[4] and set(ia) & set(ib) and list(ia[:3]) != list(ib)
        assert S[1].tobytes() == S[4].tobytes() and n[1].tobytes() == n[4].tobytes()
    if ba >= 3 and M > 5:                                        # the all-missing sample: exactly nothing, either way round
        a1 = np.flatnonzero(ia == 1)
        assert len(a1) and not n[a1].any() and not S[a1].any() and not Ta[a1].any() and not Tb[a1].any()
    if bb >= 3 and M > 5 and kind == "perm":
        b1 = np.flatnonzero(ib == 1)
        assert len(b1) and not n[:, b1].any() and not S[:, b1].any() and not Ta[:, b1].any() and not Tb[:, b1].any()
    if K > 1 and bb >= 3:
        assert want["fallbacks"] > 0                             # sample 2 carries the last component alone: its refit falls back to p


@pytest.mark.gpu
def test_several_ranges():
    """The smallest M at which a 70 x 70 block is cut into two ranges, taken from nadm_resid_cor_ranges: partials of two blocks per
    pair, folded in range order."""
    from neural_admixture_amd._lib import lib
    M = next(m for m in range(300, 4000, 100) if int(lib.nadm_resid_cor_ranges(70, 70, m, 4)) >= 2)
    assert int(lib.nadm_resid_cor_ranges(70, 70, M, 4)) >= 2
    got, want, _, _ = _run_block(70, 70, M, 3, "perm")
    _check_block(got, want, f"ba=70 bb=70 M={M} K=3 ranges={int(lib.nadm_resid_cor_ranges(70, 70, M, 4))}")


@pytest.mark.gpu
def test_same_bits_twice_and_a_permuted_list_permutes_the_columns():
    M, K = 515, 3
    xp, Pp, Qp, B, C = _device_sums(M, K)
    ia, ib = _lists(70, 70, "perm")
    a = _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib)
    b = _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    perm = np.random.default_rng(3).permutation(70)
    c = _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib[perm])
    assert all(np.ascontiguousarray(x[:, perm]).tobytes() == y.tobytes() for x, y in zip(a, c))
    B2, C2 = (t.clone() for t in _device_sums(M, K)[3:])
    assert torch.equal(B, B2) and torch.equal(C, C2)            # the sums, too, come out with the same bits


@pytest.mark.gpu
def test_pad_bits_and_p_where_nobody_observes_do_not_enter():
    from neural_admixture_amd._packed import pad_P
    M, K = 515, 3
    Gm, P, Q = _panel(M, K)
    xp, Pp, Qp, B, C = _device_sums(M, K)
    ia, ib = _lists(70, 70, "perm")
    clean = _gpu_block(xp, M, K, Pp, Qp, B, C, ia, ib)
    dirty = _gpu_block(_packed(Gm, dirty=True).to(xp.device), M, K, Pp, Qp, B, C, ia, ib)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    assert (Gm[:, 3] == 3).all()
    P2 = P.copy()
    P2[3] = 0.731
    other = _gpu_block(xp, M, K, pad_P(P2, xp.device), Qp, B, C, ia, ib)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, other))


def _cor_tolerance(want):
    """First-order bound of c = S / sqrt(Ta Tb) from the three sums' bounds, with 1 % for the second order."""
    S, Ta, Tb = want["S"], want["Ta"], want["Tb"]
    tS = TOL_ACC * want["absS"] + TOL_D * want["linS"]
    tA = TOL_ACC * Ta + 2 * TOL_D * want["linTa"]
    tB = TOL_ACC * Tb + 2 * TOL_D * want["linTb"]
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(Ta * Tb)
        return 1.01 * (tS / root + np.abs(S) / root * (tA / (2 * Ta) + tB / (2 * Tb)))


@pytest.mark.gpu
def test_resid_cor_is_symmetric_has_a_nan_diagonal_and_equals_the_block_oracle():
    """70 samples in blocks of 32 rows: nine ordered blocks, three of them ragged."""
    from neural_admixture_amd import fitcheck
    dev = _dev()
    M, K = 515, 3
    Gm, P, Q = FO.make_panel(70, M, K, seed=2)
    xp = _packed(Gm).to(dev)
    cor, n = fitcheck.resid_cor(xp, M, P, Q, rows=32)
    B, C = fitcheck.em_sums(xp, M, P, Q)
    torch.cuda.synchronize()
    assert cor.dtype == torch.float64 and n.dtype == torch.int32 and tuple(cor.shape) == tuple(n.shape) == (70, 70)
    c, nn = cor.cpu().numpy(), n.cpu().numpy()
    assert c.tobytes() == np.ascontiguousarray(c.T).tobytes() and np.isnan(np.diagonal(c)).all()
    want = FO.resid_cor_block(Gm, Gm, P, Q, Q, B[:, :K].cpu().numpy(), C[:, :K].cpu().numpy())
    assert np.array_equal(nn, want["n"]) and np.array_equal(nn, nn.T)
    c64 = FO.cor_of(want["S"], want["Ta"], want["Tb"])
    tol = _cor_tolerance(want)
    w = (c64 + c64.T) * 0.5
    t = (tol + tol.T) * 0.5
    np.fill_diagonal(w, np.nan)
    assert np.array_equal(np.isnan(c), np.isnan(w)) and np.isnan(c[1]).all() and np.isfinite(c).sum() >= 68 * 67
    ok = ~np.isnan(w)
    # sample 2 alone carries the last component: the refit without anybody else reproduces its genotype, its residual is round-off
    # and so is its correlation with anybody (the bound says as much); the printed difference leaves it out
    plain = ok.copy()
    plain[2], plain[:, 2] = False, False
    print(f"resid_cor rows=32: largest share of its bound {(np.abs(c - w)[ok] / t[ok]).max():.3e}; largest |c - c64| {np.abs(c - w)[plain].max():.3e} "
          f"(with the sample that alone carries a component: {np.abs(c - w)[ok].max():.3e})")
    assert (np.abs(c - w)[ok] <= t[ok]).all()
    whole, n2 = fitcheck.resid_cor(xp, M, P, Q)                  # one block: the same sums in the same order
    assert torch.equal(n2, n) and whole.cpu().numpy().tobytes() == c.tobytes()
    sub = torch.tensor([5, 40, 2, 69, 33], device=dev)
    cs, ns = fitcheck.resid_cor(xp, M, P, Q, pairs_idx=sub)
    assert cs.cpu().numpy().tobytes() == np.ascontiguousarray(c[np.ix_(sub.cpu().numpy(), sub.cpu().numpy())]).tobytes()


@pytest.mark.gpu
def test_engine_resid_cor_equals_the_library_free_form_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from neural_admixture_amd import fitcheck
    from oracle import nadm_oracle as O
    dev = _dev()
    N, M, ks, Hd, C_ = 96, 1027, [3, 5], 32, 8
    Gm = O.synth_genotypes(N, M, 5, seed=3, missing=0.05)
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, C_)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(sum(ks), M)).astype(np.float32)
    p = O.make_params(42, V0, P0, Hd, ks)
    small = np.concatenate([p.g, p.W1.reshape(-1), p.b1] + [x for h in range(len(ks)) for x in (p.Wk[h].reshape(-1), p.bk[h])])
    bmax = 40
    e = na.Engine(M, C_, Hd, ks, dev, bmax)
    e.load_params(V0, P0, small)
    e.pack_from_host(torch.from_numpy(Gm))
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (e.pflat, e.mflat, e.vflat)]
    Qh = torch.cat([e.infer_q(idx[s:s + bmax], min(bmax, N - s))[1] for s in range(0, N, bmax)], dim=0)
    got = e.resid_cor(head=1, rows=64)
    want = fitcheck.resid_cor(e.xp, M, e.P(1).clone(), Qh, rows=64)
    assert torch.equal(got[0].nan_to_num(7.0), want[0].nan_to_num(7.0)) and torch.equal(got[1], want[1])
    assert tuple(got[0].shape) == (N, N) and int(torch.isfinite(got[0]).sum()) > N * (N - 1) // 2
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_fit_end_to_end(tmp_path, caplog):
    """The `fit` mode on a small BED written here: a panel of four unadmixed populations of 12 samples x 1500 SNPs fitted with K = 3
    (the last two share a component), the .P / .Q files of that fit and the populations as --pops_path.  The three files hold what
    fitcheck.resid_cor and group_means return; the log warns about the two merged populations and the pair of them, and about
    nothing else."""
    from neural_admixture_amd import cli, fitcheck
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    Gm, P, Q, pop = FO.panel_merged(3, N=48, M=1500, hi=0.4)
    N, M = Gm.shape
    np.savetxt(tmp_path / "run.3.Q", Q.astype(np.float32), delimiter=" ")
    np.savetxt(tmp_path / "run.3.P", P.astype(np.float32), delimiter=" ")
    LO.write_bed(tmp_path / "panel", Gm)
    (tmp_path / "pops").write_text("".join(f"pop{p}\n" for p in pop))
    caplog.set_level(logging.INFO)
    argv = ["fit", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(tmp_path), "--name", "run", "--k", "3"]
    assert cli.main(argv + ["--pops_path", str(tmp_path / "pops"), "--out_name", "chk", "--matrix"]) == 0
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    assert not data.flipped
    Pr, Qr = (np.loadtxt(tmp_path / f"run.3.{x}", dtype=np.float32, ndmin=2) for x in "PQ")
    cor, n = fitcheck.resid_cor(data.packed, M, Pr, Qr)
    c = cor.cpu().numpy()
    back = np.loadtxt(tmp_path / "chk.3.cor", dtype=np.float32, ndmin=2)
    assert back.shape == (N, N) and np.array_equal(back, c.astype(np.float32), equal_nan=True)
    labels = np.asarray([f"pop{p}" for p in pop])
    means, counts, groups = fitcheck.group_means(c, labels)
    lines = (tmp_path / "chk.3.cor_pop").read_text().splitlines()
    assert lines[0].split() == groups == ["pop0", "pop1", "pop2", "pop3"]
    assert np.allclose(np.asarray([[float(v) for v in ln.split()] for ln in lines[1:]]), means, atol=5.1e-9)
    sm, sn = fitcheck.sample_means(c)
    smp = np.loadtxt(tmp_path / "chk.3.cor_sample", ndmin=2)
    assert smp.shape == (N, 2) and np.allclose(smp[:, 0], sm, atol=5.1e-9) and np.array_equal(smp[:, 1].astype(np.int64), sn) and (sn == N - 1).all()
    print("group means:\n" + "\n".join(" ".join(f"{v:+.4f}" for v in row) for row in means))
    assert means[2, 2] > 0.05 and means[3, 3] > 0.05 and means[2, 3] < -0.05
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("Fit check (K=3): mean residual correlation within groups ") for m in msgs)
    warns = [m for m in msgs if "Warning (K=3): group" in m]
    assert any("group pop2:" in m and "positive within a group" in m for m in warns)
    assert any("group pop3:" in m and "positive within a group" in m for m in warns)
    assert any("groups pop2 and pop3:" in m and "negative between groups" in m for m in warns)
    assert len(warns) == 3, warns
    assert any("Largest move of a frequency under one EM step of P from the given P (K=3)" in m for m in msgs)
    assert not any("fixed point" in m for m in msgs)            # the .P is a converged block-EM fit
    assert any("Residual correlations saved." in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    # without labels the groups are the largest components, named 1..K; a subsample takes the pairs among fewer samples
    caplog.clear()
    assert cli.main(argv + ["--out_name", "sub", "--subsample", "20", "--seed", "5"]) == 0
    lines = (tmp_path / "sub.3.cor_pop").read_text().splitlines()
    assert lines[0].split() == ["1", "2", "3"] and len(lines) == 4
    assert len((tmp_path / "sub.3.cor_sample").read_text().splitlines()) == 20 and not (tmp_path / "sub.3.cor").exists()
    pick = np.sort(np.random.default_rng(5).choice(N, size=20, replace=False))
    smp = np.loadtxt(tmp_path / "sub.3.cor_sample", ndmin=2)
    assert np.allclose(smp[:, 0], fitcheck.sample_means(c[np.ix_(pick, pick)])[0], atol=5.1e-9)
    assert any("--subsample: the pairs among 20 of 48 samples" in r.getMessage() for r in caplog.records)


@pytest.mark.gpu
def test_train_fit_check_end_to_end_on_the_demo(tmp_path, caplog):
    """Train the demo for a few epochs with --polish 2 --fit_check, then run the `fit` mode on the written files: both write
    {name}.3.cor_pop and .cor_sample, equal entry for entry, and both log the line per K."""
    from neural_admixture_amd import cli
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = np.load(f"{golden}/demo_k3.npz")
    N = int(d["N"])
    d["bed_bytes"].tofile(tmp_path / "demo.bed")
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    assert cli.main(["train", "--epochs", "5", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--polish", "2", "--fit_check"]) == 0
    assert cli.main(["fit", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--out_name", "again"]) == 0
    for ext in ("cor_pop", "cor_sample"):
        a, b = ((out / f"{name}.3.{ext}").read_text() for name in ("demo", "again"))
        assert a == b and len(a.splitlines()) == (N if ext == "cor_sample" else 1 + len(a.splitlines()[0].split()))
    msgs = [r.getMessage() for r in caplog.records]
    assert len([m for m in msgs if m.startswith("Fit check (K=3): mean residual correlation within groups ")]) == 2
    assert any("Residual correlations saved." in m for m in msgs)
