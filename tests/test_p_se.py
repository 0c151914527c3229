"""Standard errors of P (nadm_snp_info, pse.p_info / se_from_info / p_se, Engine.p_se, the `pse` mode of the command line and `train
--p_se`).  The numpy restatements (float64 truth, float32 yardstick, the per-SNP inverse, the calibration) live in tests/pse_oracle.py.

The tolerance of the sums against float64 is set as tests/test_hwe.py sets its own: the float32 RESTATEMENT (pse_oracle.info32: fp32
pi with k in order, an fp32 product r u and an fp32 division, fp32 products w q_a and (w q_a) q_b, fp32 sums in sample order over
slices of at most 4096 samples, slices added in float64) is run on the CPU over the same cases, its largest relative deviation from
float64 is taken, and a margin of 8 x covers another summation order, fused multiply-adds and the hardware's 1-ulp reciprocal.  n is
an integer: equal.  An entry that is 0 in float64 must be exactly +0.0; otherwise, every term being non-negative,
    |I - I64| <= TOL I64        per entry
MEASURED with the restatement on the CPU (largest ratio over the cases of a group; per case 4.9e-7 .. 1.9e-6):
    CASES (b <= 200)            YARD      = 1.898e-06 (b = 130, M = 1027, K = 1)
    b = 4200, M = 257, K = 8    YARD_BIG  = 1.008e-05
    b = 12000, M = 3001, K = 8  YARD_DEEP = 1.002e-05
    planted panel, SE           YARD_SE   = 6.035e-07   (info32 pushed through the float64 inversion, relative, SNPs with cond <= 1e6)
    se_from_info against numpy  YARD_INV  = 4.372e-16  (the batched Cholesky route on CPU tensors against numpy.linalg.inv, relative)
(The two large shapes are dominated by the restatement's 4096-term fp32 sums; the library's slices are shorter there.)
`python tests/test_p_se.py` measures the yardsticks again and prints them (CPU only).
OBSERVED on an MI355X: see DESIGN.md section 4.14 (each case prints its ratio before it asserts)."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hwe_oracle as HO  # noqa: E402
import ld_oracle as LO  # noqa: E402
import pse_oracle as PO  # noqa: E402
from packed_rows import case_rows, dev as _dev, packed as _packed  # noqa: E402

ROWS = 200                   # resident rows of the GPU cases
_rows = functools.partial(case_rows, resident=ROWS)
# (b, M, K, rows): every b, M and K of the issue at least once, not their product: every kp (4, 8, 12, 16) full and with a K below it.
# rows: "list" = a permuted gather list with a duplicate, "none" = rows 0..b without a list
CASES = [(1, 257, 2, "list"), (70, 1027, 3, "none"), (130, 3001, 8, "list"), (200, 257, 9, "list"), (70, 3001, 16, "list"),
         (130, 1027, 1, "list"), (200, 1027, 4, "none"), (130, 257, 13, "none"), (200, 3001, 5, "list"), (70, 257, 12, "list")]
BIG_B, BIG_M, BIG_K = 4200, 257, 8                       # crosses the 4096 samples of one fp32 sum
DEEP_B, DEEP_M, DEEP_K = 12000, 3001, 8                  # slices of several tiles: the steady state of the tile loop
MARGIN = 8.0
YARD, YARD_BIG, YARD_DEEP = 1.898e-06, 1.008e-05, 1.002e-05                # measured: module docstring
YARD_SE, YARD_INV = 6.035e-07, 4.372e-16
TOL, TOL_BIG, TOL_DEEP, TOL_SE, TOL_INV = (MARGIN * y for y in (YARD, YARD_BIG, YARD_DEEP, YARD_SE, YARD_INV))
COND_CAP, COND_SHARE = 1e6, 0.95


# ------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS resident rows with the planted cases of hwe_oracle.make_edge_case; the tests leave them as they are."""
    return HO.make_edge_case(ROWS, M, K)


@functools.lru_cache(maxsize=None)
def _weights(M, K):
    Gm, P, Q, _ = _case(M, K)
    return PO.weights(Gm, P, Q)


@functools.lru_cache(maxsize=None)
def _planted():
    """The planted panel with its TRUE P and Q: (G, P, Q, info64, n64, the oracle's se result).  The expected information does not
    depend on the calls' values, so the planted artefacts of the panel do not matter here."""
    Gm, P, Q, _ = HO.make_planted(0)
    I, n = PO.info(Gm, P, Q)
    return Gm, P, Q, I, n, PO.se(I, P, n)


def _ratio(I, I64):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(I64 > 0, np.abs(I - I64) / I64, 0.0)))


def _rel_se(se, se64, ok):
    """Largest relative deviation of se from se64 over the SNPs ``ok`` (NaN entries must pair up: checked by the callers)."""
    a, b = se[ok], se64[ok]
    both = ~np.isnan(b)
    return float(np.max(np.abs(a[both] - b[both]) / b[both]))


# ------------------------------------------------------------------------------------------------ CPU: hand cases
def _se_torch(I, P, n, bound=1e-4):
    from neural_admixture_amd import pse
    r = pse.se_from_info(torch.from_numpy(np.asarray(I, dtype=np.float64)), torch.from_numpy(np.asarray(P, dtype=np.float32)),
                         torch.from_numpy(np.asarray(n).astype(np.int32)), bound)
    assert r.se.dtype == torch.float64 and r.n_eff.dtype == torch.float64 and r.n.dtype == torch.int32
    assert r.fixed.dtype == torch.bool and r.unseen.dtype == torch.bool and r.se.device.type == "cpu"
    return r.se.numpy(), r.n_eff.numpy(), r.fixed.numpy(), r.unseen.numpy()


def test_k1_is_the_binomial_standard_error():
    """K = 1, Q = 1: I = 2 n / (p (1 - p)), SE = sqrt(p (1 - p) / (2 n)) and n_eff = 2 n, through the oracle and through
    pse.se_from_info on CPU tensors."""
    rng = np.random.default_rng(5)
    Gm = rng.binomial(2, 0.4, size=(50, 40)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.2] = 3
    P = rng.uniform(0.1, 0.9, size=(40, 1)).astype(np.float32)
    Q = np.ones((50, 1), dtype=np.float32)
    I, n = PO.info(Gm, P, Q)
    assert np.array_equal(n, (Gm != 3).sum(axis=0)) and (n > 0).all()
    p = P[:, 0].astype(np.float64)
    want = np.sqrt(p * (1 - p) / (2.0 * n))
    for s, ne in (PO.se(I, P, n)[:2], _se_torch(I, P, n)[:2]):
        assert np.abs(s[:, 0] / want - 1).max() < 1e-13 and np.abs(ne[:, 0] / (2.0 * n) - 1).max() < 1e-13


def test_one_hot_q_gives_per_population_binomial_errors():
    """One-hot Q rows: the information is diagonal, SE_jk = sqrt(p_jk (1 - p_jk) / (2 n_jk)) with n_jk the observed samples of
    population k at SNP j, and n_eff = 2 n_jk."""
    rng = np.random.default_rng(6)
    N, M, K = 60, 30, 3
    pop = rng.integers(0, K, size=N)
    Q = np.eye(K, dtype=np.float32)[pop]
    P = rng.uniform(0.1, 0.9, size=(M, K)).astype(np.float32)
    Gm = rng.binomial(2, 0.5, size=(N, M)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.1] = 3
    I, n = PO.info(Gm, P, Q)
    njk = np.stack([(Gm[pop == k] != 3).sum(axis=0) for k in range(K)], axis=1)
    assert (njk > 0).all()
    offd = [t for t, (a, b) in enumerate(PO.pairs(K)) if a != b]
    assert (I[:, offd] == 0).all()
    p = P.astype(np.float64)
    want = np.sqrt(p * (1 - p) / (2.0 * njk))
    for s, ne in (PO.se(I, P, n)[:2], _se_torch(I, P, n)[:2]):
        assert np.abs(s / want - 1).max() < 1e-13 and np.abs(ne / (2.0 * njk) - 1).max() < 1e-13


def test_three_samples_two_components_by_hand():
    """Q_a = (1, 0), Q_b = (1/2, 1/2), Q_c = (0, 1).
    SNP 0, P = (1/2, 1/2): every pi = 1/2, w = 2 / (1/4) = 8.  I00 = 8 (1 + 1/4) = 10, I01 = 8 / 4 = 2, I11 = 10; the inverse is
        [[10, -2], [-2, 10]] / 96: SE = sqrt(10 / 96) for both, n_eff = (1/4) (96 / 10) = 2.4.
    SNP 1, P = (1/4, 3/4), b missing: pi_a = 1/4, pi_c = 3/4, w = 2 / (3/16) = 32/3 for both; I = diag(32/3, 32/3), n = 2:
        SE = sqrt(3 / 32), n_eff = (3/16) (32/3) = 2 -- one sample, two allele copies each.
    SNP 2, P = (1/4, 3/4), everybody observed: pi_b = 1/2 adds 8/4 = 2 to every entry: I00 = I11 = 38/3, I01 = 2, det = 1408/9,
        SE = sqrt((38/3) / (1408/9)) = sqrt(57 / 704).
    The calls' own values do not enter."""
    Gm = np.asarray([[2, 1, 0], [1, 3, 2], [0, 2, 1]], dtype=np.uint8)
    Q = np.asarray([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], dtype=np.float32)
    P = np.asarray([[0.5, 0.5], [0.25, 0.75], [0.25, 0.75]], dtype=np.float32)
    for fn, tol in ((PO.info, 1e-14), (PO.info32, 1e-6)):
        I, n = fn(Gm, P, Q)
        assert np.array_equal(n, [3, 2, 3])
        assert np.allclose(I, [[10, 2, 10], [32 / 3, 0, 32 / 3], [38 / 3, 2, 38 / 3]], rtol=tol, atol=0)
        assert I[1, 1] == 0.0
    I, n = PO.info(Gm, P, Q)
    want = np.sqrt(np.asarray([[10 / 96] * 2, [3 / 32] * 2, [57 / 704] * 2]))
    for s, ne in (PO.se(I, P, n)[:2], _se_torch(I, P, n)[:2]):
        assert np.abs(s / want - 1).max() < 1e-14
        assert np.allclose(ne[:2], [[2.4, 2.4], [2.0, 2.0]], rtol=1e-13, atol=0)
    I2, n2 = PO.info(np.asarray([[0, 0, 2], [2, 3, 0], [1, 1, 0]], dtype=np.uint8), P, Q)        # other observed codes: the same bits
    assert I2.tobytes() == I.tobytes() and np.array_equal(n2, n)


def test_nan_exactly_where_a_component_is_fixed_unseen_or_nobody_observes():
    """K = 3, four samples: a (1, 0, 0), b (1/2, 1/2, 0), c (0, 1, 0), d (0, 0, 1) -- d alone carries component 2.
    SNP 0: everything in order: three finite SEs.
    SNP 1: p_0 = 5e-5 <= bound: fixed -> NaN there alone; the block of components 1 and 2 is inverted without it.
    SNP 2: p_1 = 1 - 5e-5 >= 1 - bound: fixed, likewise.
    SNP 3: d is missing: component 2 is unseen -> NaN there alone, and SE_0, SE_1 are those of the 2 x 2 block.
    SNP 4: nobody observed: n = 0 -> NaN in every entry, every component unseen.
    SNP 5: p_0 = 2e-4 is not fixed at the default bound and is at bound = 1e-3."""
    Q = np.asarray([[1, 0, 0], [0.5, 0.5, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    P = np.asarray([[0.3, 0.6, 0.5], [5e-5, 0.6, 0.5], [0.3, 1 - 5e-5, 0.5], [0.3, 0.6, 0.5], [0.3, 0.6, 0.5], [2e-4, 0.6, 0.5]], dtype=np.float32)
    Gm = np.ones((4, 6), dtype=np.uint8)
    Gm[3, 3] = 3
    Gm[:, 4] = 3
    I, n = PO.info(Gm, P, Q)
    assert np.array_equal(n, [4, 4, 4, 3, 0, 4])
    want_nan = np.zeros((6, 3), dtype=bool)
    want_nan[1, 0] = want_nan[2, 1] = want_nan[3, 2] = True
    want_nan[4] = True
    for s, ne, fixed, unseen in (PO.se(I, P, n)[:4], _se_torch(I, P, n)):
        assert np.array_equal(np.isnan(s), want_nan) and np.array_equal(np.isnan(ne), want_nan)
        assert np.array_equal(fixed, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
        assert np.array_equal(unseen, [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]])
        # the dropped component leaves the block of the others: d is one-hot, so components 0 and 1 never see component 2
        assert np.allclose(s[3, :2], s[0, :2], rtol=1e-14, atol=0) and np.allclose(s[0, 2], np.sqrt(0.25 / 2), rtol=1e-14, atol=0)
        # SNP 1 without component 0: samples b (q_1 = 1/2) and c (q_1 = 1) carry component 1
        pi_b, pi_c = 0.5 * float(P[1, 0]) + 0.5 * float(P[1, 1]), float(P[1, 1])
        i11 = 2 / (pi_b * (1 - pi_b)) / 4 + 2 / (pi_c * (1 - pi_c))
        assert np.allclose(s[1, 1], 1 / np.sqrt(i11), rtol=1e-13, atol=0)
    s3 = _se_torch(I, P, n, bound=1e-3)
    assert np.isnan(s3[0][5, 0]) and s3[2][5, 0] and np.isfinite(s3[0][5, 1:]).all() and np.isfinite(_se_torch(I, P, n)[0][5]).all()
    assert np.isnan(PO.se(I, P, n, bound=1e-3)[0][5, 0])


def test_a_block_that_is_not_positive_definite_is_nan_throughout():
    """Two components that every observed sample carries in the same proportion: the 2 x 2 block is singular (in float64 a
    factorisation either fails or yields a non-positive pivot) or, made indefinite by hand, certainly not positive definite."""
    P = np.asarray([[0.3, 0.6], [0.3, 0.6]], dtype=np.float32)
    I = np.asarray([[1.0, 2.0, 1.0], [4.0, 1.0, 2.0]])                 # SNP 0: [[1, 2], [2, 1]] is indefinite; SNP 1 is fine
    n = np.asarray([5, 5])
    for s in (PO.se(I, P, n)[0], _se_torch(I, P, n)[0]):
        assert np.isnan(s[0]).all() and np.isfinite(s[1]).all()
        assert np.allclose(s[1], np.sqrt(np.asarray([2.0, 4.0]) / 7.0), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ CPU: the real function, calibration
def test_oracle_alone_meets_the_condition_cap_on_the_planted_panel():
    Gm, P, Q, I, n, (s, ne, fixed, unseen, cond) = _planted()
    share = float((cond <= COND_CAP).mean())
    print(f"planted panel: {share:.4f} of the SNPs have a free block with condition number <= {COND_CAP:g}; median {np.median(cond):.2f}, max {cond.max():.3e}")
    assert Gm.shape == (300, 3000) and share >= COND_SHARE
    assert not fixed.any() and not unseen.any() and np.isfinite(s).all()          # P in [0.02, 0.98], every component is carried


def test_se_from_info_against_the_oracle_on_the_planted_panel():
    """pse.se_from_info (the batched Cholesky route, CPU tensors) against numpy.linalg.inv per SNP, over the SNPs whose free block
    has a condition number <= 1e6; the same NaN pattern; the tolerance is 8 x the largest deviation measured (module docstring)."""
    Gm, P, Q, I, n, (s64, ne64, fixed64, unseen64, cond) = _planted()
    s, ne, fixed, unseen = _se_torch(I, P, n)
    ok = cond <= COND_CAP
    assert ok.mean() >= COND_SHARE
    assert np.array_equal(np.isnan(s), np.isnan(s64)) and np.array_equal(fixed, fixed64) and np.array_equal(unseen, unseen64)
    r = _rel_se(s, s64, ok)
    print(f"se_from_info against numpy.linalg.inv: largest relative deviation {r:.3e} (bound {TOL_INV:.3e})")
    assert r <= TOL_INV
    assert _rel_se(ne, ne64, ok) <= 2.5 * TOL_INV                                  # n_eff ~ se^-2


def test_calibration_of_the_restated_procedure():
    """pse_oracle.calibration: 40 independently drawn panels of 300 x 600, K = 3, 5 % of the calls missing, P refitted by masked EM
    at the true Q, the SE from the expected information at the fit.  The median over the interior entries of SE / spread must be
    within [0.95, 1.05] and the share of |z| < 1.96 within [0.92, 0.97].
    MEASURED with the committed oracle: ratio 1.0056 (5 % - 95 %: 0.837 - 1.207), coverage 94.46 %, sd of z 1.021, 1337 interior
    entries, the last of the 60 EM steps 5e-5 (150 steps change the ratio in the sixth digit).  With 1337 entries whose ratio has a
    spread of 0.11 the sampling error of the median is about 0.4 %: the bounds leave about ten standard errors."""
    r = PO.calibration()
    print(f"calibration: SE / spread median {r['ratio']:.4f} (5 % - 95 %: {r['ratio_5_95'][0]:.3f} - {r['ratio_5_95'][1]:.3f}), coverage "
          f"{r['coverage']:.4f}, sd of z {r['z_sd']:.4f}, {r['interior']} interior entries, last EM step {r['em_step']:.1e}")
    assert r["interior"] >= 1200
    assert 0.95 <= r["ratio"] <= 1.05
    assert 0.92 <= r["coverage"] <= 0.97


# ------------------------------------------------------------------------------------------------ CPU: host-side checks
def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_snp_info", "nadm_snp_info_slices", "nadm_snp_info_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "EXPECTED information" in header


def test_slices_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    sl, f = lib.nadm_snp_info_slices, lib.nadm_snp_info_scratch_floats
    bs, Ms, kps = (1, 63, 64, 65, 130, 4096, 4097, 32768, 100000), (1, 255, 256, 257, 3001, 500000), (4, 8, 12, 16)
    for b in bs:
        for M in Ms:
            s, tiles, chunks = int(sl(b, M)), (b + 63) // 64, (M + 255) // 256
            assert s == int(lib.nadm_snp_hwe_slices(b, M)) and 1 <= s <= tiles and -(-tiles // s) * 64 <= 4096
            for kp in kps:
                assert int(f(b, M, kp)) >= s * chunks * 256 * (kp * (kp + 1) // 2 + 1)
            v = [int(f(b, M, kp)) for kp in kps]
            assert v[0] > 0 and all(y > x for x, y in zip(v, v[1:]))           # grows with kp
    for kp in kps:
        for b in bs:
            v = [int(f(b, M, kp)) for M in Ms]
            assert all(y >= x for x, y in zip(v, v[1:]))
        for M in Ms:
            v = [int(f(b, M, kp)) for b in bs]
            assert all(y >= x for x, y in zip(v, v[1:]))
    # the block rule of pse.p_info: at most 8 slices of 32768 rows, 0.6 GB at M = 500k, K = 8
    assert int(sl(32768, 500000)) == 8 and int(f(32768, 500000, 8)) * 4 <= 0.6 * 1024 ** 3
    for bad in ((0, 100, 4), (-1, 100, 4), (4, 0, 4), (4, -5, 4), (4, 100, 0), (4, 100, 6), (4, 100, 24), (4, 100, 64)):
        assert int(f(*bad)) == 0
    assert int(sl(0, 100)) == 0 and int(sl(4, 0)) == 0


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 24), 0.25)
    P = torch.full((50, 24), 0.25)
    info = torch.empty(50 * 6, dtype=torch.float64)
    nobs = torch.empty(50, dtype=torch.int32)
    scratch = torch.empty(4 * 256 * 7)
    keep = (xp, P, Q, info, nobs, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, Q=Q.data_ptr(), q_stride=24, k=3, kp=4, P=P.data_ptr(), eps=1e-6,
             info=info.data_ptr(), nobs=nobs.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(P=None), "null pointer"), (dict(info=None), "null pointer"),
    (dict(nobs=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(b=0), "empty block"), (dict(b=-3), "empty block"), (dict(M=0), "empty block"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(k=17, kp=24), "K must be <= 16"), (dict(k=64, kp=64, q_stride=64), "K must be <= 16"),
    (dict(unaligned="xp"), "must be 16-byte aligned"), (dict(unaligned="Q"), "must be 16-byte aligned"), (dict(unaligned="P"), "must be 16-byte aligned"),
    (dict(unaligned="scratch"), "must be 16-byte aligned"), (dict(unaligned="info"), "8-byte"), (dict(unaligned2="nobs"), "4-byte"),
])
def test_snp_info_refuses_before_any_launch(change, message):
    """Every refusal of nadm_snp_info is decided on the host: it is reported with its message on a machine without a GPU (where a
    launch would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "unaligned2" in change:
        a[change["unaligned2"]] += 2
    else:
        a.update(change)
    status = lib.nadm_snp_info(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_snp_info"):
        check(status, "snp_info")
    del keep


def test_snp_info_se_refuses_before_any_launch():
    """The inversion kernel's entry: null pointers, an empty block, K outside 1..16 and misalignment, each with its message."""
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "nadm_snp_info_se(" in open(os.path.join(root, "include", "nadm.h")).read() and "nadm_snp_info_se" in EXPORTS
    info, drop = torch.zeros(5 * 6, dtype=torch.float64), torch.zeros(5 * 3, dtype=torch.uint8)
    nobs, se = torch.ones(5, dtype=torch.int32), torch.zeros(5 * 3, dtype=torch.float64)
    base = dict(info=info.data_ptr(), drop=drop.data_ptr(), nobs=nobs.data_ptr(), M=5, k=3, se=se.data_ptr(), stream=None)
    for change, message in ((dict(info=None), "null pointer"), (dict(drop=None), "null pointer"), (dict(nobs=None), "null pointer"),
                            (dict(se=None), "null pointer"), (dict(M=0), "empty block"), (dict(k=0), "K must be in 1..16"),
                            (dict(k=17), "K must be in 1..16"), (dict(info=info.data_ptr() + 4), "8-byte"),
                            (dict(se=se.data_ptr() + 4), "8-byte"), (dict(nobs=nobs.data_ptr() + 2), "4-byte")):
        a = dict(base, **change)
        assert lib.nadm_snp_info_se(*a.values()) != 0 and message in lib.nadm_last_error().decode()


def test_python_layer_refuses_a_wide_head_and_a_bad_row_block_in_words():
    from neural_admixture_amd import pse
    xp = torch.zeros((4, 16), dtype=torch.uint8)                     # (a CPU tensor: the refusals come before it is looked at)
    with pytest.raises(RuntimeError, match="K must be <= 16 for standard errors of P"):
        pse.p_info(xp, 50, np.full((50, 17), 0.5, dtype=np.float32), np.full((4, 17), 1 / 17, dtype=np.float32))
    for rb in (0, 100, -64):
        with pytest.raises(RuntimeError, match="row_block must be a positive multiple of 64"):
            pse.p_info(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None, row_block=rb)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        pse.p_info(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None)
    with pytest.raises(RuntimeError, match=r"bound must be in \[0, 0.5\)"):
        pse.se_from_info(torch.zeros((2, 1), dtype=torch.float64), np.full((2, 1), 0.5), torch.ones(2, dtype=torch.int32), bound=0.5)
    with pytest.raises(RuntimeError, match=r"info must be \[2, 3\]"):
        pse.se_from_info(torch.zeros((2, 2), dtype=torch.float64), np.full((2, 2), 0.5), torch.ones(2, dtype=torch.int32))


def test_cli_pse_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing or misshapen files end the run with the offender named, before the GPU check and before a genotype
    is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["pse", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_pse_args(base[1:] + ["--k", "3"])
    assert (a.k, a.min_k, a.max_k, a.bound, a.out_name, a.threads, a.extract) == (3, None, None, 1e-4, None, 1, None)
    a = cli.parse_pse_args(base[1:] + ["--min_k", "2", "--max_k", "4", "--bound", "0.001", "--out_name", "o", "--threads", "4", "--extract", "f"])
    assert (a.min_k, a.max_k, a.bound, a.out_name, a.threads, a.extract) == (2, 4, 0.001, "o", 4, "f")

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    with pytest.raises(SystemExit, match="--k cannot be given together with --min_k / --max_k"):
        cli.main(base + ["--k", "3", "--min_k", "2"])
    for ks in (["--k", "17"], ["--min_k", "15", "--max_k", "17"]):
        with pytest.raises(SystemExit, match=r"pse needs every K <= 16.*K = 17 was asked for"):
            cli.main(base + ks)
    for value in ("0.5", "-0.1", "nan"):
        with pytest.raises(SystemExit, match=r"--bound must be in \[0, 0.5\)"):
            cli.main(base + ["--k", "3", "--bound", value])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen"), "--k", "3"])
    with pytest.raises(SystemExit, match=r"pse needs the .*run\.3\.P not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"run\.4\.P not found"):
        cli.main(base + ["--min_k", "3", "--max_k", "4"])
    with pytest.raises(SystemExit, match=r"x\.fam not found"):
        cli.main(base + ["--k", "3"])
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j + 1}\tA\tG\n" for j in range(9)))
    bed.write_bytes(bytes(3 + 2 * 9))                        # N = 5, M = 9; the .P has 10 rows
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 3 matrix, the model needs 9 x 3"):
        cli.main(base + ["--k", "3"])
    (tmp_path / "list").write_text("rs1\nrs7\nrs3\n")
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 3 matrix, the model needs 3 x 3"):
        cli.main(base + ["--k", "3", "--extract", str(tmp_path / "list")])
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + ["--k", "3"])
    assert not list(tmp_path.glob("*.P_se"))


def test_train_p_se_refuses_sharded_and_supervised_runs(tmp_path, monkeypatch):
    """`train --p_se`: the refusals and the wording of --bootstrap, before the GPU check; the keyword of train() likewise."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["train", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "x.bed"), "--k", "3", "--p_se"]
    assert cli.parse_train_args(base[1:]).p_se is True and cli.parse_train_args(base[1:-1]).p_se is False
    with pytest.raises(SystemExit, match=r"--p_se is single-GPU: run it with --num_gpus 1"):
        cli.main(base + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--p_se ignores labels: it is not available with --pops_path"):
        cli.main(base + ["--pops_path", str(tmp_path / "pops")])
    with pytest.raises(SystemExit, match=r"--p_se needs every K <= 16"):
        cli.main(base[:-3] + ["--min_k", "15", "--max_k", "17", "--p_se"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(base)
    G0, V0 = torch.zeros((4, 100), dtype=torch.uint8), np.zeros((8, 100), np.float32)
    with pytest.raises(ValueError, match="p_se needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 2, 16, True, V0, None, p_se=True)
    with pytest.raises(ValueError, match="p_se needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 1, 16, True, V0, ["a", "b", "c", "a"], p_se=True)
    with pytest.raises(ValueError, match="p_se needs every K <= 16"):
        na.train(1, 8, 1e-3, 17, 0, G0, torch.device("cpu"), 1, 16, True, V0, None, p_se=True)
    with pytest.raises(RuntimeError, match="GPU"):               # default off: the positional signature is the reference's
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 0, 16, True, V0, None)


def test_sharded_and_cpu_engines_refuse_p_se():
    """Engine.p_se is single-GPU and needs the resident matrix; the checks come first, so a stand-in without device state shows them."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.p_se is single-GPU"):
        e.p_se()
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.p_se(0, 1e-3)
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.p_se needs the HIP engine with its packed matrix resident"):
        e.p_se()


def test_public_names():
    import neural_admixture_amd as na
    for name in ("p_se", "p_info", "se_from_info"):
        assert callable(getattr(na, name)) and name in na.__all__


def test_writer_round_trips_nan_included(tmp_path):
    from neural_admixture_amd import pse
    se = torch.tensor([[0.125, float("nan"), 3.0e-4], [float("nan"), float("nan"), float("nan")], [0.5, 0.03125, 1.0]], dtype=torch.float64)
    se[1, 1] = -se[1, 1]                                         # whatever NaN it is, the file says `nan`
    pse.write_se(tmp_path / "r.3.P_se", se)
    text = (tmp_path / "r.3.P_se").read_text()
    rows = [ln.split(" ") for ln in text.splitlines()]
    assert len(rows) == 3 and all(len(r) == 3 for r in rows) and rows[1] == ["nan", "nan", "nan"] and rows[0][1] == "nan"
    assert rows[0][0] == "1.250000000000000000e-01"              # the .P text format
    back = np.loadtxt(tmp_path / "r.3.P_se", dtype=np.float32, ndmin=2)
    assert np.array_equal(back, se.numpy().astype(np.float32), equal_nan=True)
    with pytest.raises(RuntimeError, match="must be a matrix"):
        pse.write_se(tmp_path / "bad", torch.zeros(3))


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_info(xp, M, P, Q, rows, kind, **kw):
    """One pse.p_info call -> numpy (info, n); Q [ROWS, K] are the resident rows' fractions."""
    from neural_admixture_amd import pse
    if kind == "none":
        out = pse.p_info(xp[:len(rows)], M, P, Q[:len(rows)], None, **kw)
    else:
        out = pse.p_info(xp, M, P, Q[rows], torch.from_numpy(rows).to(xp.device), **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_info(got, want, tol, what):
    """n equal; an entry that is 0 in float64 exactly +0.0, else |I - I64| <= tol I64; prints the largest ratio before it asserts."""
    I, n = got
    I64, n64 = want
    r = _ratio(I, I64)
    print(f"{what}: max |I - I64| / I64 = {r:.3e} (bound {tol:.3e})")
    assert I.dtype == np.float64 and n.dtype == np.int32 and I.shape == I64.shape
    assert np.array_equal(n, n64)
    zero = I64 == 0
    assert (I[zero] == 0).all() and not np.signbit(I[zero]).any()
    assert (np.abs(I - I64) <= tol * I64).all()
    return r


def _run_case(b, M, K, kind, tol, **kw):
    from neural_admixture_amd._lib import lib
    dev = _dev()
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(b, kind)
    want = PO.from_weights(_weights(M, K), Q, rows)
    got = _gpu_info(_packed(Gm).to(dev), M, P, Q, rows, kind, **kw)
    _check_info(got, want, tol, f"b={b} M={M} K={K} rows={kind} slices={int(lib.nadm_snp_info_slices(b, M))}")
    assert (got[0][dead] == 0).all() and (got[1][dead] == 0).all()      # the SNPs nobody observes: exactly nothing
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, kind", CASES)
def test_sums_against_float64(b, M, K, kind):
    """n equal, zeros exact, every other entry within the tolerance of the module docstring; every case prints its ratio first."""
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(b, kind)
    if kind == "list" and b > 2:
        assert Q[rows].max(axis=1).max() == 1.0 and (Gm[rows] == 3).all(axis=1).any() and ((Gm[rows] != 3).sum(axis=1) == 7).any()
        assert rows[-1] == rows[0] and len(set(rows.tolist())) == b - 1 and (P[0] == 0).all() and (P[1] == 1).all()
    _run_case(b, M, K, kind, TOL)


@pytest.mark.gpu
def test_more_samples_than_one_fp32_sum_covers():
    """b = 4200 rows (the resident ones with repeats): more than 4096 samples, hence several slices whatever M is."""
    from neural_admixture_amd._lib import lib
    assert int(lib.nadm_snp_info_slices(BIG_B, BIG_M)) >= 2
    _run_case(BIG_B, BIG_M, BIG_K, "list", TOL_BIG)


@pytest.mark.gpu
def test_slices_of_several_tiles():
    """The steady state of a real call: b = 12000 rows over 12 chunks leave slices of 3 tiles, so that the tile loop hands the
    prefetched rows over, reuses both LDS buffers and accumulates across tiles."""
    from neural_admixture_amd._lib import lib
    s = int(lib.nadm_snp_info_slices(DEEP_B, DEEP_M))
    assert -(-((DEEP_B + 63) // 64) // s) >= 3
    _run_case(DEEP_B, DEEP_M, DEEP_K, "list", TOL_DEEP)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["list", "none"])
def test_row_blocks_add_up_in_block_order(kind):
    """p_info(..., row_block=128) on 200 rows: within the tolerance of the truth, and bit-equal to the separate calls' results added
    in block order."""
    dev = _dev()
    M, K = 1027, 5
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(200, kind)
    xp = _packed(Gm).to(dev)
    (got, n), _ = _run_case(200, M, K, kind, TOL, row_block=128)
    if kind == "none":
        parts = [_gpu_info(xp[s:e], M, P, Q[s:e], np.arange(e - s, dtype=np.int32), "none") for s, e in ((0, 128), (128, 200))]
    else:
        parts = [_gpu_info(xp, M, P, Q, rows[s:e], "list") for s, e in ((0, 128), (128, 200))]
    assert (parts[0][0] + parts[1][0]).tobytes() == got.tobytes() and np.array_equal(parts[0][1] + parts[1][1], n)
    whole = _gpu_info(xp, M, P, Q, rows, kind)
    assert np.array_equal(whole[1], n) and _ratio(whole[0], got) < 2 * TOL


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    dev = _dev()
    M, K = 3001, 9
    Gm, P, Q, dead = _case(M, K)
    xp, rows = _packed(Gm).to(dev), _rows(130)
    a = _gpu_info(xp, M, P, Q, rows, "list")
    b = _gpu_info(xp, M, P, Q, rows, "list")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
def test_masked_terms_are_exactly_zero_and_the_calls_values_do_not_enter():
    """Ones in the pad bits of every row's last byte (and in the bytes behind it), a NaN or another P at the SNPs nobody observes,
    and other observed codes in place of the observed ones leave every output bit-identical."""
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(130)
    clean = _gpu_info(_packed(Gm).to(dev), M, P, Q, rows, "list")
    dirty = _gpu_info(_packed(Gm, dirty=True).to(dev), M, P, Q, rows, "list")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    assert (Gm[:, dead] == 3).all()
    P2 = P.copy()
    P2[dead[0]] = np.float32(np.nan)
    P2[dead[1]] = 0.731
    other = _gpu_info(_packed(Gm).to(dev), M, P2, Q, rows, "list")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, other))
    G2 = Gm.copy()
    obs = G2 != 3
    G2[obs] = np.random.default_rng(8).integers(0, 3, size=int(obs.sum())).astype(np.uint8)
    assert (G2 != Gm).mean() > 0.3
    recoded = _gpu_info(_packed(G2).to(dev), M, P, Q, rows, "list")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, recoded))


@pytest.mark.gpu
def test_planted_panel_on_the_gpu():
    """pse.p_se on the planted panel packed with the project's packer against the oracle's SE over the SNPs under the condition cap:
    within 8 x the yardstick (info32 pushed through the float64 inversion on the CPU), the NaN pattern identical."""
    from neural_admixture_amd import pse
    dev = _dev()
    Gm, P, Q, I64, n64, (s64, ne64, fixed64, unseen64, cond) = _planted()
    res = pse.p_se(_packed(Gm).to(dev), Gm.shape[1], P, Q)
    assert all(t.dtype == torch.float64 and t.device.type == "cuda" and tuple(t.shape) == P.shape for t in (res.se, res.n_eff))
    s, ne = res.se.cpu().numpy(), res.n_eff.cpu().numpy()
    assert np.array_equal(res.n.cpu().numpy(), n64) and np.array_equal(res.fixed.cpu().numpy(), fixed64) and np.array_equal(res.unseen.cpu().numpy(), unseen64)
    assert np.array_equal(np.isnan(s), np.isnan(s64)) and np.array_equal(np.isnan(ne), np.isnan(ne64))
    ok = cond <= COND_CAP
    assert ok.mean() >= COND_SHARE
    r = _rel_se(s, s64, ok)
    print(f"planted panel: largest relative deviation of SE {r:.3e} (bound {TOL_SE:.3e}); median SE {np.nanmedian(s):.4f}, median n_eff {np.nanmedian(ne):.1f}")
    assert r <= TOL_SE and _rel_se(ne, ne64, ok) <= 2.5 * TOL_SE


def _random_blocks(M, K, seed):
    """M random K x K information matrices with condition numbers of tens to thousands (A = B B^T / 2K, B [K, 2K] normal, scaled by 10^U(0, 6)),
    P in (0.05, 0.95) and n = 100, with the patterns planted: SNP 0 nobody observes, SNP 1 indefinite (a negated diagonal entry),
    every 11th SNP a fixed component (p = 0), every 13th an unseen one (a zero diagonal entry), SNP 2 with every component fixed."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((M, K, 2 * K))
    A = B @ B.transpose(0, 2, 1) / (2 * K) * (10.0 ** rng.uniform(0, 6, size=M))[:, None, None]
    w = np.linalg.eigvalsh(A)
    cond = w[:, -1] / w[:, 0]                                   # per block, before the patterns are planted
    P = rng.uniform(0.05, 0.95, size=(M, K)).astype(np.float32)
    n = np.full(M, 100, dtype=np.int32)
    n[0] = 0
    A[1, K - 1, K - 1] *= -1.0
    P[np.arange(11, M, 11), rng.integers(0, K, size=len(range(11, M, 11)))] = 0.0
    P[2] = 1.0
    un = np.arange(13, M, 13)
    A[un, un % K, un % K] = 0.0
    ia, ib = np.triu_indices(K)
    return A[:, ia, ib].copy(), P, n, cond


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 4, 7, 8, 13, 16])
def test_the_inversion_kernel_against_the_cpu_route(K):
    """pse.se_from_info on device tensors (nadm_snp_info_se: a thread per SNP) against the same function on CPU tensors (LAPACK) over
    70001 random blocks -- more than the 65536 of one batch, where torch's batched route on the device went wrong -- every kp, K at
    and below it: the NaN pattern, fixed and unseen identical; the values of SNP j within 100 K u cond_j, the textbook forward error
    of a Cholesky solve with a modest constant (u = 2.2e-16; cond_j: the condition number of the SNP's whole block, which bounds
    that of every sub-block left by dropped components; asserted below 1e6)."""
    from neural_admixture_amd import pse
    dev = _dev()
    M = 70001
    info, P, n, cond = _random_blocks(M, K, seed=K)
    assert cond.max() < 1e6
    want = pse.se_from_info(torch.from_numpy(info), P, torch.from_numpy(n))
    got = pse.se_from_info(torch.from_numpy(info).to(dev), P, torch.from_numpy(n).to(dev))
    torch.cuda.synchronize()
    assert got.se.device.type == "cuda" and got.se.dtype == torch.float64 and tuple(got.se.shape) == (M, K)
    s, s64 = got.se.cpu().numpy(), want.se.numpy()
    assert torch.equal(got.fixed.cpu(), want.fixed) and torch.equal(got.unseen.cpu(), want.unseen)
    assert np.array_equal(np.isnan(s), np.isnan(s64))
    assert np.isnan(s[:3]).all() and np.isfinite(s[3:]).mean() > 0.8 and np.isnan(s[11]).sum() == 1
    both = ~np.isnan(s64)
    tol = np.broadcast_to((100 * K * 2.2e-16 * cond)[:, None], s.shape)
    rel = np.abs(s[both] - s64[both]) / s64[both]
    print(f"K={K}: inversion kernel against LAPACK, largest relative deviation {rel.max():.3e}, largest share of its bound "
          f"{(rel / tol[both]).max():.3e} (cond up to {cond.max():.1f})")
    assert (rel <= tol[both]).all()
    assert np.array_equal(np.isnan(got.n_eff.cpu().numpy()), np.isnan(s64))
    again = pse.se_from_info(torch.from_numpy(info).to(dev), P, torch.from_numpy(n).to(dev))
    assert again.se.cpu().numpy().tobytes() == s.tobytes()


@pytest.mark.gpu
def test_engine_p_se_equals_the_library_free_form_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from neural_admixture_amd import pse
    from oracle import nadm_oracle as O
    dev = _dev()
    N, M, ks, Hd, C_ = 96, 3001, [3, 5], 32, 8
    Gm = O.synth_genotypes(N, M, 5, seed=3, missing=0.05)
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, C_)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(sum(ks), M)).astype(np.float32)
    p = O.make_params(42, V0, P0, Hd, ks)
    small = np.concatenate([p.g, p.W1.reshape(-1), p.b1] + [x for h in range(len(ks)) for x in (p.Wk[h].reshape(-1), p.bk[h])])
    bmax = 40                                                                     # rows per encoder batch: three batches
    e = na.Engine(M, C_, Hd, ks, dev, bmax)
    e.load_params(V0, P0, small)
    e.pack_from_host(torch.from_numpy(Gm))
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    for s in (0, 40, 0):
        e.train_step(idx[s:s + bmax], bmax, 2e-3, True)
    e.sync()
    before = [t.clone() for t in (e.pflat, e.mflat, e.vflat)]
    for head in (0, 1):
        Qh = torch.cat([e.infer_q(idx[s:s + bmax], min(bmax, N - s))[head] for s in range(0, N, bmax)], dim=0)
        got = e.p_se(head=head, bound=1e-3)
        want = pse.p_se(e.xp, M, e.P(head).clone(), Qh, bound=1e-3)
        assert all(torch.equal(a.nan_to_num(7.0) if a.dtype.is_floating_point else a, b.nan_to_num(7.0) if b.dtype.is_floating_point else b)
                   for a, b in zip(got, want))
        assert tuple(got.se.shape) == (M, ks[head]) and int(torch.isfinite(got.se).sum()) > M * ks[head] // 2
    with pytest.raises(RuntimeError, match="head must be in 0..1"):
        e.p_se(head=2)
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_pse_end_to_end(tmp_path, caplog):
    """The `pse` mode on a small BED written here (140 samples x 1027 SNPs drawn from the model) with the .P / .Q files of the true
    model for K = 3 and K = 2: the files hold what pse.p_se returns, M x K, and the log lines appear; --extract is honoured."""
    from neural_admixture_amd import cli, pse
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    N, M = 140, 1027
    rng = np.random.default_rng(11)
    ids = [f"snp{j}" for j in range(M)]
    Gm = None
    for K in (3, 2):
        P = rng.uniform(0.05, 0.4, size=(M, K)).astype(np.float32)               # minor alleles: the reader leaves the file unflipped
        Q = rng.dirichlet(np.full(K, 0.5), size=N).astype(np.float32)
        if Gm is None:
            Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0, 1)).astype(np.uint8)
            Gm[rng.random(Gm.shape) < 0.03] = 3
            P[17, 1] = 0.0                                                        # a fixed component: nan in the file
        np.savetxt(tmp_path / f"run.{K}.Q", Q, delimiter=" ")
        np.savetxt(tmp_path / f"run.{K}.P", P, delimiter=" ")
    LO.write_bed(tmp_path / "panel", Gm, ids)
    caplog.set_level(logging.INFO)
    argv = ["--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(tmp_path), "--name", "run"]
    assert cli.main(["pse"] + argv + ["--min_k", "2", "--max_k", "3", "--out_name", "err"]) == 0
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    assert not data.flipped
    for K in (2, 3):
        Pr, Qr = (np.loadtxt(tmp_path / f"run.{K}.{x}", dtype=np.float32, ndmin=2) for x in "PQ")
        res = pse.p_se(data.packed, M, Pr, Qr)
        back = np.loadtxt(tmp_path / f"err.{K}.P_se", dtype=np.float32, ndmin=2)
        assert back.shape == (M, K) and np.array_equal(back, res.se.cpu().numpy().astype(np.float32), equal_nan=True)
        assert np.isfinite(back).mean() > 0.99
    assert np.isnan(np.loadtxt(tmp_path / "err.3.P_se", dtype=np.float32, ndmin=2)[17, 1])
    msgs = [r.getMessage() for r in caplog.records]
    for K in (2, 3):
        assert any(m.startswith(f"P standard errors (K={K}): median SE ") and "median n_eff per component" in m
                   and f"of {M * K} SNP-components" in m and "fixed" in m and "unseen" in m and "NaN" in m for m in msgs)
    assert any("1 fixed, 0 unseen, 1 NaN" in m for m in msgs if "(K=3)" in m)
    assert any("Standard errors of P saved." in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    # --extract: the listed SNPs only, against a .P with one row per listed SNP
    keep = np.zeros(M, dtype=bool)
    keep[5:400:3] = True
    (tmp_path / "list").write_text("".join(f"{s}\n" for s, k in zip(ids, keep) if k))
    ext = ["pse"] + argv + ["--k", "2", "--extract", str(tmp_path / "list"), "--out_name", "sub"]
    with pytest.raises(SystemExit, match=rf"run\.2\.P holds a {M} x 2 matrix, the model needs {int(keep.sum())} x 2"):
        cli.main(ext)
    full = np.loadtxt(tmp_path / "err.2.P_se", dtype=np.float32, ndmin=2)
    np.savetxt(tmp_path / "run.2.P", np.loadtxt(tmp_path / "run.2.P", dtype=np.float32, ndmin=2)[keep], delimiter=" ")
    assert cli.main(ext) == 0
    sub = np.loadtxt(tmp_path / "sub.2.P_se", dtype=np.float32, ndmin=2)
    assert sub.shape == (int(keep.sum()), 2) and np.array_equal(sub, full[keep], equal_nan=True)


@pytest.mark.gpu
def test_train_p_se_end_to_end_on_the_demo(tmp_path, caplog):
    """Train the demo for a few epochs with --polish 2 --p_se, then run the `pse` mode on the written files: both write {name}.3.P_se
    of the .P's shape, equal entry for entry (the mode reads the .P / .Q that train wrote: 18 digits, the same float32), positive
    where finite, and both log the line per K."""
    from neural_admixture_amd import cli
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = np.load(f"{golden}/demo_k3.npz")
    N = int(d["N"])
    d["bed_bytes"].tofile(tmp_path / "demo.bed")
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    assert cli.main(["train", "--epochs", "5", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--polish", "2", "--p_se"]) == 0
    assert cli.main(["pse", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--out_name", "again"]) == 0
    P = np.loadtxt(out / "demo.3.P", ndmin=2)
    a, b = (np.loadtxt(out / f"{name}.3.P_se", ndmin=2) for name in ("demo", "again"))
    assert a.shape == P.shape and np.array_equal(a, b, equal_nan=True)
    assert np.isfinite(a).mean() > 0.1 and (a[np.isfinite(a)] > 0).all()
    assert np.isnan(a[(P <= 1e-4) | (P >= 1 - 1e-4)]).all()
    msgs = [r.getMessage() for r in caplog.records]
    assert len([m for m in msgs if m.startswith("P standard errors (K=3): median SE ")]) == 2
    assert any("Standard errors of P saved." in m for m in msgs)


# ------------------------------------------------------------------------------------------------ the yardsticks, by hand
def _measure_yardsticks():
    """Largest deviation of the float32 restatement from float64 per group of cases, and the two SE yardsticks (CPU only)."""
    def dev_of(b, M, K, kind):
        Gm, P, Q, _ = _case(M, K)
        rows = _rows(b, kind)
        I64, n64 = PO.from_weights(_weights(M, K), Q, rows)
        I, n = PO.info32(Gm[rows], P, Q[rows])
        assert np.array_equal(n, n64) and (I[I64 == 0] == 0).all()
        r = _ratio(I, I64)
        print(f"  b={b} M={M} K={K} rows={kind}: {r:.3e}")
        return r
    for name, cases in (("YARD", CASES), ("YARD_BIG", [(BIG_B, BIG_M, BIG_K, "list")]), ("YARD_DEEP", [(DEEP_B, DEEP_M, DEEP_K, "list")])):
        print(f"{name} = {max(dev_of(*c) for c in cases):.3e}")
    Gm, P, Q, I64, n64, (s64, ne64, fixed64, unseen64, cond) = _planted()
    ok = cond <= COND_CAP
    I32, n32 = PO.info32(Gm, P, Q)
    s32 = PO.se(I32, P, n32)[0]
    assert np.array_equal(np.isnan(s32), np.isnan(s64))
    print(f"YARD_SE = {_rel_se(s32, s64, ok):.3e}   ({ok.mean():.4f} of the SNPs under the condition cap; info32 itself {_ratio(I32, I64):.3e})")
    print(f"YARD_INV = {_rel_se(_se_torch(I64, P, n64)[0], s64, ok):.3e}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # the package, for se_from_info
    _measure_yardsticks()
