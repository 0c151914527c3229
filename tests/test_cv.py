"""Cross-validation over held-out calls (the fold of a call, nadm_cv_mask, nadm_cv_deviance, cv.mask_fold / heldout_deviance /
cv_error, Engine.cv_error, the `cv` mode of the command line and `train --cv`).  The numpy restatements (the fold function in uint64
arithmetic, the float64 truth, the float32 yardstick, the float64 block EM) live in tests/cv_oracle.py; the edge-case data is
hwe_oracle.make_edge_case's.

The tolerance of the deviance against float64 is set as tests/test_hwe.py sets its own: the float32 RESTATEMENT
(cv_oracle.deviance32: fp32 pi with k in order, fp32 log2, fp32 sums in sample order over slices of at most 4096 samples, slices
added in float64) is run on the CPU over the same cases, its largest deviation from float64 is taken per group, and a margin of
8 x covers another summation order, fused multiply-adds and the hardware's 1-ulp v_log_f32.  nheld is an integer: equal.
    |dev - dev64| <= TOL D_abs        (D_abs = sum |d| over the held-out calls of the SNP)
MEASURED with the restatement on the CPU (largest ratio over the cases of a group; per case 3.3e-7 .. 3.9e-6 for 70 <= b <= 200):
    b = 1, M = 257, K = 2              4.234e-05 of D_abs
    CASES + WIDE with 70 <= b <= 200   3.935e-06 of D_abs (b = 130, M = 1027, K = 20)
    b = 4200, M = 257, K = 8           7.153e-06
    b = 12000, M = 3001, K = 8         5.102e-06
so that TOL_ONE = 3.387e-04, TOL = 3.148e-05; at b = 4200 5.722e-05; at b = 12000 4.082e-05.  (The largest ratios belong to SNPs
whose few held-out calls are heterozygotes near pi = 1/2: there d = -2 ln(4 pi (1 - pi)) is small against the 2 log2-units that
cancel in fp32, so a SNP with ONE held-out call -- every SNP of b = 1 -- sets its group's figure; b = 1 is a group of its own so
that it does not widen the others'.)
`python tests/test_cv.py` measures the yardstick again and prints it (CPU only).
OBSERVED on an MI355X: see DESIGN.md section 4.12 (each case prints its ratio before it asserts)."""
import functools
import logging
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv_oracle as CO  # noqa: E402
import hwe_oracle as HO  # noqa: E402
import ld_oracle as LO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

ROWS = 200                   # rows of the edge-case matrix
SEED_WIDE = (1 << 40) + 3    # a seed with bits above 2^32
# (b, M, K, folds, row0): every b, M, K, row0 and number of folds of the issue at least once, not their product
CASES = [(1, 257, 2, 2, 0), (70, 1027, 3, 5, 1000), (130, 3001, 8, 10, 0), (200, 257, 9, 5, 0), (70, 3001, 16, 2, 1000),
         (130, 1027, 20, 10, 1000), (200, 1027, 8, 5, 0), (200, 3001, 3, 2, 0)]
WIDE = [(70, 257, 30, 5, 0), (130, 257, 33, 10, 1000), (70, 1027, 64, 2, 0)]                     # kp = 32, 48, 64
BIG = (4200, 257, 8, 5, 0)                               # the 200 rows repeated: crosses the 4096 samples of one fp32 sum
DEEP = (12000, 3001, 8, 5, 1000)                         # slices of several tiles: the steady state of the tile loop
MARGIN = 8.0
YARD_ONE, YARD, YARD_BIG, YARD_DEEP = 4.234e-05, 3.935e-06, 7.153e-06, 5.102e-06      # measured: module docstring
TOL_ONE, TOL, TOL_BIG, TOL_DEEP = MARGIN * YARD_ONE, MARGIN * YARD, MARGIN * YARD_BIG, MARGIN * YARD_DEEP
MASK_SHAPES = [(1, 257), (70, 1027), (200, 3001)]
MASK_DRAWS = [(2, 0, 0), (5, 42, 0), (10, SEED_WIDE, 1000)]                       # (folds, seed, row0)


# ------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS rows with the planted cases of hwe_oracle.make_edge_case; the tests leave them as they are."""
    return HO.make_edge_case(ROWS, M, K)


@functools.lru_cache(maxsize=None)
def _terms(M, K):
    Gm, P, Q, _ = _case(M, K)
    return CO.terms(Gm, P, Q)


def _draw(b, M, folds, row0):
    """(seed, fold) of a deviance case: the wide seed where the rows start at 1000, a fold that moves with the shape."""
    return (SEED_WIDE if row0 else 42), (b + M) % folds


def _want(b, M, K, folds, row0):
    """The float64 truth of a case over the matrix of b rows that repeats the edge case's ROWS rows: (dev, nheld, D_abs)."""
    Gm, _, _, _ = _case(M, K)
    seed, fold = _draw(b, M, folds, row0)
    F = CO.folds_of(seed, row0 + np.arange(b), M, folds)
    if b <= ROWS:
        return CO.from_terms(_terms(M, K)[:b], Gm[:b], F, fold)
    return CO.from_terms(_terms(M, K), Gm, F, fold, period=ROWS)


def _unpack(xp, M):
    a = np.asarray(xp)
    return np.stack([(a >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(a.shape[0], -1)[:, :M]


@functools.lru_cache(maxsize=None)
def _panel():
    return CO.make_panel(3)


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_reproduces_the_known_answers_of_the_fold_function():
    assert [int(x) for x in CO.mix32([0, 1, 2, 0xFFFFFFFF])] == [0x0, 0x688990C0, 0xD1132181, 0x6768824A]
    table = {(0, 5, 0): ["3 3 0 2 0 1 4 1 1 4 4 1", "2 3 2 3 0 2 1 0 4 0 1 3", "2 1 3 3 3 1 0 0 2 1 1 4"],
             (42, 5, 0): ["0 0 4 4 0 0 3 1 3 2 4 2", "4 2 3 3 3 0 2 2 2 2 2 0", "0 1 1 0 3 3 0 2 4 1 1 4"],
             (SEED_WIDE, 10, 1000): ["3 2 7 3 5 2 7 9 6 7 2 1", "9 4 6 2 5 0 5 5 7 0 3 9", "6 6 5 9 8 9 2 9 2 6 8 8"]}
    for (seed, folds, row0), rows in table.items():
        F = CO.folds_of(seed, row0 + np.arange(3), 12, folds)
        assert F.dtype == np.uint8 and [" ".join(str(v) for v in r) for r in F.tolist()] == rows


@pytest.mark.parametrize("rows, M, folds, seed", [(200, 3001, 5, 0), (200, 3001, 5, 42), (130, 1027, 10, 7), (70, 257, 2, SEED_WIDE),
                                                  (4200, 257, 5, 1)])
def test_fold_shares_of_rows_snps_and_row_pairs(rows, M, folds, seed):
    """Every fold's share of every row and of every SNP, and the share of SNPs at which two rows agree (300 random pairs), lie
    within 6 binomial sigma of 1 / folds (measured over the five cases: at most 4.62, 4.60 and 3.96 sigma)."""
    F = CO.folds_of(seed, np.arange(rows), M, folds)
    p = 1.0 / folds
    assert F.max() == folds - 1 and F.min() == 0
    worst = []
    for axis, n in ((1, M), (0, rows)):                      # a row's share over its SNPs, a SNP's share over the rows
        z = max(float(np.abs((F == f).mean(axis=axis) - p).max()) for f in range(folds)) / math.sqrt(p * (1 - p) / n)
        worst.append(z)
    rng = np.random.default_rng(rows + M)
    a, b = rng.integers(0, rows, size=300), rng.integers(0, rows, size=300)
    a, b = a[a != b], b[a != b]
    worst.append(float(np.abs((F[a] == F[b]).mean(axis=1) - p).max()) / math.sqrt(p * (1 - p) / M))
    print(f"rows={rows} M={M} folds={folds} seed={seed}: largest deviations {worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f} sigma")
    assert max(worst) <= 6.0


def test_deviance_on_a_case_worked_out_by_hand():
    """Three samples, three SNPs, K = 2, two folds, seed 4.  Q_a = (1, 0), Q_b = (1/2, 1/2), Q_c = (0, 1); P = (1/2, 1/2),
    (1/4, 3/4), (0, 1/4).
        pi_a = 1/2, 1/4, 0        pi_b = 1/2, 1/2, 1/8      pi_c = 1/2, 3/4, 1/4
        g_a  = 2, 1, 2            g_b  = 1, missing, 0      g_c  = 0, 2, 2
        fold_a = 1, 0, 0          fold_b = 0, 1, 0          fold_c = 0, 1, 1
    Fold 0 holds a at SNPs 1 and 2, b at SNPs 0 and 2, c at SNP 0:
        SNP 0: b is a heterozygote at pi = 1/2: exactly 0; c: g = 0 at pi = 1/2: -4 ln(1/2) = 4 ln 2.          dev = 4 ln 2, nheld = 2
        SNP 1: a: g = 1 at pi = 1/4: -2 ln(3/16) - 4 ln 2 = -2 ln(3/4).                                       dev = -2 ln(3/4), nheld = 1
        SNP 2: a: g = 2 where pi = 0, the impossible call: -4 ln eps, finite; b: g = 0 at pi = 1/8: -4 ln(7/8).  nheld = 2
    Fold 1 holds a at SNP 0 (g = 2 at 1/2: 4 ln 2), b at SNP 1 (missing: nothing), c at SNP 1 (g = 2 at 3/4: -4 ln(3/4)) and at
    SNP 2 (g = 2 at 1/4: 8 ln 2): nheld = 1, 1, 1.  Tolerances relative to max(1, |x|): 1e-15 in float64, 1e-6 in float32."""
    Gm = np.asarray([[2, 1, 2], [1, 3, 0], [0, 2, 2]], dtype=np.uint8)
    Q = np.asarray([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], dtype=np.float32)
    P = np.asarray([[0.5, 0.5], [0.25, 0.75], [0.0, 0.25]], dtype=np.float32)
    F = CO.folds_of(4, np.arange(3), 3, 2)
    assert F.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 1]]
    ln, eps = math.log, float(np.float32(1e-6))
    want = {0: ([4 * ln(2), -2 * ln(0.75), -4 * ln(eps) - 4 * ln(0.875)], [2, 1, 2]),
            1: ([4 * ln(2), -4 * ln(0.75), 8 * ln(2)], [1, 1, 1])}
    for fold, (dev_w, n_w) in want.items():
        d64, n64, dabs = CO.deviance(Gm, P, Q, F, fold)
        d32, n32 = CO.deviance32(Gm, P, Q, F, fold)
        assert np.array_equal(n64, n_w) and np.array_equal(n32, n_w)
        assert np.allclose(d64, dev_w, rtol=1e-15, atol=1e-15) and np.allclose(dabs, dev_w, rtol=1e-15, atol=1e-15)
        assert np.allclose(d32, dev_w, rtol=1e-6, atol=1e-6)
    t = CO.terms(Gm, P, Q)
    assert t[1, 0] == 0.0 and t[1, 1] == 0.0 and np.isfinite(t).all() and abs(t[0, 2] + 4 * ln(eps)) <= 1e-13
    only_b = CO.deviance32(Gm[1:2], P, Q[1:2], F[1:2], 0)                  # the heterozygote at pi = 1/2 alone: exactly 0 in float32 too
    assert only_b[0][0] == 0.0 and only_b[1][0] == 1
    masked = CO.mask_genotypes(Gm, F, 0)
    assert masked.tolist() == [[2, 3, 3], [3, 3, 3], [3, 2, 2]]


def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_cv_mask", "nadm_cv_deviance", "nadm_cv_deviance_slices", "nadm_cv_deviance_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "0x7FEB352D" in header and "0x846CA68B" in header and "0x9E3779B9" in header


def test_slices_and_scratch_follow_the_sweep_rule():
    """The deviance shares the sweep of nadm_snp_hwe: the same slices, and two scratch words per (slice, SNP) where that has four."""
    from neural_admixture_amd._lib import lib
    for b in (1, 64, 65, 130, 4097, 100000):
        for M in (1, 256, 257, 3001, 500000):
            s = int(lib.nadm_cv_deviance_slices(b, M))
            assert s == int(lib.nadm_snp_hwe_slices(b, M)) >= 1
            f = int(lib.nadm_cv_deviance_scratch_floats(b, M))
            assert 2 * f == int(lib.nadm_snp_hwe_scratch_floats(b, M)) and f >= s * ((M + 255) // 256) * 256 * 2
    for bad in ((0, 100), (-1, 100), (4, 0), (4, -5)):
        assert int(lib.nadm_cv_deviance_slices(*bad)) == 0 and int(lib.nadm_cv_deviance_scratch_floats(*bad)) == 0


def _mask_args():
    xp, xo = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros((4, 16), dtype=torch.uint8)
    return dict(xp=xp.data_ptr(), ld=16, rows=4, row0=0, M=50, seed=0, folds=5, fold=0, xo=xo.data_ptr(), stream=None), (xp, xo)


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(xo=None), "null pointer"), (dict(rows=0), "empty block"), (dict(M=0), "empty block"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"),
    (dict(row0=-1), "row0 + rows <= 2^31"), (dict(row0=(1 << 31) - 3), "row0 + rows <= 2^31"), (dict(M=(1 << 31) + 1, ld=1 << 30), "M must be <= 2^31"),
    (dict(folds=1), "folds must be in 2..NADM_CV_MAX_FOLDS"), (dict(folds=65), "folds must be in 2..NADM_CV_MAX_FOLDS"),
    (dict(fold=5), "fold must be in 0..folds-1"), (dict(fold=-1), "fold must be in 0..folds-1"),
    (dict(unaligned="xp"), "16-byte aligned"), (dict(unaligned="xo"), "16-byte aligned"), (dict(overlap=16), "overlaps"),
])
def test_cv_mask_refuses_before_any_launch(change, message):
    """Every refusal of nadm_cv_mask is decided on the host: it is reported with its message on a machine without a GPU."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _mask_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "overlap" in change:
        big = torch.zeros((8, 16), dtype=torch.uint8)
        base = (big.data_ptr() + 15) // 16 * 16
        a.update(xp=base, xo=base + change["overlap"], rows=2)
        keep = keep + (big,)
    else:
        a.update(change)
    status = lib.nadm_cv_mask(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_cv_mask"):
        check(status, "cv_mask")
    del keep


def _dev_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q, P = torch.full((4, 4), 0.25), torch.full((50, 4), 0.25)
    dev, nheld, scratch = torch.empty(50, dtype=torch.float64), torch.empty(50, dtype=torch.int32), torch.empty(2 * 256)
    a = dict(xp=xp.data_ptr(), ld=16, b=4, row0=0, M=50, Q=Q.data_ptr(), q_stride=4, k=3, kp=4, P=P.data_ptr(), eps=1e-6, seed=0, folds=5,
             fold=0, dev=dev.data_ptr(), nheld=nheld.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, (xp, Q, P, dev, nheld, scratch)


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(P=None), "null pointer"), (dict(dev=None), "null pointer"),
    (dict(nheld=None), "null pointer"), (dict(scratch=None), "null pointer"), (dict(b=0), "empty block"), (dict(M=0), "empty block"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(q_stride=3), "q_stride < kp"),
    (dict(q_stride=6), "q_stride must be a multiple of 4"), (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"),
    (dict(row0=-1), "row0 + rows <= 2^31"), (dict(row0=(1 << 31) - 3), "row0 + rows <= 2^31"),
    (dict(folds=1), "folds must be in 2..NADM_CV_MAX_FOLDS"), (dict(folds=65), "folds must be in 2..NADM_CV_MAX_FOLDS"),
    (dict(fold=5), "fold must be in 0..folds-1"),
    (dict(unaligned="xp"), "16-byte aligned"), (dict(unaligned="Q"), "16-byte aligned"), (dict(unaligned="P"), "16-byte aligned"),
    (dict(unaligned="scratch"), "16-byte aligned"), (dict(unaligned="dev"), "8-byte"), (dict(unaligned2="nheld"), "4-byte"),
])
def test_cv_deviance_refuses_before_any_launch(change, message):
    from neural_admixture_amd._lib import lib, check
    a, keep = _dev_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "unaligned2" in change:
        a[change["unaligned2"]] += 2
    else:
        a.update(change)
    status = lib.nadm_cv_deviance(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_cv_deviance"):
        check(status, "cv_deviance")
    del keep


def test_python_layer_checks_its_arguments_without_a_gpu():
    from neural_admixture_amd import cv
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    for kw, msg in ((dict(fold=0, folds=1), "folds must be in 2..64"), (dict(fold=5, folds=5), r"fold must be in 0..4"),
                    (dict(fold=0, folds=5, seed=-1), "seed must be in"), (dict(fold=0, folds=5, row0=-2), "row0 must be >= 0")):
        with pytest.raises(RuntimeError, match=msg):
            cv.mask_fold(xp, 50, **{"seed": 0, **kw})
    with pytest.raises(RuntimeError, match="must be on a ROCm GPU"):
        cv.mask_fold(xp, 50, 0, 5, 0)
    with pytest.raises(RuntimeError, match="rounds must be >= 1"):
        cv.cv_error(xp, 50, [np.zeros((50, 2))], [np.zeros((4, 2))], rounds=0)
    with pytest.raises(RuntimeError, match="one P and one Q per head"):
        cv.cv_error(xp, 50, [np.zeros((50, 2))], [])


def test_results_table_best_k_and_log_lines(tmp_path, caplog):
    from neural_admixture_amd import cv
    res = [cv.CvResult(2, 1.1587, 0.0009, [1.15, 1.16], 850000, [30, 28], True),
           cv.CvResult(3, 1.10931234567, 0.0007, [1.10, 1.11], 850000, [12, 30], True),
           cv.CvResult(4, 1.1137, 0.0008, [1.11, 1.12], 850000, [9, 11], False)]
    assert cv.best_k(res) == 3
    cv.write_table(tmp_path / "run.cv", res)
    lines = [ln.split() for ln in (tmp_path / "run.cv").read_text().splitlines()]
    assert [f[0] for f in lines] == ["2", "3", "4"] and [f[3] for f in lines] == ["850000"] * 3 and [f[4] for f in lines] == ["30", "30", "11"]
    assert all(float(f[1]) == r.error and float(f[2]) == r.se and len(f) == 5 for f, r in zip(lines, res))
    caplog.set_level(logging.INFO)
    cv.log_results(res, logging.getLogger("test_cv"))
    msgs = [r.getMessage() for r in caplog.records]
    assert "CV error (K=3): 1.10931" in msgs and "CV error (K=2): 1.15870" in msgs and any("K = 3" in m and "Lowest" in m for m in msgs)
    warn = [m for m in msgs if "--cv_rounds" in m]
    assert len(warn) == 1 and "K = 2, 3" in warn[0] and "optimistic" in warn[0]


def test_cli_cv_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing files end the run with the offender named, before the GPU check (there is no GPU as far as the
    mode can tell) and before a genotype is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    common = ["--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_cv_args(common + ["--k", "3"])
    assert (a.folds, a.cv_rounds, a.cv_tol, a.seed, a.out_name, a.extract, a.threads) == (5, 50, 1e-5, 42, None, None, 1)
    a = cli.parse_train_args(common + ["--k", "3"])
    assert (a.cv, a.cv_rounds, a.cv_tol) == (0, 50, 1e-5)

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    span = ["--min_k", "2", "--max_k", "3"]
    with pytest.raises(SystemExit, match=r"--k cannot be given together with --min_k"):
        cli.main(["cv"] + common + ["--k", "3", "--min_k", "2", "--max_k", "3"])
    with pytest.raises(SystemExit, match=r"provide either --k or both --min_k and --max_k"):
        cli.main(["cv"] + common + ["--min_k", "2"])
    with pytest.raises(SystemExit, match=r"--folds must be in 2..64"):
        cli.main(["cv"] + common + span + ["--folds", "1"])
    with pytest.raises(SystemExit, match=r"--cv_rounds must be >= 1"):
        cli.main(["cv"] + common + span + ["--cv_rounds", "0"])
    with pytest.raises(SystemExit, match=r"--cv_tol must be >= 0"):
        cli.main(["cv"] + common + span + ["--cv_tol", "nan"])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(["cv"] + common[:-1] + [str(tmp_path / "x.pgen")] + span)
    np.savetxt(tmp_path / "run.2.P", np.full((10, 2), 0.5))
    np.savetxt(tmp_path / "run.2.Q", np.full((5, 2), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"run\.3\.P not found"):          # a missing .P for one of several Ks
        cli.main(["cv"] + common + span)
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    bed.write_bytes(bytes(3 + 2 * 10))                                     # N = 5, M = 10
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 9 x 3 matrix, the model needs 10 x 3"):
        cli.main(["cv"] + common + span)
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):             # everything is in order: the GPU check is what is left
        cli.main(["cv"] + common + span)
    assert not list(tmp_path.glob("*.cv"))
    # train --cv: refused in --polish's words, before the GPU check too
    train = ["train"] + common + ["--k", "3", "--cv", "5"]
    with pytest.raises(SystemExit, match=r"--cv is single-GPU: run it with --num_gpus 1"):
        cli.main(train + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--cv ignores labels: it is not available with --pops_path"):
        cli.main(train + ["--pops_path", str(tmp_path / "absent.pop")])
    with pytest.raises(SystemExit, match=r"--cv must be in 2..64"):
        cli.main(["train"] + common + ["--k", "3", "--cv", "1"])
    with pytest.raises(SystemExit, match=r"--cv_rounds must be >= 1"):
        cli.main(train + ["--cv_rounds", "0"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(train)


def test_train_refuses_cv_on_sharded_and_supervised_runs():
    from neural_admixture_amd.train import train
    args = (1, 8, 1e-3, 3, 0, None, torch.device("cpu"))
    with pytest.raises(ValueError, match="cv needs a single-GPU, unsupervised run"):
        train(*args, 2, 8, True, None, None, cv=5)
    with pytest.raises(ValueError, match="cv needs a single-GPU, unsupervised run"):
        train(*args, 1, 8, True, None, ["a", "b"], cv=5)
    with pytest.raises(ValueError, match="cv must be 0 or a number of folds in 2..64"):
        train(*args, 1, 8, True, None, None, cv=1)
    with pytest.raises(ValueError, match="cv_rounds must be >= 1"):
        train(*args, 1, 8, True, None, None, cv=5, cv_rounds=0)


def test_sharded_and_cpu_engines_refuse_cv_error():
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.cv_error is single-GPU"):
        e.cv_error()
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.cv_error needs the HIP engine with its packed matrix resident"):
        e.cv_error(folds=5, rounds=3)


def test_public_names():
    import neural_admixture_amd as na
    for name in ("cv_error", "mask_fold", "heldout_deviance"):
        assert callable(getattr(na, name)) and name in na.__all__


# ------------------------------------------------------------------------------------------------ GPU: the masked copy
@pytest.mark.gpu
@pytest.mark.parametrize("folds, seed, row0", MASK_DRAWS)
@pytest.mark.parametrize("rows, M", MASK_SHAPES)
def test_mask_bytes_partition_and_no_leak(rows, M, folds, seed, row0):
    """Per fold the bytes equal the oracle's exactly (pad bits and tail bytes included, the input packed dirty); in place equals out
    of place; over the folds the blanked sets are disjoint and their union is the observed set; and the copy does not depend on the
    calls it hides: other observed codes at the fold's calls leave it byte-identical."""
    from neural_admixture_amd import cv
    dev = _dev()
    Gm = _case(M, 8)[0][:rows]
    host = _packed(Gm, dirty=True)
    xp = host.to(dev)
    assert np.array_equal(_unpack(host.numpy(), M), Gm) and (rows < 6 or ((Gm[4] == 3).all() and (Gm[5] != 3).sum() == 7))
    F = CO.folds_of(seed, row0 + np.arange(rows), M, folds)
    blanked = np.zeros(Gm.shape, dtype=np.int64)
    for f in range(folds):
        out = cv.mask_fold(xp, M, f, folds, seed, row0=row0)
        got = out.cpu().numpy()
        assert out is not xp and got.tobytes() == CO.mask_packed(host.numpy(), M, seed, folds, f, row0).tobytes()
        assert np.array_equal(_unpack(got, M), CO.mask_genotypes(Gm, F, f))
        blanked += (_unpack(got, M) == 3) & (Gm != 3)
        if f == folds - 1:
            same = xp.clone()
            assert cv.mask_fold(same, M, f, folds, seed, out=same, row0=row0) is same and torch.equal(same, out)
            other = Gm.copy()
            hide = (Gm != 3) & (F == f)
            other[hide] = (Gm[hide] + 1) % 3                                # other observed codes where the fold hides them
            assert hide.any() or rows == 1
            leak = cv.mask_fold(_packed(other, dirty=True).to(dev), M, f, folds, seed, row0=row0)
            assert torch.equal(leak, out)
    assert np.array_equal(blanked, (Gm != 3).astype(np.int64))             # every observed call exactly once
    assert torch.equal(xp.cpu(), host)                                      # the input is as it was


# ------------------------------------------------------------------------------------------------ GPU: the held-out deviance
@functools.lru_cache(maxsize=None)
def _resident(b, M, K):
    """The device matrix of b rows that repeats the edge case's rows, and its Q."""
    Gm, P, Q, _ = _case(M, K)
    rows = np.arange(b) % ROWS
    return _packed(Gm[rows]).to(_dev()), Q[rows]


def _gpu_dev(xp, M, P, Q, fold, folds, seed, row0):
    from neural_admixture_amd import cv
    out = cv.heldout_deviance(xp, M, P, Q, fold, folds, seed, row0=row0)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_dev(got, want, tol, what):
    """nheld equal, |dev - dev64| <= tol D_abs; prints the largest ratio before it asserts."""
    d, n = got
    d64, n64, dabs = want
    err = np.abs(d - d64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(dabs > 0, err / dabs, 0.0)))
    print(f"{what}: max |dev - dev64| / D_abs = {ratio:.3e} (bound {tol:.3e})")
    assert d.dtype == np.float64 and n.dtype == np.int32 and np.isfinite(d).all()
    assert np.array_equal(n, n64)
    assert (err <= tol * dabs).all()
    return ratio


def _run_case(b, M, K, folds, row0, tol):
    from neural_admixture_amd._lib import lib
    Gm, P, Q, dead = _case(M, K)
    seed, fold = _draw(b, M, folds, row0)
    xp, Qb = _resident(b, M, K)
    got = _gpu_dev(xp, M, P, Qb, fold, folds, seed, row0)
    want = _want(b, M, K, folds, row0)
    _check_dev(got, want, tol, f"b={b} M={M} K={K} folds={folds} fold={fold} row0={row0} slices={int(lib.nadm_cv_deviance_slices(b, M))}")
    for j in dead:                                           # the SNPs nobody observes: exactly nothing
        assert got[0][j] == 0.0 and not np.signbit(got[0][j]) and got[1][j] == 0
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, folds, row0", CASES)
def test_deviance_against_float64(b, M, K, folds, row0):
    """nheld equal, dev within the tolerance of the module docstring; every case prints its ratio before it asserts."""
    _run_case(b, M, K, folds, row0, TOL_ONE if b == 1 else TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, folds, row0", WIDE)
def test_the_widest_heads(b, M, K, folds, row0):
    """kp = 32, 48 and 64: they must work, they need not be fast.  The same tolerance."""
    from neural_admixture_amd._lib import lib
    assert int(lib.nadm_pad_k(K)) in (32, 48, 64)
    _run_case(b, M, K, folds, row0, TOL)


@pytest.mark.gpu
def test_more_samples_than_one_fp32_sum_covers():
    """b = 4200 rows (the 200 rows repeated): more than 4096 samples, hence several slices whatever M is."""
    from neural_admixture_amd._lib import lib
    assert int(lib.nadm_cv_deviance_slices(BIG[0], BIG[1])) >= 2
    _run_case(*BIG, TOL_BIG)


@pytest.mark.gpu
def test_slices_of_several_tiles():
    """b = 12000 rows over 12 chunks leave slices of 3 tiles: the tile loop hands the prefetched rows over and the body's row
    counter runs across tiles, from a slice's first row."""
    from neural_admixture_amd._lib import lib
    s = int(lib.nadm_cv_deviance_slices(DEEP[0], DEEP[1]))
    assert s >= 2 and -(-((DEEP[0] + 63) // 64) // s) >= 3
    _run_case(*DEEP, TOL_DEEP)


@pytest.mark.gpu
def test_all_missing_row_impossible_calls_and_the_same_bits_twice():
    dev = _dev()
    M, K, folds, seed = 1027, 8, 5, 42
    Gm, P, Q, dead = _case(M, K)
    xp = _packed(Gm).to(dev)
    for f in range(folds):                                   # sample 4 is all missing: nothing, whatever the fold
        d, n = _gpu_dev(xp[4:5], M, P, Q[4:5], f, folds, seed, 4)
        assert not d.any() and not np.signbit(d).any() and not n.any()
    F = CO.folds_of(seed, np.arange(ROWS), M, folds)
    f = int(F[0, 0])                                         # sample 0 at SNP 0: g = 2 where pi = 0 (P row 0 is exactly 0)
    assert Gm[0, 0] == 2 and (P[0] == 0).all()
    a = _gpu_dev(xp, M, P, Q, f, folds, seed, 0)
    assert np.isfinite(a[0]).all() and a[0][0] >= -4.0 * math.log(1e-6) * (1 - 1e-6)
    b = _gpu_dev(xp, M, P, Q, f, folds, seed, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    dirty = _gpu_dev(_packed(Gm, dirty=True).to(dev), M, P, Q, f, folds, seed, 0)       # the pad bits do not enter
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, dirty))


@pytest.mark.gpu
def test_nheld_is_what_the_mask_hides_and_the_folds_partition_the_observed_calls():
    from neural_admixture_amd import cv, ld
    dev = _dev()
    M, K, folds, seed, row0 = 3001, 3, 10, SEED_WIDE, 1000
    Gm, P, Q, dead = _case(M, K)
    xp = _packed(Gm).to(dev)
    n_obs = ld.snp_counts(xp, M)[:, 0]
    assert np.array_equal(n_obs.cpu().numpy(), (Gm != 3).sum(axis=0))
    total = torch.zeros_like(n_obs)
    for f in range(folds):
        _, nheld = cv.heldout_deviance(xp, M, P, Q, f, folds, seed, row0=row0)
        assert torch.equal(nheld, n_obs - ld.snp_counts(cv.mask_fold(xp, M, f, folds, seed, row0=row0), M)[:, 0])
        total += nheld
    assert torch.equal(total, n_obs)


@pytest.mark.gpu
def test_row_ranges_with_row0_add_up_to_one_call():
    dev = _dev()
    M, K, folds, seed, fold = 1027, 9, 5, 42, 3
    Gm, P, Q, dead = _case(M, K)
    xp = _packed(Gm).to(dev)
    whole = _gpu_dev(xp, M, P, Q, fold, folds, seed, 0)
    lo = _gpu_dev(xp[:130], M, P, Q[:130], fold, folds, seed, 0)
    hi = _gpu_dev(xp[130:], M, P, Q[130:], fold, folds, seed, 130)
    assert np.array_equal(lo[1] + hi[1], whole[1])
    dabs = CO.from_terms(_terms(M, K), Gm, CO.folds_of(seed, np.arange(ROWS), M, folds), fold)[2]
    assert (np.abs(lo[0] + hi[0] - whole[0]) <= 2 * TOL * dabs).all()       # each side within TOL of the truth
    wrong = _gpu_dev(xp[130:], M, P, Q[130:], fold, folds, seed, 0)        # (row0 matters)
    assert not np.array_equal(wrong[1], hi[1])


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_cv_error_finds_the_planted_k_and_agrees_with_the_float64_procedure():
    """The panel of DESIGN.md 4.12 (N = 300, M = 3000, planted K = 3, 5 % missing); fits for K = 2, 3, 4 by project.polish from a
    seeded random start, 150 rounds; cv_error(folds = 5, rounds = 30, tol = 0, seed = 42).  K = 3 has the lowest error; every
    observed call is held out once; the limit and not the tolerance stopped the refits; and the K = 3 error lies within a tenth of
    the float64 oracle's own error(4) - error(3) of the oracle's value (same start, float64 EM, 30 rounds, the same folds)."""
    from neural_admixture_amd import cv, project
    dev = _dev()
    Gm, _, _ = _panel()
    N, M = Gm.shape
    xp = _packed(Gm).to(dev)
    rng = np.random.default_rng(17)
    ks = [2, 3, 4]
    P0 = [rng.uniform(0.1, 0.9, size=(M, k)).astype(np.float32) for k in ks]
    Q0 = [rng.dirichlet(np.ones(k), size=N).astype(np.float32) for k in ks]
    Ps, Qs, _, _, _ = project.polish(xp, M, P0, Q0, 150, 0.0)
    before = [t.clone() for t in Ps + Qs]
    res = cv.cv_error(xp, M, Ps, Qs, folds=5, rounds=30, tol=0.0, seed=42)
    assert all(torch.equal(a, b) for a, b in zip(before, Ps + Qs))
    err = {r.k: r.error for r in res}
    print("cv_error on the GPU: " + ", ".join(f"K={r.k}: {r.error:.5f} +- {r.se:.5f}" for r in res))
    assert [r.k for r in res] == ks and err[3] < err[2] and err[3] < err[4] and cv.best_k(res) == 3
    n_obs = int((Gm != 3).sum())
    for r in res:
        assert r.n_held == n_obs and r.hit_limit and r.rounds_run == [30] * 5 and len(r.per_fold) == 5
        assert abs(r.error - float(np.mean(r.per_fold))) < 1e-3 and 0 < r.se < 0.01
    want = CO.cv_error(Gm, [Ps[1].cpu().numpy(), Ps[2].cpu().numpy()], [Qs[1].cpu().numpy(), Qs[2].cpu().numpy()], 5, 30, 42)
    gap = want[1][0] - want[0][0]
    print(f"float64 oracle: K=3: {want[0][0]:.5f}, K=4: {want[1][0]:.5f}, gap {gap:.5f}; |GPU - oracle| at K=3: {abs(err[3] - want[0][0]):.3e}")
    assert gap > 0 and want[0][2] == n_obs
    assert abs(err[3] - want[0][0]) < 0.1 * gap


@pytest.mark.gpu
def test_engine_cv_error_returns_one_result_per_head_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from oracle import nadm_oracle as O
    dev = _dev()
    N, M, ks, Hd, C_ = 96, 3001, [3, 5], 32, 8
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
    for s in (0, 40, 0):
        e.train_step(idx[s:s + bmax], bmax, 2e-3, True)
    e.sync()
    before = [t.clone() for t in (e.big, e.small, e.pflat, e.mflat, e.vflat, e.xp)]
    res = e.cv_error(folds=2, rounds=3, tol=0.0, seed=1)
    e.sync()
    assert [r.k for r in res] == ks and all(r.n_held == int((Gm != 3).sum()) and r.hit_limit and np.isfinite(r.error) for r in res)
    for t, w in zip((e.big, e.small, e.pflat, e.mflat, e.vflat, e.xp), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_cv_end_to_end(tmp_path, caplog):
    """The `cv` mode on a small BED written here with the .P / .Q files of two fits: the .cv file has one line per K that reads back
    to what cv.cv_error returns, and the log carries ADMIXTURE's own lines."""
    from neural_admixture_amd import cli, cv
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    N, M = 140, 1027
    rng = np.random.default_rng(11)
    P = rng.uniform(0.05, 0.4, size=(M, 3)).astype(np.float32)                # minor alleles: the reader leaves the file unflipped
    Q = rng.dirichlet(np.full(3, 0.5), size=N).astype(np.float32)
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0, 1)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.03] = 3
    LO.write_bed(tmp_path / "panel", Gm, [f"snp{j}" for j in range(M)])
    np.savetxt(tmp_path / "run.3.Q", Q, delimiter=" ")
    np.savetxt(tmp_path / "run.3.P", P, delimiter=" ")
    Q2 = np.stack([Q[:, 0] + Q[:, 1], Q[:, 2]], axis=1)
    np.savetxt(tmp_path / "run.2.Q", Q2 / Q2.sum(axis=1, keepdims=True), delimiter=" ")
    np.savetxt(tmp_path / "run.2.P", np.stack([(P[:, 0] + P[:, 1]) / 2, P[:, 2]], axis=1), delimiter=" ")
    caplog.set_level(logging.INFO)
    argv = ["cv", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(tmp_path), "--name", "run", "--min_k", "2", "--max_k", "3",
            "--folds", "5", "--cv_rounds", "4", "--out_name", "pick"]
    assert cli.main(argv) == 0
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    assert not data.flipped
    mats = [[np.loadtxt(tmp_path / f"run.{k}.{ext}", dtype=np.float32, ndmin=2) for k in (2, 3)] for ext in ("P", "Q")]
    want = cv.cv_error(data.packed, M, mats[0], mats[1], 5, 4, 1e-5, 42)
    lines = [ln.split() for ln in (tmp_path / "pick.cv").read_text().splitlines()]
    assert len(lines) == 2 and [f[0] for f in lines] == ["2", "3"]
    for f, r in zip(lines, want):
        assert float(f[1]) == r.error and float(f[2]) == r.se and int(f[3]) == r.n_held == int((Gm != 3).sum()) and int(f[4]) == max(r.rounds_run)
    msgs = [r.getMessage() for r in caplog.records]
    for r in want:
        assert f"CV error (K={r.k}): {r.error:.5f}" in msgs
    assert any(m.startswith("CV error (K=2): ") for m in msgs) and any(m.startswith("CV error (K=3): ") for m in msgs)
    assert any("Lowest cross-validation error: K = " in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    assert any("--cv_rounds" in m for m in msgs) == any(r.hit_limit for r in want)


@pytest.mark.gpu
def test_cli_train_with_cv_logs_the_error_of_the_written_matrices(tmp_path, caplog):
    """`train --cv 2` on a small BED: after training the log carries `CV error (K=3): x`, and x is what cv.cv_error gives for the
    written .P / .Q (read back as float32) with the run's --seed, --cv_rounds and --cv_tol."""
    from neural_admixture_amd import cli, cv
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    N, M = 200, 1027
    rng = np.random.default_rng(5)
    P = rng.uniform(0.05, 0.4, size=(M, 3)).astype(np.float32)
    Q = rng.dirichlet(np.full(3, 0.5), size=N).astype(np.float32)
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0, 1)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.03] = 3
    LO.write_bed(tmp_path / "panel", Gm)
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    assert cli.main(["train", "--epochs", "2", "--k", "3", "--name", "run", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--cv", "2", "--cv_rounds", "3", "--cv_tol", "0"]) == 0
    msgs = [r.getMessage() for r in caplog.records]
    line = [m for m in msgs if m.startswith("CV error (K=3): ")]
    assert len(line) == 1 and any("--cv_rounds" in m for m in msgs)
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    Pw, Qw = np.loadtxt(out / "run.3.P", dtype=np.float32, ndmin=2), np.loadtxt(out / "run.3.Q", dtype=np.float32, ndmin=2)
    assert not data.flipped
    want = cv.cv_error(data.packed, M, [Pw], [Qw], 2, 3, 0.0, 42)[0]
    assert abs(float(line[0].split(": ")[1]) - want.error) <= 1e-5 and want.n_held == int((Gm != 3).sum())


# ------------------------------------------------------------------------------------------------ the yardstick, by hand
def _measure_yardstick():
    """Largest deviation of the float32 restatement from float64 per group of cases (CPU only)."""
    def dev_of(b, M, K, folds, row0):
        Gm, P, Q, _ = _case(M, K)
        seed, fold = _draw(b, M, folds, row0)
        rows = np.arange(b) % ROWS
        d64, n64, dabs = _want(b, M, K, folds, row0)
        d32, n32 = CO.deviance32(Gm[rows], P, Q[rows], CO.folds_of(seed, row0 + np.arange(b), M, folds), fold)
        assert np.array_equal(n32, n64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = float(np.max(np.where(dabs > 0, np.abs(d32 - d64) / dabs, 0.0)))
        assert (np.abs(d32 - d64)[dabs == 0] == 0).all()
        print(f"  b={b} M={M} K={K} folds={folds} row0={row0}: {r:.3e}")
        return r
    for name, cases in (("b = 1", [c for c in CASES if c[0] == 1]), ("CASES + WIDE with b >= 70", [c for c in CASES + WIDE if c[0] > 1]),
                        ("b = 4200", [BIG]), ("b = 12000", [DEEP])):
        print(f"{name}: YARD = {max(dev_of(*c) for c in cases):.3e}")


if __name__ == "__main__":
    _measure_yardstick()
