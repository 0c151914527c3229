"""Hardy-Weinberg score test given ancestry (nadm_snp_hwe, hwe.snp_hwe_sums / snp_hwe / hwe_keep, Engine.snp_hwe, the `hwe` mode of
the command line).  The numpy restatements (float64 truth, float32 yardstick) and the shared data live in tests/hwe_oracle.py.

The tolerances of the sums against float64 are set as tests/test_project_p.py sets its own: the float32 RESTATEMENT
(hwe_oracle.sums32: fp32 pi with k in order, fp32 divisions, fp32 sums in sample order over slices of at most 4096 samples, slices
added in float64) is run on the CPU over the same cases, its largest deviation from float64 is taken per quantity, and a margin of
8 x covers another summation order, fused multiply-adds and the hardware's 1-ulp reciprocal.  n and Hobs are integers: equal.
    |U - U64| <= TOL_U T_abs        |Hexp - Hexp64| <= TOL_H Hexp64        (T_abs = sum m |t|)
MEASURED with the restatement on the CPU (largest ratio over the cases of a group; per case U 5.9e-8 .. 5.6e-7, Hexp 2.9e-7 .. 7.8e-7):
    CASES + WIDE (b <= 200)    U 5.595e-07 of T_abs (b = 1, M = 257, K = 2, pimin = 0)    Hexp 7.832e-07 of Hexp64 (b = 200, M = 1027, K = 8)
    b = 4200, M = 257, K = 8   U 9.594e-07 (pimin = 0), 6.162e-07 (pimin = 0.05)          Hexp 6.962e-06
    b = 12000, M = 3001, K = 8 U 1.093e-06                                                Hexp 7.891e-06
so that TOL_U = 4.476e-06, TOL_H = 6.266e-06; at b = 4200 7.675e-06 and 5.570e-05; at b = 12000 8.744e-06 and 6.313e-05.  (The two
large shapes are dominated by the restatement's 4096-term fp32 sums; the library's slices are shorter there.)
`python tests/test_hwe.py` measures the yardstick again and prints it (CPU only).
OBSERVED on an MI355X: see DESIGN.md section 4.11 (each case prints its two ratios before it asserts)."""
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
from packed_rows import case_rows, dev as _dev, packed as _packed  # noqa: E402

ROWS = 200                   # resident rows of the GPU cases
_rows = functools.partial(case_rows, resident=ROWS)
# (b, M, K, pimin, rows): every b, M, K and pimin of the issue at least once, not their product.  rows: "list" = a permuted gather
# list with a duplicate, "none" = rows 0..b without a list
CASES = [(1, 257, 2, 0.0, "list"), (70, 1027, 3, 0.05, "none"), (130, 3001, 8, 0.0, "list"), (200, 257, 9, 0.05, "list"),
         (70, 3001, 16, 0.0, "list"), (130, 1027, 20, 0.05, "list"), (200, 1027, 8, 0.0, "none"), (130, 257, 16, 0.05, "none"),
         (200, 3001, 3, 0.0, "list")]
WIDE = [(70, 257, 30, 0.0, "list"), (130, 257, 33, 0.05, "list"), (70, 1027, 64, 0.0, "none")]      # kp = 32, 48, 64
BIG_B, BIG_M, BIG_K = 4200, 257, 8                       # crosses the 4096 samples of one fp32 sum
DEEP_B, DEEP_M, DEEP_K = 12000, 3001, 8                  # slices of several tiles: the steady state of the tile loop
MARGIN = 8.0
YARD_U, YARD_H = 5.595e-07, 7.832e-07                                # CASES + WIDE            (measured: module docstring)
YARD_U_BIG, YARD_H_BIG = 9.594e-07, 6.962e-06                        # b = 4200
YARD_U_DEEP, YARD_H_DEEP = 1.093e-06, 7.891e-06                      # b = 12000
TOL_U, TOL_H = MARGIN * YARD_U, MARGIN * YARD_H
TOL_U_BIG, TOL_H_BIG = MARGIN * YARD_U_BIG, MARGIN * YARD_H_BIG
TOL_U_DEEP, TOL_H_DEEP = MARGIN * YARD_U_DEEP, MARGIN * YARD_H_DEEP


# ------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS resident rows with the planted cases of hwe_oracle.make_edge_case; the tests leave them as they are."""
    return HO.make_edge_case(ROWS, M, K)


@functools.lru_cache(maxsize=None)
def _terms(M, K, pimin):
    Gm, P, Q, _ = _case(M, K)
    return HO.terms(Gm, P, Q, pimin)


@functools.lru_cache(maxsize=None)
def _planted():
    Gm, P, Q, planted = HO.make_planted(0)
    return Gm, P, Q, planted, HO.sums(Gm, P, Q)


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_on_a_case_worked_out_by_hand():
    """Three samples, three SNPs, K = 2.  Q_a = (1, 0), Q_b = (1/2, 1/2), Q_c = (0, 1); P = (1/2, 1/2), (1/4, 3/4), (1/4, 1/4).
        pi_a = 1/2, 1/4, 1/4      pi_b = 1/2, 1/2, 1/4      pi_c = 1/2, 3/4, 1/4
        g_a  = 2, 1, 0            g_b  = 1, missing, 0      g_c  = 0, 2, 2
        t_a  = 1, -1, 1/3         t_b  = -1, -, 1/3         t_c  = 1, 1/3, 3
    SNP 0 (every pi = 1/2: t = +-1, 2 pi (1 - pi) = 1/2): U = 1, n = 3, Hobs = 1, Hexp = 3/2, T_abs = 3; F = 1/3, Z = 1/sqrt 3,
    Fhet = 1 - 1/(3/2) = 1/3 (= F: the two agree where every pi is the same), p = erfc(1/sqrt 6).
    SNP 1: U = -1 + 1/3 = -2/3, n = 2, Hobs = 1, Hexp = 3/8 + 3/8 = 3/4, T_abs = 4/3; F = -1/3, Z = -(2/3)/sqrt 2, Fhet = -1/3.
    SNP 2: U = 1/3 + 1/3 + 3 = 11/3, n = 3, Hobs = 0, Hexp = 3 * 3/8 = 9/8, T_abs = 11/3; F = 11/9, Z = (11/3)/sqrt 3, Fhet = 1.
    With pimin = 0.3 every pi = 1/4 and the 3/4 drop out: SNP 1 keeps b alone, which is missing: n = 0, U = Hexp = 0, Z = F = p =
    Fhet = NaN; SNP 2 likewise n = 0; SNP 0 is as before."""
    from math import erfc, sqrt
    Gm = np.asarray([[2, 1, 0], [1, 3, 0], [0, 2, 2]], dtype=np.uint8)
    Q = np.asarray([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], dtype=np.float32)
    P = np.asarray([[0.5, 0.5], [0.25, 0.75], [0.25, 0.25]], dtype=np.float32)
    for fn in (HO.sums, HO.sums32):
        U, H, n, ho, T = fn(Gm, P, Q)
        Z, F, Fhet, p = HO.stats(U, H, n, ho)
        tol = 1e-15 if fn is HO.sums else 1e-6
        assert np.allclose(U, [1.0, -2 / 3, 11 / 3], rtol=0, atol=tol) and np.allclose(H, [1.5, 0.75, 1.125], rtol=0, atol=tol)
        assert np.array_equal(n, [3, 2, 3]) and np.array_equal(ho, [1, 1, 0]) and np.allclose(T, [3.0, 4 / 3, 11 / 3], rtol=0, atol=tol)
        assert np.allclose(Z, [1 / sqrt(3), -(2 / 3) / sqrt(2), (11 / 3) / sqrt(3)], rtol=0, atol=tol)
        assert np.allclose(F, [1 / 3, -1 / 3, 11 / 9], rtol=0, atol=tol) and np.allclose(Fhet, [1 / 3, -1 / 3, 1.0], rtol=0, atol=tol)
        assert np.allclose(p, [erfc(1 / sqrt(6)), erfc((2 / 3) / 2), erfc((11 / 3) / sqrt(6))], rtol=0, atol=tol)
    U, H, n, ho, T = HO.sums(Gm, P, Q, pimin=0.3)
    Z, F, Fhet, p = HO.stats(U, H, n, ho)
    assert np.array_equal(n, [3, 0, 0]) and np.array_equal(ho, [1, 0, 0]) and np.array_equal(U, [1.0, 0.0, 0.0]) and np.array_equal(H, [1.5, 0.0, 0.0])
    assert Z[0] == 1 / sqrt(3) and np.isnan(Z[1:]).all() and np.isnan(F[1:]).all() and np.isnan(Fhet[1:]).all() and np.isnan(p[1:]).all()


def test_k1_is_the_heterozygosity_estimate():
    """K = 1, Q = 1, P = sum g / 2n: F = U / n equals 1 - Hobs / Hexp to 1e-12 and Hexp = 2 n p (1 - p).  64 samples without a missing
    call, so that the sample frequency s / 128 is a float32 number; SNPs with p outside [0.1, 0.9] are left out (pi away from the clip)."""
    rng = np.random.default_rng(3)
    Gm = rng.binomial(2, rng.uniform(0.2, 0.8, size=400)[None, :], size=(64, 400)).astype(np.uint8)
    P, Q = HO.sample_frequency(Gm)
    ok = (P[:, 0] >= 0.1) & (P[:, 0] <= 0.9)
    assert ok.sum() > 300 and np.array_equal(P[:, 0].astype(np.float64), Gm.sum(axis=0) / 128.0)
    U, H, n, ho, _ = HO.sums(Gm, P, Q)
    Z, F, Fhet, p = HO.stats(U, H, n, ho)
    p64 = P[:, 0].astype(np.float64)
    assert (n == 64).all() and np.array_equal(ho, (Gm == 1).sum(axis=0))
    assert np.abs(H - 2.0 * 64 * p64 * (1.0 - p64))[ok].max() <= 1e-12
    assert np.abs(F - Fhet)[ok].max() <= 1e-12 and np.abs(F - (1.0 - ho / H))[ok].max() <= 1e-12


def test_calibration_and_power_on_the_planted_panel():
    """The statistic itself, float64, true Q and P (rounded to float32), seed 0 of hwe_oracle.make_planted.  Null SNPs: |mean Z| <
    0.05, sd in [0.95, 1.05], at most 2 of 2900 with p < 1e-6.  Planted SNPs (30 % of the heterozygotes recalled as homozygous):
    median Z >= 4.5, median F in [0.25, 0.35].  The plain K = 1 test on the same data is NOT calibrated (Wahlund): null mean Z >= 0.7
    and at least 10 null SNPs with p < 1e-6."""
    Gm, P, Q, planted, (U, H, n, ho, T) = _planted()
    assert Gm.shape == (300, 3000) and planted.sum() == 100 and 0.04 < (Gm == 3).mean() < 0.06
    Z, F, Fhet, p = HO.stats(U, H, n, ho)
    zn = Z[~planted]
    print(f"null: mean Z {zn.mean():.4f}, sd {zn.std():.4f}, p < 1e-6: {(p[~planted] < 1e-6).sum()}; planted: median Z "
          f"{np.median(Z[planted]):.3f}, median F {np.median(F[planted]):.3f}")
    assert len(zn) == 2900 and abs(zn.mean()) < 0.05 and 0.95 <= zn.std() <= 1.05 and (p[~planted] < 1e-6).sum() <= 2
    assert np.median(Z[planted]) >= 4.5 and 0.25 <= np.median(F[planted]) <= 0.35
    P1, Q1 = HO.sample_frequency(Gm)
    Z1, _, _, p1 = HO.stats(*HO.sums(Gm, P1, Q1)[:4])
    print(f"K = 1: null mean Z {Z1[~planted].mean():.4f}, p < 1e-6: {(p1[~planted] < 1e-6).sum()}")
    assert Z1[~planted].mean() >= 0.7 and (p1[~planted] < 1e-6).sum() >= 10


def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_snp_hwe", "nadm_snp_hwe_slices", "nadm_snp_hwe_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14


def test_slices_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    sl, f = lib.nadm_snp_hwe_slices, lib.nadm_snp_hwe_scratch_floats
    bs, Ms = (1, 63, 64, 65, 130, 4096, 4097, 100000), (1, 255, 256, 257, 3001, 500000)
    for b in bs:
        for M in Ms:
            s, tiles, chunks = int(sl(b, M)), (b + 63) // 64, (M + 255) // 256
            assert 1 <= s <= tiles and -(-tiles // s) * 64 <= 4096           # whole tiles, at most 4096 samples in one fp32 sum
            assert int(f(b, M)) >= s * chunks * 256 * 4                      # U, Hexp, n, Hobs per (slice, SNP of a whole chunk)
            assert s == int(sl(b, M))                                        # the same answer twice
    assert int(sl(64, 500000)) == 1 and int(sl(130, 257)) == 3 and int(sl(4097, 500000)) >= 2 and int(sl(100000, 500000)) >= 25
    for b in bs:
        v = [int(f(b, M)) for M in Ms]
        assert v[0] > 0 and all(y >= x for x, y in zip(v, v[1:]))
    for M in Ms:
        v = [int(f(b, M)) for b in bs]
        assert all(y >= x for x, y in zip(v, v[1:]))
    for M in (257, 3001):
        v = [int(f(b, M)) for b in range(1, 9000, 7)]
        assert all(y >= x for x, y in zip(v, v[1:]))
    for b in (70, 4200):                                                     # the wobble of ceil(1024 / chunks) * chunks is not in the size
        v = [int(f(b, M)) for M in range(1, 300000, 251)]
        assert all(y >= x for x, y in zip(v, v[1:]))
    for bad in ((0, 100), (-1, 100), (4, 0), (4, -5)):
        assert int(f(*bad)) == 0 and int(sl(*bad)) == 0


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 4), 0.25)
    P = torch.full((50, 4), 0.25)
    U, Hexp = torch.empty(50, dtype=torch.float64), torch.empty(50, dtype=torch.float64)
    nobs, Hobs = torch.empty(50, dtype=torch.int32), torch.empty(50, dtype=torch.int32)
    scratch = torch.empty(4 * 256)
    keep = (xp, P, Q, U, Hexp, nobs, Hobs, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, Q=Q.data_ptr(), q_stride=4, k=3, kp=4, P=P.data_ptr(), eps=1e-6, pimin=0.0,
             U=U.data_ptr(), Hexp=Hexp.data_ptr(), nobs=nobs.data_ptr(), Hobs=Hobs.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(P=None), "null pointer"), (dict(U=None), "null pointer"),
    (dict(nobs=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(b=0), "empty block"), (dict(b=-3), "empty block"), (dict(M=0), "empty block"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(pimin=-1e-3), "pimin must be in [0, 0.5)"), (dict(pimin=0.5), "pimin must be in [0, 0.5)"), (dict(pimin=float("nan")), "pimin must be in [0, 0.5)"),
    (dict(unaligned="xp"), "must be 16-byte aligned"), (dict(unaligned="Q"), "must be 16-byte aligned"), (dict(unaligned="P"), "must be 16-byte aligned"),
    (dict(unaligned="scratch"), "must be 16-byte aligned"), (dict(unaligned="U"), "8-byte"), (dict(unaligned="Hexp"), "8-byte"),
    (dict(unaligned2="nobs"), "4-byte"), (dict(unaligned2="Hobs"), "4-byte"),
])
def test_snp_hwe_refuses_before_any_launch(change, message):
    """Every refusal of nadm_snp_hwe is decided on the host: it is reported with its message on a machine without a GPU (where a launch
    would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "unaligned2" in change:
        a[change["unaligned2"]] += 2
    else:
        a.update(change)
    status = lib.nadm_snp_hwe(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_snp_hwe"):
        check(status, "snp_hwe")
    del keep


def test_null_hexp_and_hobs_are_not_refused():
    """Hexp = NULL and Hobs = NULL pass every check: a later refusal (here: the q_stride, checked after the pointers) is what comes back."""
    from neural_admixture_amd._lib import lib
    a, keep = _refusal_args()
    a.update(Hexp=None, Hobs=None, q_stride=6)
    assert lib.nadm_snp_hwe(*a.values()) != 0 and "q_stride must be a multiple of 4" in lib.nadm_last_error().decode()
    del keep


def _hand_result():
    from neural_admixture_amd import hwe
    U = torch.tensor([3.0, -12.0, 0.0, 60.0], dtype=torch.float64)
    Hexp = torch.tensor([40.5, 50.0, 0.0, 30.0], dtype=torch.float64)
    n = torch.tensor([100, 144, 0, 100], dtype=torch.int32)
    Hobs = torch.tensor([39, 62, 0, 12], dtype=torch.int32)
    return hwe.stats_from_sums(U, Hexp, n, Hobs)


def test_statistics_keep_list_and_table_on_a_hand_made_result(tmp_path):
    """Z = U / sqrt n = 0.3, -1, NaN, 6; F = U / n; p = erfc(|Z| / sqrt 2).  At alpha = 1e-6 only the last SNP goes (p = 1.97e-9); the SNP
    nobody observes is kept and printed as nan; at alpha = 0.5 the second goes too (p = 0.317)."""
    from math import erfc, sqrt
    from neural_admixture_amd import hwe, ld
    res = _hand_result()
    assert all(t.dtype == torch.float64 for t in (res.Z, res.F, res.Fhet, res.p, res.Hexp)) and res.n.dtype == torch.int32 and res.Hobs.dtype == torch.int32
    assert res.Z.tolist()[:2] == [0.3, -1.0] and res.Z[3] == 6.0 and torch.isnan(res.Z[2]) and torch.isnan(res.F[2]) and torch.isnan(res.p[2])
    assert res.F.tolist()[:2] == [0.03, -12.0 / 144.0] and abs(float(res.Fhet[0]) - (1 - 39 / 40.5)) < 1e-15 and torch.isnan(res.Fhet[2])
    for j in (0, 1, 3):
        assert abs(float(res.p[j]) - erfc(abs(float(res.Z[j])) / sqrt(2.0))) <= 1e-15 * max(1.0, float(res.p[j]))
    assert hwe.hwe_keep(res.p, 1e-6).tolist() == [True, True, True, False]
    assert hwe.hwe_keep(res.p, 0.5, res.n).tolist() == [True, False, True, False]
    assert hwe.hwe_keep(res.p, 1.0, res.n).tolist() == [False, False, True, False] and hwe.hwe_keep(res.p.numpy(), 1e-300).all()
    ids = ["rs1", "rs2", "dead", "rs4"]
    hwe.write_table(tmp_path / "t.hwe", ids, res)
    lines = [ln.split() for ln in (tmp_path / "t.hwe").read_text().splitlines()]
    assert len(lines) == 4 and [f[0] for f in lines] == ids
    assert lines[0][1:3] == ["100", "39"] and lines[2] == ["dead", "0", "0", "0", "nan", "nan", "nan"]
    for j, f in enumerate(lines):
        for got, want in zip(f[3:], (res.Hexp[j], res.F[j], res.Z[j], res.p[j])):
            assert float(got) == float(want) or (got == "nan" and np.isnan(float(want)))
    keep = hwe.hwe_keep(res.p, n=res.n)
    ld.write_id_list(tmp_path / "t.hwe.in", [s for s, k in zip(ids, keep) if k])
    back = ld.read_id_list(tmp_path / "t.hwe.in")
    assert back == ["rs1", "rs2", "dead"] and ld.resolve_ids(ids, back).tolist() == keep.tolist()
    with pytest.raises(RuntimeError, match="one ID per SNP"):
        hwe.write_table(tmp_path / "u.hwe", ids[:3], res)


def test_cli_hwe_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing or misshapen .P / .Q / .bim / .fam / .bed files end the run with the offender named, before the GPU
    check (there is no GPU as far as the mode can tell) and before a genotype is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["hwe", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_hwe_args(base[1:])
    assert (a.pimin, a.alpha, a.out_name, a.threads, a.extract) == (0.0, 1e-6, None, 1, None)
    a = cli.parse_hwe_args(base[1:] + ["--out_name", "o", "--alpha", "0.001", "--pimin", "0.01", "--threads", "4", "--extract", "f"])
    assert (a.out_name, a.alpha, a.pimin, a.threads, a.extract) == ("o", 0.001, 0.01, 4, "f")

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit):
        cli.main(["hwe", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)])               # no --k
    for flag, value, msg in (("--pimin", "0.5", r"--pimin must be in \[0, 0.5\)"), ("--pimin", "-0.1", r"--pimin must be in \[0, 0.5\)"),
                             ("--alpha", "0", r"--alpha must be in \(0, 1\]"), ("--alpha", "1.5", r"--alpha must be in \(0, 1\]"),
                             ("--alpha", "nan", r"--alpha must be in \(0, 1\]")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + [flag, value])
    with pytest.raises(SystemExit, match=r"--k must be in 1..64"):
        cli.main(base[:2] + ["65"] + base[3:])
    with pytest.raises(SystemExit, match=r"not available for VCF input"):
        cli.main(base[:-1] + [str(tmp_path / "x.vcf")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen")])
    with pytest.raises(SystemExit, match=r"run\.3\.P not found"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q not found"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((6, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"x\.bim not found"):
        cli.main(base)
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j + 1}\tA\tG\n" for j in range(9)))
    with pytest.raises(SystemExit, match=r"x\.fam not found"):
        cli.main(base)
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    with pytest.raises(SystemExit, match=r"x\.bed not found"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10 + 1))
    with pytest.raises(SystemExit, match=r"x\.bed does not hold whole SNPs of the 5 samples"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10))                       # N = 5, M = 10; the .bim lists 9
    with pytest.raises(SystemExit, match=r"x\.bim lists 9 SNPs, the \.bed holds 10"):
        cli.main(base)
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j + 1}\tA\tG\n" for j in range(10)))
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 6 x 3 matrix, the data needs 5 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 2), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 5 x 2 matrix, the data needs 5 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 9 x 3 matrix, the model needs 10 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.P", np.full((10, 2), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 2 matrix, the model needs 10 x 3"):
        cli.main(base)
    # --extract: the list is resolved before anything else is read, and the .P then has one row per listed SNP
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    with pytest.raises(SystemExit, match=r"nolist not found"):
        cli.main(base + ["--extract", str(tmp_path / "nolist")])
    (tmp_path / "list").write_text("rs1\nrs77\n")
    with pytest.raises(SystemExit, match=r"SNP ID rs77 of .*list is not in .*x\.bim"):
        cli.main(base + ["--extract", str(tmp_path / "list")])
    (tmp_path / "list").write_text("rs1\nrs7\nrs3\n")
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 3 matrix, the model needs 3 x 3"):
        cli.main(base + ["--extract", str(tmp_path / "list")])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base)
    assert not list(tmp_path.glob("*.hwe*"))
    with pytest.raises(AssertionError, match='Please provide either the argument "train" or "infer"'):
        cli.main(["hardy"])


def test_sharded_and_cpu_engines_refuse_snp_hwe():
    """Engine.snp_hwe is single-GPU and needs the resident matrix; the checks come first, so a stand-in without device state shows them."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.snp_hwe is single-GPU"):
        e.snp_hwe()
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.snp_hwe(0, 0.05)
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.snp_hwe needs the HIP engine with its packed matrix resident"):
        e.snp_hwe()


def test_public_names():
    import neural_admixture_amd as na
    for name in ("snp_hwe", "snp_hwe_sums", "hwe_keep"):
        assert callable(getattr(na, name)) and name in na.__all__


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_sums(xp, M, P, Q, rows, kind, pimin):
    """One call through hwe.snp_hwe_sums -> numpy (U, Hexp, n, Hobs); Q [ROWS, K] are the resident rows' fractions."""
    from neural_admixture_amd import hwe
    if kind == "none":
        out = hwe.snp_hwe_sums(xp[:len(rows)], M, P, Q[:len(rows)], None, pimin)
    else:
        out = hwe.snp_hwe_sums(xp, M, P, Q[rows], torch.from_numpy(rows).to(xp.device), pimin)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_sums(got, want, tol_u, tol_h, what):
    """n and Hobs equal, |U - U64| <= tol_u T_abs, |Hexp - Hexp64| <= tol_h Hexp64; prints the two largest ratios before it asserts."""
    U, H, n, ho = got
    U64, H64, n64, ho64, T = want
    eu, eh = np.abs(U - U64), np.abs(H - H64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ru = float(np.max(np.where(T > 0, eu / T, 0.0)))
        rh = float(np.max(np.where(H64 > 0, eh / H64, 0.0)))
    print(f"{what}: max |U - U64| / T_abs = {ru:.3e} (bound {tol_u:.3e}), max |Hexp - Hexp64| / Hexp64 = {rh:.3e} (bound {tol_h:.3e})")
    assert U.dtype == np.float64 and H.dtype == np.float64 and n.dtype == np.int32 and ho.dtype == np.int32
    assert np.array_equal(n, n64) and np.array_equal(ho, ho64)
    assert (eu <= tol_u * T).all()
    assert (eh <= tol_h * H64).all()
    return ru, rh


def _run_case(b, M, K, pimin, kind, tol_u, tol_h):
    from neural_admixture_amd._lib import lib
    dev = _dev()
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(b, kind)
    want = HO.from_terms(_terms(M, K, pimin), Gm, rows)
    got = _gpu_sums(_packed(Gm).to(dev), M, P, Q, rows, kind, pimin)
    _check_sums(got, want, tol_u, tol_h, f"b={b} M={M} K={K} pimin={pimin} rows={kind} slices={int(lib.nadm_snp_hwe_slices(b, M))}")
    for j in dead:                                           # the SNPs nobody observes: exactly nothing
        assert got[0][j] == 0.0 and got[1][j] == 0.0 and got[2][j] == 0 and got[3][j] == 0
        assert not np.signbit(got[0][j]) and not np.signbit(got[1][j])
    if pimin > 0 and b > 2:                                  # the mask did drop calls
        assert (want[2] < np.bincount(rows, minlength=ROWS) @ (Gm != 3).astype(np.int64)).any()
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, pimin, kind", CASES)
def test_sums_against_float64(b, M, K, pimin, kind):
    """n and Hobs equal, U and Hexp within the tolerances of the module docstring; every case prints its two ratios before it asserts."""
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(b, kind)
    if kind == "list" and b > 2:
        assert Q[rows].max(axis=1).max() == 1.0 and (Gm[rows] == 3).all(axis=1).any() and ((Gm[rows] != 3).sum(axis=1) == 7).any()
        assert rows[-1] == rows[0] and len(set(rows.tolist())) == b - 1 and (P[0] == 0).all() and (P[1] == 1).all()
    _run_case(b, M, K, pimin, kind, TOL_U, TOL_H)


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, pimin, kind", WIDE)
def test_the_widest_heads(b, M, K, pimin, kind):
    """kp = 32, 48 and 64: they must work, they need not be fast.  The same tolerances."""
    from neural_admixture_amd._lib import lib
    assert int(lib.nadm_pad_k(K)) in (32, 48, 64)
    _run_case(b, M, K, pimin, kind, TOL_U, TOL_H)


@pytest.mark.gpu
@pytest.mark.parametrize("pimin", [0.0, 0.05])
def test_more_samples_than_one_fp32_sum_covers(pimin):
    """b = 4200 rows (the resident ones with repeats): more than 4096 samples, hence several slices whatever M is."""
    from neural_admixture_amd._lib import lib
    assert int(lib.nadm_snp_hwe_slices(BIG_B, BIG_M)) >= 2
    _run_case(BIG_B, BIG_M, BIG_K, pimin, "list", TOL_U_BIG, TOL_H_BIG)


@pytest.mark.gpu
def test_slices_of_several_tiles():
    """The steady state of a real call: b = 12000 rows over 12 chunks leave slices of 3 tiles, so that the tile loop hands the
    prefetched rows over, reuses both LDS buffers and accumulates across tiles."""
    from neural_admixture_amd._lib import lib
    s = int(lib.nadm_snp_hwe_slices(DEEP_B, DEEP_M))
    assert -(-((DEEP_B + 63) // 64) // s) >= 3
    _run_case(DEEP_B, DEEP_M, DEEP_K, 0.0, "list", TOL_U_DEEP, TOL_H_DEEP)


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    dev = _dev()
    M, K = 3001, 9
    Gm, P, Q, dead = _case(M, K)
    xp, rows = _packed(Gm).to(dev), _rows(130)
    a = _gpu_sums(xp, M, P, Q, rows, "list", 0.05)
    b = _gpu_sums(xp, M, P, Q, rows, "list", 0.05)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
def test_masked_terms_are_exactly_zero():
    """Ones in the pad bits of every row's last byte (and in the bytes behind it), and another P at the SNPs nobody observes, leave
    every output bit-identical."""
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead = _case(M, K)
    rows = _rows(130)
    clean = _gpu_sums(_packed(Gm).to(dev), M, P, Q, rows, "list", 0.0)
    dirty = _gpu_sums(_packed(Gm, dirty=True).to(dev), M, P, Q, rows, "list", 0.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    assert (Gm[:, dead] == 3).all()
    P2 = P.copy()
    P2[dead[0]] = np.float32(np.nan)
    P2[dead[1]] = 0.731
    other = _gpu_sums(_packed(Gm).to(dev), M, P2, Q, rows, "list", 0.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, other))


@pytest.mark.gpu
def test_without_hexp_and_hobs():
    """Hexp = Hobs = NULL: the same U and n bits."""
    from neural_admixture_amd import project
    from neural_admixture_amd._lib import lib, check, ptr
    dev = _dev()
    M, K = 1027, 3
    Gm, P, Q, dead = _case(M, K)
    xp, rows = _packed(Gm).to(dev), _rows(70)
    full = _gpu_sums(xp, M, P, Q, rows, "list", 0.05)
    Pp = project.pad_P(P, dev)
    Qp = project.pad_Q(Q[rows], len(rows), K, Pp.shape[1], dev)
    idx = torch.from_numpy(rows).to(dev)
    U = torch.empty(M, dtype=torch.float64, device=dev)
    n = torch.empty(M, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.nadm_snp_hwe_scratch_floats(len(rows), M)), dtype=torch.float32, device=dev)
    check(lib.nadm_snp_hwe(ptr(xp), xp.shape[1], ptr(idx), len(rows), M, ptr(Qp), Qp.stride(0), K, Pp.shape[1], ptr(Pp), 1e-6, 0.05,
                           ptr(U), None, ptr(n), None, ptr(scratch), project._stream()), "snp_hwe")
    torch.cuda.synchronize()
    assert U.cpu().numpy().tobytes() == full[0].tobytes() and n.cpu().numpy().tobytes() == full[2].tobytes()


@pytest.mark.gpu
def test_planted_panel_on_the_gpu():
    """hwe.snp_hwe on the planted panel packed with the project's packer: Z within 8 TOL_U T_abs / sqrt n of the oracle's, and the set
    removed at alpha = 1e-6 is the oracle's but for SNPs whose oracle p lies within a factor 1.001 of alpha (at most 3 of them)."""
    from neural_admixture_amd import hwe
    dev = _dev()
    Gm, P, Q, planted, (U64, H64, n64, ho64, T) = _planted()
    Z64, F64, Fhet64, p64 = HO.stats(U64, H64, n64, ho64)
    res = hwe.snp_hwe(_packed(Gm).to(dev), Gm.shape[1], P, Q)
    assert all(t.dtype == torch.float64 and t.device.type == "cuda" for t in (res.Z, res.F, res.Fhet, res.p, res.Hexp))
    Z, F, Fhet, p = (t.cpu().numpy() for t in (res.Z, res.F, res.Fhet, res.p))
    assert np.array_equal(res.n.cpu().numpy(), n64) and np.array_equal(res.Hobs.cpu().numpy(), ho64) and (n64 > 0).all()
    err, bound = np.abs(Z - Z64), 8.0 * TOL_U * T / np.sqrt(n64)
    print(f"planted panel: max |Z - Z64| = {err.max():.3e}, largest share of its bound {np.max(err / bound):.3e}; max |F - F64| = {np.abs(F - F64).max():.3e}")
    assert (err <= bound).all()
    assert (np.abs(p - p64) <= bound).all()                  # |dp / dZ| = sqrt(2 / pi) exp(-Z^2 / 2) < 1
    alpha = 1e-6
    keep, keep64 = hwe.hwe_keep(res.p, alpha, res.n), p64 >= alpha
    edge = (p64 > alpha / 1.001) & (p64 < alpha * 1.001)
    assert int(edge.sum()) <= 3
    assert np.array_equal(keep[~edge], keep64[~edge])
    assert (~keep)[~planted].sum() <= 2 and (~keep)[planted].sum() == (~keep64)[planted].sum() > 0


@pytest.mark.gpu
def test_engine_snp_hwe_equals_the_library_free_form_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from neural_admixture_amd import hwe
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
        got = e.snp_hwe(head=head, pimin=0.01)
        want = hwe.snp_hwe(e.xp, M, e.P(head).clone(), Qh, pimin=0.01)
        assert all(torch.equal(a.nan_to_num(7.0) if a.dtype.is_floating_point else a, b.nan_to_num(7.0) if b.dtype.is_floating_point else b)
                   for a, b in zip(got, want))
        seen = got.n > 0
        assert got.Z.shape == (M,) and int(seen.sum()) > M // 2 and bool(torch.isfinite(got.Z[seen]).all()) and bool(torch.isnan(got.Z[~seen]).all())
    with pytest.raises(RuntimeError, match="head must be in 0..1"):
        e.snp_hwe(head=2)
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_hwe_end_to_end(tmp_path, caplog):
    """The `hwe` mode on a small BED written here (140 samples x 1027 SNPs drawn from the model, five SNPs recalled as all-heterozygous)
    with the .P / .Q files of the true model: the table has M lines and holds what hwe.snp_hwe returns, the two lists partition the
    .bim's IDs in file order, and `kinship --extract` takes the .hwe.in once the .P rows are subset."""
    from neural_admixture_amd import cli, hwe, ld
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    N, M, K = 140, 1027, 3
    rng = np.random.default_rng(11)
    P = rng.uniform(0.05, 0.4, size=(M, K)).astype(np.float32)               # minor alleles: the reader leaves the file unflipped
    Q = rng.dirichlet(np.full(K, 0.5), size=N).astype(np.float32)
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0, 1)).astype(np.uint8)
    bad = np.asarray([3, 200, 512, 700, 1026])
    Gm[:, bad] = 1
    Gm[rng.random(Gm.shape) < 0.03] = 3
    ids = [f"snp{j}" for j in range(M)]
    LO.write_bed(tmp_path / "panel", Gm, ids)
    np.savetxt(tmp_path / "run.3.Q", Q, delimiter=" ")
    np.savetxt(tmp_path / "run.3.P", P, delimiter=" ")
    caplog.set_level(logging.INFO)
    argv = ["--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(tmp_path), "--name", "run", "--k", "3"]
    assert cli.main(["hwe"] + argv + ["--out_name", "qc", "--pimin", "0.01"]) == 0
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    assert not data.flipped
    Pr, Qr = np.loadtxt(tmp_path / "run.3.P", dtype=np.float32, ndmin=2), np.loadtxt(tmp_path / "run.3.Q", dtype=np.float32, ndmin=2)
    res = hwe.snp_hwe(data.packed, M, Pr, Qr, pimin=0.01)
    lines = [ln.split() for ln in (tmp_path / "qc.3.hwe").read_text().splitlines()]
    assert len(lines) == M and [f[0] for f in lines] == ids and all(len(f) == 7 for f in lines)
    assert [int(f[1]) for f in lines] == res.n.tolist() and [int(f[2]) for f in lines] == res.Hobs.tolist()
    for col, t in ((3, res.Hexp), (4, res.F), (5, res.Z), (6, res.p)):
        assert np.array_equal(np.asarray([float(f[col]) for f in lines]), t.cpu().numpy(), equal_nan=True)
    kept, gone = ld.read_id_list(tmp_path / "qc.3.hwe.in"), ld.read_id_list(tmp_path / "qc.3.hwe.out")
    want = hwe.hwe_keep(res.p, 1e-6, res.n)
    assert kept == [s for s, k in zip(ids, want) if k] and gone == [s for s, k in zip(ids, want) if not k]
    assert set(ids[j] for j in bad) <= set(gone) and len(gone) <= len(bad) + 2 and len(kept) + len(gone) == M
    msgs = [r.getMessage() for r in caplog.records]
    assert any(f"{M} of {M} SNPs tested, {len(gone)} removed at p < 1e-06" in m for m in msgs)
    assert any("Z over the tested SNPs: median" in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    # the list is in the format --extract expects: the old .P is a .P of the wrong height, the subset .P is taken
    kin = ["kinship"] + argv + ["--extract", str(tmp_path / "qc.3.hwe.in")]
    with pytest.raises(SystemExit, match=rf"run\.3\.P holds a {M} x 3 matrix, the model needs {len(kept)} x 3"):
        cli.main(kin)
    np.savetxt(tmp_path / "run.3.P", Pr[want], delimiter=" ")
    assert cli.main(kin) == 0 and (tmp_path / "run.3.kin").is_file()
    # and `hwe --extract` itself tests the listed SNPs only
    assert cli.main(["hwe"] + argv + ["--extract", str(tmp_path / "qc.3.hwe.in"), "--out_name", "again"]) == 0
    again = (tmp_path / "again.3.hwe").read_text().splitlines()
    assert len(again) == len(kept) and [ln.split()[0] for ln in again] == kept


# ------------------------------------------------------------------------------------------------ the yardstick, by hand
def _measure_yardstick():
    """Largest deviation of the float32 restatement from float64 per group of cases (CPU only)."""
    def dev_of(b, M, K, pimin, kind):
        Gm, P, Q, _ = _case(M, K)
        rows = _rows(b, kind)
        U64, H64, n64, ho64, T = HO.from_terms(_terms(M, K, pimin), Gm, rows)
        U, H, n, ho, _ = HO.sums32(Gm[rows], P, Q[rows], pimin)
        assert np.array_equal(n, n64) and np.array_equal(ho, ho64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ru = float(np.max(np.where(T > 0, np.abs(U - U64) / T, 0.0)))
            rh = float(np.max(np.where(H64 > 0, np.abs(H - H64) / H64, 0.0)))
        print(f"  b={b} M={M} K={K} pimin={pimin} rows={kind}: U {ru:.3e}  Hexp {rh:.3e}")
        return ru, rh
    for name, cases in (("CASES + WIDE", CASES + WIDE), ("b = 4200", [(BIG_B, BIG_M, BIG_K, pm, "list") for pm in (0.0, 0.05)]),
                        ("b = 12000", [(DEEP_B, DEEP_M, DEEP_K, 0.0, "list")])):
        r = [dev_of(*c) for c in cases]
        print(f"{name}: YARD_U = {max(x for x, _ in r):.3e}, YARD_H = {max(y for _, y in r):.3e}")


if __name__ == "__main__":
    _measure_yardstick()
