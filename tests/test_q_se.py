"""Standard errors of Q given P (nadm_sample_info, qse.q_info / se_from_info / q_se, Engine.q_se, the `qse` mode of the command line,
`infer --refine N --q_se` and `train --q_se`).  The numpy restatements (float64 truth, float32 yardstick, both forms of the
constrained inverse, the calibration experiment) live in tests/qse_oracle.py.

The tolerance of the sums against float64 is set as tests/test_p_se.py sets its own: the float32 RESTATEMENT (qse_oracle.info32: fp32
pi with k in order, an fp32 product r u and an fp32 division, fp32 products w p_a and (w p_a) p_b, fp32 sums in SNP order over the
library's ranges, the ranges added in float64) is run on the CPU, its largest relative deviation from float64 is taken, and a margin
of 8 x covers another summation order, fused multiply-adds and the hardware's 1-ulp reciprocal.  n is an integer: equal.  An entry
that is 0 in float64 must be exactly +0.0; otherwise, every term being non-negative,
    |A - A64| <= TOL A64        per entry
MEASURED with the restatement on the CPU (`python tests/test_q_se.py` measures them again and prints them):
    b = 200, M = 4099, K = 8 (the largest case; one chunk per range)   YARD      = 2.180e-07
    b = 70, M = 300000, K = 3 (two chunks per range)                   YARD_LONG = 2.219e-07
    planted panel, SE (info32 through the float64 inversion)           YARD_SE   = 2.232e-06   (the unadmixed samples' differences
                                                                                             of nearly equal sums carry it)
The device's inversion against the CPU's: both are float64 Cholesky factorisations of the same block J, so they differ by round-off
times the block's condition number; allowed per sample: 8 K cond(J) 2^-52 (relative), the measured figure is printed (on an MI355X at K = 2, 3, 8, 16: 0, 1.7e-2, 3.6e-3,
1.1e-3 of the allowed).
Calibration (qse_oracle.calibration, seeds 0, 1, 2; K = 3, 24 samples x 3000 SNPs, Fst 0.1, 5 % missing, 60 panels):
    median SE / spread over interior samples   1.0498, 1.0106, 0.9763      band 0.9763 (1 - 0.09) .. 1.0498 (1 + 0.09): the sampling
                                                                            error of a standard deviation from 60 draws is 9 %
    coverage of |z| < 1.96                     0.9583, 0.9509, 0.9431      band 0.9431 - 3 s .. 0.9583 + 3 s, s = sqrt(.05 x .95 / 1440)
                                                                            = 0.0057 (12 samples x 2 free components x 60 panels)
    unadmixed samples, absent component        SE 0.0281 .. 0.0284 against a spread of the truncated estimate of 0.0119 .. 0.0128
OBSERVED on an MI355X: see DESIGN.md section 4.18 (each case prints its ratio before it asserts)."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qse_oracle as QO  # noqa: E402
from packed_rows import case_rows, dev as _dev  # noqa: E402

ROWS = 210                   # resident rows of the GPU cases
_rows = functools.partial(case_rows, resident=ROWS)
CASES = [(1, 1, 1), (3, 255, 2), (64, 256, 3), (65, 257, 4), (130, 1030, 7), (200, 4099, 8), (70, 2051, 13), (67, 1500, 16)]
LONG_B, LONG_M, LONG_K = 70, 300000, 3                   # more than one chunk per range: the steady state of the chunk loop
MARGIN = 8.0
YARD, YARD_LONG, YARD_SE = 2.180e-07, 2.219e-07, 2.232e-06                 # measured: module docstring
TOL, TOL_LONG, TOL_SE = (MARGIN * y for y in (YARD, YARD_LONG, YARD_SE))
RATIO_BAND = (0.9763 * (1 - 0.09), 1.0498 * (1 + 0.09))
COVER_BAND = (0.9431 - 3 * 0.0057, 0.9583 + 3 * 0.0057)


# ------------------------------------------------------------------------------------------------ shared data
@functools.lru_cache(maxsize=None)
def _case(M, K, rows=ROWS, seed=0):
    """``rows`` resident rows drawn from the model with 10 % of the calls missing; row 2 is one-hot, row 4 has no observed call, row 5
    only among its first forty.  (G uint8 [rows, M], P float32 [M, K], Q float32 [rows, K]); the tests leave them as they are."""
    rng = np.random.default_rng(1000 * K + M + seed)
    P = rng.uniform(0.02, 0.98, size=(M, K)).astype(np.float32)
    Q = rng.dirichlet(np.full(K, 0.7), size=rows).astype(np.float32)
    if rows > 5:
        Q[2] = np.eye(K, dtype=np.float32)[0]
    Gm = rng.binomial(2, np.clip(Q.astype(np.float64) @ P.astype(np.float64).T, 0, 1)).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.10] = 3
    if rows > 5:
        Gm[4] = 3
        Gm[5, 40:] = 3
    return Gm, P, Q


@functools.lru_cache(maxsize=None)
def _truth(M, K, rows=ROWS):
    Gm, P, Q = _case(M, K, rows)
    return QO.info(Gm, P, Q)


def _pack(Gm, extra=16, dirty=True):
    """Packed rows [N, ld] on the host with ld = ceil(M/4) rounded up to 16 PLUS ``extra``; ``dirty``: every bit that holds no SNP set."""
    from neural_admixture_amd._lib import lib, check, ptr
    N, M = Gm.shape
    ld = ((M + 3) // 4 + 15) // 16 * 16 + extra
    out = torch.zeros((N, ld), dtype=torch.uint8)
    check(lib.nadm_pack2bit_host(ptr(torch.from_numpy(np.ascontiguousarray(Gm))), ptr(out), N, M, ld), "pack2bit_host")
    if dirty:
        a = out.numpy()
        a[:, (M + 3) // 4:] = 0xFF
        if M % 4:
            a[:, M // 4] |= (0xFF << (2 * (M % 4))) & 0xFF
    return out


@functools.lru_cache(maxsize=None)
def _planted():
    """One panel of the calibration experiment with the fitted Q: (G, P float32, Q float32, the oracle's float64 info, n, se)."""
    P, Qt, _ = QO.make_panel(0)
    Gm = QO.draw(np.random.default_rng(5), P, Qt)
    P32 = P.astype(np.float32)
    Q32 = QO.project_fit(Gm, P32).astype(np.float32)
    I, n = QO.info(Gm, P32, Q32)
    return Gm, P32, Q32, I, n, QO.se(I, 3, n)


def _ratio(I, I64):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(I64 > 0, np.abs(I - I64) / I64, 0.0)))


def _cpr(b, M):
    from neural_admixture_amd._lib import lib
    chunks = (M + 255) // 256
    return -(-chunks // int(lib.nadm_sample_info_ranges(b, M)))


def _se_cpu(I, Q, n, bound=1e-4):
    from neural_admixture_amd import qse
    r = qse.se_from_info(torch.from_numpy(np.asarray(I, dtype=np.float64)), torch.from_numpy(np.asarray(Q, dtype=np.float32)),
                         torch.from_numpy(np.asarray(n).astype(np.int32)), bound)
    assert r.se.dtype == torch.float64 and r.n.dtype == torch.int32 and r.at_bound.dtype == torch.bool and r.cov is None
    assert r.se.device.type == "cpu"
    return r.se.numpy(), r.at_bound.numpy()


# ------------------------------------------------------------------------------------------------ CPU: hand cases
def test_k1_is_exactly_zero_and_n_is_the_observed_count():
    Gm = np.array([[0, 1, 3, 2, 3], [3, 3, 3, 3, 3], [2, 2, 2, 2, 2]], dtype=np.uint8)
    P, Q = np.full((5, 1), 0.3), np.ones((3, 1))
    I, n = QO.info(Gm, P, Q)
    assert n.tolist() == [3, 0, 5]
    se, at = _se_cpu(I, Q, n)
    assert se[0, 0] == 0.0 and se[2, 0] == 0.0 and np.isnan(se[1, 0]) and at.all()
    assert np.array_equal(QO.se(I, 1, n), se, equal_nan=True)


def test_two_components_three_snps_by_hand():
    """K = 2: the free direction is (1, -1), so both components have SE = 1 / sqrt(sum_j w_j (p_j0 - p_j1)^2)."""
    P = np.array([[0.2, 0.7], [0.5, 0.1], [0.9, 0.4]])
    Q = np.array([[0.3, 0.7]])
    Gm = np.array([[1, 0, 2]], dtype=np.uint8)
    pi = Q @ P.T
    w = 2.0 / (pi * (1 - pi))
    want = 1.0 / np.sqrt((w * (P[:, 0] - P[:, 1]) ** 2).sum())
    I, n = QO.info(Gm, P, Q)
    se, at = _se_cpu(I, Q, n)
    assert np.allclose(se, want, rtol=1e-13, atol=0) and not at.any()
    assert np.allclose(QO.se(I, 2, n), want, rtol=1e-13, atol=0)
    assert np.allclose(QO.se_schur(QO.full(I, 2)[0]), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("K", [2, 3, 8, 16])
def test_schur_form_equals_the_drop_one_form_for_every_c(K):
    from neural_admixture_amd import qse
    rng = np.random.default_rng(K)
    for _ in range(5):
        X = rng.normal(size=(3 * K + 5, K))
        A = X.T @ X + 0.05 * np.eye(K)
        s = QO.se_schur(A)
        for c in range(K):
            d = QO.se_drop(A, c)
            keep = np.arange(K) != c
            assert np.isnan(d[c]) and np.allclose(d[keep], s[keep], rtol=1e-10, atol=0)
        I = np.array([[A[a, b] for a, b in QO.pairs(K)]])
        got, _ = _se_cpu(I, np.full((1, K), 1.0 / K), np.array([7]))
        assert np.allclose(got[0], s, rtol=1e-10, atol=0)
        # drop_one's layout: the a-major pairs of the K - 1 components left
        J = qse.drop_one(torch.from_numpy(I), K, K - 1).numpy()[0]
        keep = list(range(K - 1))
        Jw = (A[np.ix_(keep, keep)] - A[K - 1, keep][None, :]) - (A[keep, K - 1][:, None] - A[K - 1, K - 1])
        assert np.allclose(J, [Jw[a, b] for a, b in QO.pairs(K - 1)], rtol=1e-13, atol=0)


@pytest.mark.parametrize("twins", [(0, 1), (1, 2), (0, 3), (2, 3), (1, 3)])
def test_nan_exactly_where_nothing_is_observed_or_the_block_is_singular(twins):
    """Sample 1 has no observed call; two columns of P are identical in a copy of the panel, which makes every block singular; the
    rest is finite, at the bound included."""
    rng = np.random.default_rng(3)
    M, K = 400, 4
    P = rng.uniform(0.05, 0.95, size=(M, K))
    Q = rng.dirichlet(np.ones(K), size=6)
    Q[2] = [1.0, 0.0, 0.0, 0.0]
    Q[3] = [0.0, 0.5, 0.5 - 5e-5, 5e-5]
    Gm = rng.binomial(2, Q @ P.T).astype(np.uint8)
    Gm[rng.random(Gm.shape) < 0.1] = 3
    Gm[1] = 3
    I, n = QO.info(Gm, P, Q)
    se, at = _se_cpu(I, Q, n)
    assert np.isnan(se[1]).all() and np.isfinite(np.delete(se, 1, axis=0)).all() and (np.delete(se, 1, axis=0) > 0).all()
    assert np.array_equal(at, (Q <= 1e-4) | (Q >= 1 - 1e-4)) and at[2].all() and at[3].tolist() == [True, False, False, True]
    assert np.allclose(se, QO.se(I, K, n), rtol=1e-9, atol=0, equal_nan=True)
    _, at2 = _se_cpu(I, Q, n, bound=0.0)
    assert at2[2].all() and not at2[0].any()
    P2 = P.copy()
    P2[:, twins[1]] = P2[:, twins[0]]
    I2, n2 = QO.info(Gm, P2, Q)
    se2, _ = _se_cpu(I2, Q, n2)
    assert np.isnan(se2).all() and np.isnan(QO.se(I2, K, n2)).all()


def test_calibration_of_the_restated_procedure():
    ratio, coverage, pure_se, pure_spread = QO.calibration(0)
    print(f"median SE / spread {ratio:.4f}, coverage {coverage:.4f}, absent component: SE {pure_se:.4f}, spread {pure_spread:.4f}")
    assert RATIO_BAND[0] <= ratio <= RATIO_BAND[1]
    assert COVER_BAND[0] <= coverage <= COVER_BAND[1]
    assert pure_se > pure_spread


# ------------------------------------------------------------------------------------------------ CPU: host-side checks
def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_sample_info", "nadm_sample_info_ranges", "nadm_sample_info_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "CONDITIONAL on P" in header


def test_ranges_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    rg, f = lib.nadm_sample_info_ranges, lib.nadm_sample_info_scratch_floats
    bs, Ms, kps = (1, 64, 255, 256, 257, 600, 4096, 32768, 100000), (1, 255, 256, 257, 3001, 300000, 600000, 300000000), (4, 8, 12, 16)
    for b in bs:
        for M in Ms:
            r, tiles, chunks = int(rg(b, M)), (b + 255) // 256, (M + 255) // 256
            assert 1 <= r <= chunks and -(-chunks // r) <= 1024                                  # no fp32 sum over more than 2^18 SNPs
            want = max(min(-(-1024 // tiles), chunks), -(-chunks // 1024))                       # the split rule, restated
            assert r == -(-chunks // -(-chunks // want))
            for kp in kps:
                assert int(f(b, M, kp)) >= r * tiles * 256 * (kp * (kp + 1) // 2 + 1)            # the slabs the launch writes
            v = [int(f(b, M, kp)) for kp in kps]
            assert v[0] > 0 and all(y > x for x, y in zip(v, v[1:]))                             # grows with kp
    for kp in kps:
        for b in bs:
            v = [int(f(b, M, kp)) for M in Ms]
            assert all(y >= x for x, y in zip(v, v[1:]))
        for M in Ms:
            v = [int(f(b, M, kp)) for b in bs]
            assert all(y >= x for x, y in zip(v, v[1:]))
    # the block rule of qse.q_info: 32768 rows at M = 600k, K = 8 stay below 0.2 GB
    assert int(f(32768, 600000, 8)) * 4 <= 0.2 * 1024 ** 3
    for bad in ((0, 100, 4), (-1, 100, 4), (4, 0, 4), (4, -5, 4), (4, 100, 0), (4, 100, 6), (4, 100, 24), (4, 100, 64)):
        assert int(f(*bad)) == 0
    assert int(rg(0, 100)) == 0 and int(rg(4, 0)) == 0


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 24), 0.25)
    P = torch.full((50, 24), 0.25)
    info = torch.empty(4 * 6, dtype=torch.float64)
    nobs = torch.empty(4, dtype=torch.int32)
    scratch = torch.empty(256 * 11)
    keep = (xp, P, Q, info, nobs, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, P=P.data_ptr(), k=3, kp=4, Q=Q.data_ptr(), q_stride=24, eps=1e-6,
             info=info.data_ptr(), nobs=nobs.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(P=None), "null pointer"), (dict(info=None), "null pointer"),
    (dict(nobs=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(b=0), "empty batch"), (dict(b=-3), "empty batch"), (dict(M=0), "empty batch"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(k=17, kp=24), "K must be <= 16"), (dict(k=64, kp=64, q_stride=64), "K must be <= 16"),
    (dict(unaligned="xp"), "must be 16-byte aligned"), (dict(unaligned="Q"), "must be 16-byte aligned"), (dict(unaligned="P"), "must be 16-byte aligned"),
    (dict(unaligned="scratch"), "must be 16-byte aligned"), (dict(unaligned="info"), "8-byte"), (dict(unaligned2="nobs"), "4-byte"),
])
def test_sample_info_refuses_before_any_launch(change, message):
    """Every refusal of nadm_sample_info is decided on the host: it is reported with its message on a machine without a GPU (where a
    launch would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    elif "unaligned2" in change:
        a[change["unaligned2"]] += 2
    else:
        a.update(change)
    status = lib.nadm_sample_info(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_sample_info"):
        check(status, "sample_info")
    del keep


def test_python_layer_refuses_a_wide_head_and_a_bad_row_block_in_words():
    from neural_admixture_amd import qse
    xp = torch.zeros((4, 16), dtype=torch.uint8)                     # (a CPU tensor: the refusals come before it is looked at)
    with pytest.raises(RuntimeError, match="K must be <= 16 for standard errors of Q"):
        qse.q_info(xp, 50, np.full((50, 17), 0.5, dtype=np.float32), np.full((4, 17), 1 / 17, dtype=np.float32))
    for rb in (0, 100, -256, 64):
        with pytest.raises(RuntimeError, match="row_block must be a positive multiple of 256"):
            qse.q_info(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None, row_block=rb)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        qse.q_info(xp, 50, np.full((50, 3), 0.5, dtype=np.float32), None)
    with pytest.raises(RuntimeError, match=r"bound must be in \[0, 0.5\)"):
        qse.se_from_info(torch.zeros((2, 1), dtype=torch.float64), np.ones((2, 1)), torch.ones(2, dtype=torch.int32), bound=0.5)
    with pytest.raises(RuntimeError, match=r"info must be \[2, 3\]"):
        qse.se_from_info(torch.zeros((2, 2), dtype=torch.float64), np.full((2, 2), 0.5), torch.ones(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="K must be <= 16 for standard errors of Q"):
        qse.se_from_info(torch.zeros((2, 153), dtype=torch.float64), np.full((2, 17), 1 / 17), torch.ones(2, dtype=torch.int32))


def test_writer_round_trips_nan_included_and_the_log_names_the_least_certain(tmp_path, caplog):
    from neural_admixture_amd import qse
    se = torch.tensor([[0.125, 0.25, 3.0e-4], [float("nan"), float("nan"), float("nan")], [0.5, 0.03125, 0.01], [0.01, 0.02, 0.03]],
                      dtype=torch.float64)
    se[1, 1] = -se[1, 1]                                         # whatever NaN it is, the file says `nan`
    res = qse.QseResult(se, torch.tensor([40, 0, 9, 3000], dtype=torch.int32), torch.zeros((4, 3), dtype=torch.bool).index_put_(
        (torch.tensor([3]), torch.tensor([0])), torch.tensor(True)))
    qse.write_results(tmp_path, "r", [res])
    text = (tmp_path / "r.3.Q_info_se").read_text()
    rows = [ln.split(" ") for ln in text.splitlines()]
    assert len(rows) == 4 and all(len(r) == 3 for r in rows) and rows[1] == ["nan", "nan", "nan"]
    assert rows[0][0] == "1.250000000000000000e-01"              # the .Q text format
    back = np.loadtxt(tmp_path / "r.3.Q_info_se", dtype=np.float32, ndmin=2)
    assert np.array_equal(back, se.numpy().astype(np.float32), equal_nan=True)
    assert not list(tmp_path.glob("*.Q_se"))
    with pytest.raises(RuntimeError, match="must be a matrix"):
        qse.write_se(tmp_path / "bad", torch.zeros(3))
    caplog.set_level(logging.INFO)
    qse.log_results([res], logging.getLogger("t"))
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("Q standard errors given P (K=3): median SE 0.03000;") and "of 4 samples 2 have an SE above 0.1" in m
               and "of 12 entries 1 at the bound" in m and "3 NaN" in m for m in msgs)
    assert any("least certain samples" in m and m.rstrip().endswith("2: 0.500, 9, 0: 0.250, 40") for m in msgs)


def test_cli_qse_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing or misshapen files end the run with the offender named, before the GPU check and before a genotype
    is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["qse", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_qse_args(base[1:] + ["--k", "3"])
    assert (a.k, a.min_k, a.max_k, a.bound, a.out_name, a.threads, a.extract, a.keep, a.remove) == (3, None, None, 1e-4, None, 1, None, None, None)
    a = cli.parse_qse_args(base[1:] + ["--min_k", "2", "--max_k", "4", "--bound", "0.001", "--out_name", "o", "--extract", "f", "--keep", "g"])
    assert (a.min_k, a.max_k, a.bound, a.out_name, a.extract, a.keep) == (2, 4, 0.001, "o", "f", "g")

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    for ks in (["--k", "17"], ["--min_k", "15", "--max_k", "17"]):
        with pytest.raises(SystemExit, match=r"qse needs every K <= 16.*running sums of a sample.*K = 17 was asked for"):
            cli.main(base + ks)
    for value in ("0.5", "-0.1", "nan"):
        with pytest.raises(SystemExit, match=r"--bound must be in \[0, 0.5\)"):
            cli.main(base + ["--k", "3", "--bound", value])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen"), "--k", "3"])
    with pytest.raises(SystemExit, match=r"qse needs the .*run\.3\.P not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.Q", np.full((6, 3), 1 / 3))
    (tmp_path / "x.fam").write_text("\n".join(f"f s{i}" for i in range(5)) + "\n")
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j + 1}\tA\tG\n" for j in range(9)))
    bed.write_bytes(bytes(3 + 2 * 9))                        # N = 5, M = 9; the .Q has 6 rows
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 6 x 3 matrix"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + ["--k", "3"])
    assert not list(tmp_path.glob("*.Q_info_se"))


def test_infer_q_se_without_refine_is_refused_before_anything_is_loaded(tmp_path, monkeypatch):
    from neural_admixture_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)        # (the refusal comes first either way)
    base = ["infer", "--name", "nothing", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "x.bed"), "--out_name", "o", "--q_se"]
    assert cli.parse_infer_args(base[1:]).q_se is True and cli.parse_infer_args(base[1:-1]).q_se is False
    with pytest.raises(SystemExit, match=r"--q_se needs --refine N: the encoder's Q is not a maximum"):
        cli.main(base)
    with pytest.raises(SystemExit, match=r"--bound must be in \[0, 0.5\)"):
        cli.main(base + ["--refine", "5", "--bound", "0.7"])
    with pytest.raises(FileNotFoundError, match="nothing_config.json"):  # with --refine the run goes on to the files, which are not there
        cli.main(base + ["--refine", "5"])


def test_train_q_se_refuses_sharded_and_supervised_runs(tmp_path, monkeypatch):
    """`train --q_se`: the refusals and the wording of --p_se, before the GPU check; the keyword of train() likewise."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["train", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "x.bed"), "--k", "3", "--q_se"]
    assert cli.parse_train_args(base[1:]).q_se is True and cli.parse_train_args(base[1:-1]).q_se is False
    with pytest.raises(SystemExit, match=r"--q_se is single-GPU: run it with --num_gpus 1"):
        cli.main(base + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--q_se ignores labels: it is not available with --pops_path"):
        cli.main(base + ["--pops_path", str(tmp_path / "pops")])
    with pytest.raises(SystemExit, match=r"--q_se needs every K <= 16"):
        cli.main(base[:-3] + ["--min_k", "15", "--max_k", "17", "--q_se"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(base)
    G0, V0 = torch.zeros((4, 100), dtype=torch.uint8), np.zeros((8, 100), np.float32)
    with pytest.raises(ValueError, match="q_se needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 2, 16, True, V0, None, q_se=True)
    with pytest.raises(ValueError, match="q_se needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, torch.device("cpu"), 1, 16, True, V0, ["a", "b", "c", "a"], q_se=True)
    with pytest.raises(ValueError, match="q_se needs every K <= 16"):
        na.train(1, 8, 1e-3, 17, 0, G0, torch.device("cpu"), 1, 16, True, V0, None, q_se=True)
    from neural_admixture_amd.train import AFTER_TRAINING
    order = [o.kw for o in AFTER_TRAINING]
    assert order.index("p_se") < order.index("q_se") < order.index("fit_check")


def test_sharded_and_cpu_engines_refuse_q_se():
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.q_se is single-GPU"):
        e.q_se()
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.q_se needs the HIP engine with its packed matrix resident"):
        e.q_se()


def test_public_names():
    import neural_admixture_amd as na
    for name in ("q_se", "q_info"):
        assert callable(getattr(na, name)) and name in na.__all__
    from neural_admixture_amd import qse
    assert qse.QseResult._fields == ("se", "n", "at_bound", "cov") and callable(qse.se_from_info)


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_info(xp, M, P, Q, rows, kind, **kw):
    """One qse.q_info call -> numpy (info, n); Q [resident, K] are the resident rows' fractions."""
    from neural_admixture_amd import qse
    if kind == "none":
        out = qse.q_info(xp[:len(rows)], M, P, Q[:len(rows)], None, **kw)
    else:
        out = qse.q_info(xp, M, P, Q[rows], torch.from_numpy(rows).to(xp.device), **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_info(got, want, tol, what):
    """n equal; an entry that is 0 in float64 exactly +0.0, else |A - A64| <= tol A64; prints the largest ratio before it asserts."""
    I, n = got
    I64, n64 = want
    r = _ratio(I, I64)
    print(f"{what}: max |A - A64| / A64 = {r:.3e} (bound {tol:.3e})")
    assert I.dtype == np.float64 and n.dtype == np.int32 and I.shape == I64.shape
    assert np.array_equal(n, n64)
    zero = I64 == 0
    assert (I[zero] == 0).all() and not np.signbit(I[zero]).any()
    assert (np.abs(I - I64) <= tol * I64).all()
    return r


def _run_case(b, M, K, kind, tol, resident=ROWS, **kw):
    from neural_admixture_amd._lib import lib
    Gm, P, Q = _case(M, K, resident)
    rows = case_rows(b, kind, resident=resident) if resident > 5 else np.arange(b, dtype=np.int32)
    I64, n64 = _truth(M, K, resident)
    got = _gpu_info(_pack(Gm).to(_dev()), M, P, Q, rows, kind, **kw)
    _check_info(got, (I64[rows], n64[rows]), tol, f"b={b} M={M} K={K} rows={kind} ranges={int(lib.nadm_sample_info_ranges(b, M))}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["list", "none"])
@pytest.mark.parametrize("b, M, K", CASES)
def test_sums_against_float64(b, M, K, kind):
    """10 % missing calls, ld = ceil(M/4) rounded to 16 plus 16, every pad bit set; the list has a duplicate and is out of order."""
    got = _run_case(b, M, K, kind, TOL)
    rows = _rows(b, kind)
    if 4 in rows.tolist():                                       # the sample without an observed call: exactly nothing
        s = rows.tolist().index(4)
        assert got[1][s] == 0 and (got[0][s] == 0).all()


@pytest.mark.gpu
def test_several_ranges_per_tile_and_several_tiles_with_a_ragged_last_one():
    from neural_admixture_amd._lib import lib
    M = next(m for m in (200, 257, 600, 1030, 5000) if int(lib.nadm_sample_info_ranges(64, m)) > 1)
    assert int(lib.nadm_sample_info_ranges(64, M)) > 1
    _run_case(64, M, 3, "list", TOL)
    b = 600                                                      # three tiles of 256, the last with 88 rows
    assert b % 256 != 0 and int(lib.nadm_sample_info_ranges(b, 1030)) > 1
    _run_case(b, 1030, 7, "list", TOL)
    _run_case(257, 1030, 7, "list", TOL)                         # one row in the second tile: three of its waves have nothing to do


@pytest.mark.gpu
def test_more_than_one_chunk_per_range():
    """M large enough that a range holds several chunks (found by the query): the loop's steady state, its prefetch and its barriers."""
    assert _cpr(LONG_B, LONG_M) >= 2
    _run_case(LONG_B, LONG_M, LONG_K, "none", TOL_LONG, resident=LONG_B)


@pytest.mark.gpu
def test_two_launches_give_the_same_bits_and_row_blocks_do_not_matter():
    Gm, P, Q = _case(1030, 7)
    xp = _pack(Gm).to(_dev())
    rows = _rows(600, "list")
    a = _gpu_info(xp, 1030, P, Q, rows, "list")
    b = _gpu_info(xp, 1030, P, Q, rows, "list")
    c = _gpu_info(xp, 1030, P, Q, rows, "list", row_block=256)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(a, c):
        assert x.tobytes() == y.tobytes()
    d = _gpu_info(xp, 1030, P, Q, np.arange(ROWS, dtype=np.int32), "none", row_block=256)
    e = _gpu_info(xp, 1030, P, Q, np.arange(ROWS, dtype=np.int32), "none")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d, e))


@pytest.mark.gpu
def test_masked_terms_are_exactly_zero():
    """P changed at the SNPs where a sample's call is missing, and the pad bits of the row's last byte and the bytes behind it, leave
    that sample's info bit-identical; a sample with every call missing has n = 0, zero info and NaN standard errors."""
    from neural_admixture_amd import qse
    dev = _dev()
    M, K = 1030, 7
    Gm, P, Q = _case(M, K)
    rows = np.arange(ROWS, dtype=np.int32)
    base = _gpu_info(_pack(Gm, dirty=False).to(dev), M, P, Q, rows, "none")
    dirty = _gpu_info(_pack(Gm, dirty=True).to(dev), M, P, Q, rows, "none")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(base, dirty))
    for s in (0, 5, 77):
        P2 = P.copy()
        gone = Gm[s] == 3
        P2[gone] = np.random.default_rng(s).uniform(0.0, 1.0, size=(int(gone.sum()), K)).astype(np.float32)
        got = _gpu_info(_pack(Gm).to(dev), M, P2, Q, rows, "none")
        assert got[0][s].tobytes() == base[0][s].tobytes() and got[1][s] == base[1][s]
        assert got[0][0 if s else 1].tobytes() != base[0][0 if s else 1].tobytes()           # (the others do see the change)
    assert base[1][4] == 0 and (base[0][4] == 0).all() and not np.signbit(base[0][4]).any() and base[1][5] == int((Gm[5, :40] != 3).sum()) > 20
    res = qse.q_se(_pack(Gm).to(dev), M, P, Q)
    se = res.se.cpu().numpy()
    assert np.isnan(se[4]).all() and np.isfinite(np.delete(se, 4, axis=0)).all() and res.at_bound.cpu().numpy()[2].all()
    assert int(res.n[4]) == 0 and res.se.dtype == torch.float64 and tuple(res.se.shape) == (ROWS, K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3, 8, 16])
def test_the_device_inversion_equals_the_cpu_route_on_the_kernels_own_info(K):
    from neural_admixture_amd import qse
    dev = _dev()
    M = 1500
    Gm, P, Q = _case(M, K)
    info, n = qse.q_info(_pack(Gm).to(dev), M, P, Q)
    got = qse.se_from_info(info, Q, n)
    want = qse.se_from_info(info.cpu(), Q, n.cpu())
    g, w = got.se.cpu().numpy(), want.se.numpy()
    assert got.se.device.type == "cuda" and np.array_equal(np.isnan(g), np.isnan(w)) and np.isnan(g[4]).all() and np.isfinite(g[0]).all()
    assert torch.equal(got.at_bound.cpu(), want.at_bound) and torch.equal(got.n.cpu(), want.n)
    A = QO.full(info.cpu().numpy(), K)
    worst = 0.0
    for s in range(ROWS):
        if np.isnan(w[s]).any():
            continue
        cond = 0.0
        for c in (K - 1, 0):
            keep = [a for a in range(K) if a != c]
            J = (A[s][np.ix_(keep, keep)] - A[s][c, keep][None, :]) - (A[s][keep, c][:, None] - A[s][c, c])
            cond = max(cond, np.linalg.cond(J))
        tol = 8 * K * cond * 2.0 ** -52
        rel = float(np.max(np.abs(g[s] - w[s]) / w[s]))
        worst = max(worst, rel / tol)
        assert rel <= tol, (s, rel, tol)
    print(f"K={K}: device against CPU inversion, largest relative difference / allowed = {worst:.3e}")


@pytest.mark.gpu
def test_planted_panel_on_the_gpu():
    from neural_admixture_amd import qse
    Gm, P, Q, I64, n64, se64 = _planted()
    res = qse.q_se(_pack(Gm).to(_dev()), P.shape[0], P, Q)
    se = res.se.cpu().numpy()
    assert np.array_equal(res.n.cpu().numpy(), n64) and np.isfinite(se64).all() and np.isfinite(se).all()
    rel = float(np.max(np.abs(se - se64) / se64))
    print(f"planted panel: max |SE - SE64| / SE64 = {rel:.3e} (bound {TOL_SE:.3e})")
    assert rel <= TOL_SE
    assert res.at_bound.cpu().numpy().any() and (se[res.at_bound.cpu().numpy()] > 0).all()


@pytest.mark.gpu
def test_engine_q_se_equals_the_library_free_form_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from neural_admixture_amd import qse
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
    before = [t.clone() for t in (e.pflat, e.mflat, e.vflat)]
    for head in (0, 1):
        Qh = torch.cat([e.infer_q(idx[s:s + bmax], min(bmax, N - s))[head] for s in range(0, N, bmax)], dim=0)
        got = e.q_se(head=head, bound=1e-3)
        want = qse.q_se(e.xp, M, e.P(head).clone(), Qh, bound=1e-3)
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a.nan_to_num(7.0) if a.dtype.is_floating_point else a, b.nan_to_num(7.0) if b.dtype.is_floating_point else b)
        assert tuple(got.se.shape) == (N, ks[head]) and bool(torch.isfinite(got.se).all())
    with pytest.raises(RuntimeError, match="head must be in 0..1"):
        e.q_se(head=2)
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


MASKED = 7                                                        # the demo sample that loses 90 % of its calls before `infer`


def _set_missing(bed_bytes, N, sample, snps):
    """PLINK .bed bytes (SNP-major, 4 samples per byte, after the 3 magic bytes) with `sample`'s calls at `snps` set to missing (0b01)."""
    a = np.array(bed_bytes, dtype=np.uint8, copy=True)
    body = a[3:].reshape(-1, (N + 3) // 4)
    sh = 2 * (sample % 4)
    col = body[snps, sample // 4]
    body[snps, sample // 4] = (col & ~np.uint8(3 << sh)) | np.uint8(1 << sh)
    return a


@pytest.fixture(scope="module")
def demo_run(tmp_path_factory):
    """The bundled demo trained once for a few epochs with --polish 2 --q_se: (directory of the data, directory of the run, N, M, log)."""
    from neural_admixture_amd import cli
    tmp = tmp_path_factory.mktemp("qse_demo")
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = np.load(f"{golden}/demo_k3.npz")
    N, M = int(d["N"]), int(d["M"])
    d["bed_bytes"].tofile(tmp / "demo.bed")
    (tmp / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    snps = np.sort(np.random.default_rng(0).choice(M, size=int(0.9 * M), replace=False))
    _set_missing(d["bed_bytes"], N, MASKED, snps).tofile(tmp / "query.bed")
    (tmp / "query.fam").write_text("\n".join(["s"] * N) + "\n")
    out = tmp / "out"
    records = []
    handler = logging.Handler()
    handler.emit = lambda r: records.append(r.getMessage())
    root, level = logging.getLogger(), logging.getLogger().level
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    try:
        assert cli.main(["train", "--epochs", "5", "--k", "3", "--name", "demo", "--data_path", str(tmp / "demo.bed"), "--save_dir", str(out),
                         "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--polish", "2", "--q_se"]) == 0
    finally:
        root.removeHandler(handler)
        root.setLevel(level)
    return tmp, out, N, M, records


@pytest.mark.gpu
def test_train_q_se_end_to_end_on_the_demo(demo_run):
    tmp, out, N, M, msgs = demo_run
    Q = np.loadtxt(out / "demo.3.Q", ndmin=2)
    a = np.loadtxt(out / "demo.3.Q_info_se", ndmin=2)
    assert a.shape == Q.shape == (N, 3) and np.isfinite(a).all() and (a > 0).all()
    assert len([m for m in msgs if m.startswith("Q standard errors given P (K=3): median SE ")]) == 1
    assert not (out / "demo.3.Q_se").exists()


@pytest.mark.gpu
def test_cli_qse_end_to_end(demo_run, caplog):
    """The `qse` mode on the files `train --q_se` wrote: {out_name}.3.Q_info_se of the .Q's shape, equal entry for entry to train's
    (the mode reads the .P / .Q that train wrote: 18 digits, the same float32), and the log lines appear; --keep is honoured."""
    from neural_admixture_amd import cli
    tmp, out, N, M, _ = demo_run
    caplog.set_level(logging.INFO)
    argv = ["--k", "3", "--name", "demo", "--data_path", str(tmp / "demo.bed"), "--save_dir", str(out)]
    assert cli.main(["qse"] + argv + ["--out_name", "again"]) == 0
    a, b = (np.loadtxt(out / f"{name}.3.Q_info_se", ndmin=2) for name in ("demo", "again"))
    assert b.shape == (N, 3) and np.array_equal(a, b, equal_nan=True)
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("Q standard errors given P (K=3): median SE ") and f"of {N * 3} entries" in m for m in msgs)
    assert any("Standard errors of Q saved." in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    (tmp / "demo.fam").write_text("".join(f"f s{i}\n" for i in range(N)))
    (tmp / "some").write_text("".join(f"f s{i}\n" for i in range(3, N, 5)))
    np.savetxt(out / "sub.3.Q", np.loadtxt(out / "demo.3.Q", ndmin=2)[3::5], delimiter=" ")
    np.savetxt(out / "sub.3.P", np.loadtxt(out / "demo.3.P", ndmin=2), delimiter=" ")
    try:
        assert cli.main(["qse", "--k", "3", "--name", "sub", "--data_path", str(tmp / "demo.bed"), "--save_dir", str(out),
                         "--keep", str(tmp / "some")]) == 0
    finally:
        (tmp / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    # (a smaller batch may be cut into other ranges: the same sums in another order)
    assert np.allclose(np.loadtxt(out / "sub.3.Q_info_se", ndmin=2), a[3::5], rtol=1e-5, atol=0)


@pytest.mark.gpu
def test_infer_refine_q_se_end_to_end_on_the_demo(demo_run, caplog):
    """`infer --refine 20 --q_se` on a copy of the demo in which one sample lost 90 % of its calls: the file is written next to the .Q,
    of its shape, and that sample has the largest standard error of all."""
    from neural_admixture_amd import cli
    tmp, out, N, M, _ = demo_run
    caplog.set_level(logging.INFO)
    base = ["infer", "--name", "demo", "--save_dir", str(out), "--data_path", str(tmp / "query.bed")]
    assert cli.main(base + ["--out_name", "refined", "--refine", "20", "--q_se", "--batch_size", "300"]) == 0
    Qr = np.loadtxt(out / "refined.3.Q", ndmin=2)
    se = np.loadtxt(out / "refined.3.Q_info_se", ndmin=2)
    assert se.shape == Qr.shape == (N, 3) and np.isfinite(se).all() and (se > 0).all()
    worst = se.max(axis=1)
    print(f"largest SE of the masked sample {worst[MASKED]:.4f}, of the others at most {np.delete(worst, MASKED).max():.4f}")
    assert int(np.argmax(worst)) == MASKED
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("Q standard errors given P (K=3): median SE ") for m in msgs)
    assert cli.main(base + ["--out_name", "plain", "--refine", "20"]) == 0                     # without the flag: the same .Q, no SE file
    assert (out / "plain.3.Q").read_bytes() == (out / "refined.3.Q").read_bytes() and not (out / "plain.3.Q_info_se").exists()


# ------------------------------------------------------------------------------------------------ the yardsticks, by hand
def _measure_yardsticks():
    """Largest deviation of the float32 restatement from float64 on the largest case and the long one, and the SE yardstick (CPU only)."""
    def dev_of(b, M, K, resident):
        Gm, P, Q = _case(M, K, resident)
        return _ratio(QO.info32(Gm[:b], P, Q[:b], _cpr(b, M)), _truth(M, K, resident)[0][:b])
    print(f"YARD      = {dev_of(200, 4099, 8, ROWS):.3e}")
    print(f"YARD_LONG = {dev_of(LONG_B, LONG_M, LONG_K, LONG_B):.3e}")
    Gm, P, Q, I64, n64, se64 = _planted()
    se32 = QO.se(QO.info32(Gm, P, Q, _cpr(len(Gm), P.shape[0])), 3, n64)
    print(f"YARD_SE   = {float(np.max(np.abs(se32 - se64) / se64)):.3e}")
    for seed in (0, 1, 2):
        print("calibration seed", seed, ["%.4f" % v for v in QO.calibration(seed)])


if __name__ == "__main__":
    _measure_yardsticks()
