"""Admixture-aware kinship (nadm_kinship, relate.kinship_block / kinship / kinship_pairs, Engine.kinship, the `kinship` mode of the
command line).  The float64 numpy restatement and the shared data live in tests/kinship_oracle.py.

The two tolerances of a block against float64 are derived, not measured: |num - num64| <= 2^-15 abs_ab and |den - den64| <= 2^-15
den64 (abs_ab = sum_j |d_aj||d_bj|; den's terms are all >= 0, so den64 is its own sum of magnitudes).  Two round-to-nearest bf16
pieces carry a value to 2^-17 relative; the three kept products hi.hi + hi.lo + lo.hi therefore miss at most 3 * 2^-17 ~ 2.3e-5 of
|d_a||d_b| per term, the rest of 2^-15 ~ 3.05e-5 is room for the fp32 accumulation inside a range.  n is exact.
OBSERVED on an MI355X over BLOCKS and the other block tests: see DESIGN.md section 4.9 (each case prints its two ratios)."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kinship_oracle as KO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2.0 ** -15
ROWS = 140                   # resident rows of the GPU cases
# (ba, bb, M, K, pimin): every ba x bb, M, K and pimin of the issue at least once, not their product
BLOCKS = [(1, 1, 257, 2, 0.0), (16, 16, 1027, 3, 0.0), (15, 17, 3001, 8, 0.05), (70, 130, 257, 9, 0.0), (130, 70, 1027, 16, 0.05),
          (70, 130, 3001, 20, 0.0), (16, 16, 257, 8, 0.05), (15, 17, 1027, 20, 0.05), (130, 70, 3001, 2, 0.0)]


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_on_a_case_worked_out_by_hand():
    """Two samples, three SNPs, K = 2.  Q_a = (1, 0), Q_b = (1/2, 1/2); P = (1/2, 1/2), (1/4, 3/4), (1/2, 0).
        pi_a = 1/2, 1/4, 1/2         pi_b = 1/2, 1/2, 1/4
        g_a  = 2, 1, missing         g_b  = 2, 0, 1
        d_a  = 1, 1/2, 0             d_b  = 1, -1, 1/2
        s_a  = 1/2, sqrt(3)/4, 0     s_b  = 1/2, 1/2, sqrt(3)/4
    num_ab = 1 - 1/2 = 1/2, den_ab = 1/4 + sqrt(3)/8, n_ab = 2, abs_ab = 3/2; num_aa = 5/4, den_aa = 1/4 + 3/16 = 7/16, n_aa = 2;
    num_bb = 1 + 1 + 1/4 = 9/4, den_bb = 1/4 + 1/4 + 3/16 = 11/16, n_bb = 3.  phi_ab = (1/2) / (1 + sqrt(3)/2) = 0.26795,
    phi_aa = 5/7, phi_bb = 9/11.  With pimin = 0.3 the two pi = 1/4 drop out: num_ab = 1, den_ab = 1/4, n_ab = 1, phi_ab = 1;
    n_aa = 1, n_bb = 2."""
    Gm = np.asarray([[2, 1, 3], [2, 0, 1]], dtype=np.uint8)
    Q = np.asarray([[1.0, 0.0], [0.5, 0.5]], dtype=np.float32)
    P = np.asarray([[0.5, 0.5], [0.25, 0.75], [0.5, 0.0]], dtype=np.float32)
    phi, num, den, n, ab = KO.kinship(Gm, P, Q)
    r3 = np.sqrt(3.0)
    assert np.allclose(num, [[1.25, 0.5], [0.5, 2.25]], rtol=0, atol=1e-15)
    assert np.allclose(den, [[7 / 16, 0.25 + r3 / 8], [0.25 + r3 / 8, 11 / 16]], rtol=0, atol=1e-15)
    assert np.array_equal(n, [[2, 2], [2, 3]]) and ab[0, 1] == 1.5
    assert np.allclose(phi, [[5 / 7, 0.5 / (1 + r3 / 2)], [0.5 / (1 + r3 / 2), 9 / 11]], rtol=0, atol=1e-15)
    phi, num, den, n, ab = KO.kinship(Gm, P, Q, pimin=0.3)
    assert num[0, 1] == 1.0 and den[0, 1] == 0.25 and phi[0, 1] == 1.0 and np.array_equal(n, [[1, 1], [1, 2]])
    none = KO.kinship(np.full((2, 3), 3, dtype=np.uint8), P, Q)
    assert np.isnan(none[0]).all() and not none[1].any() and not none[3].any()


@functools.lru_cache(maxsize=None)
def _pedigree():
    Gm, P, Q = KO.make_pedigree(0)
    return Gm, P, Q, KO.kinship(Gm, P, Q)


def test_oracle_on_the_pedigree():
    """The estimator itself, in float64, with the true Q and P: first-degree pairs 0.25 +- 0.06, the duplicate 0.5 +- 0.06, founder
    pairs |phi| < 0.0625, founders' phi_aa 0.5 +- 0.07."""
    Gm, P, Q, (phi, num, den, n, ab) = _pedigree()
    F = KO.PED_FOUNDERS
    assert Gm.shape == (15, 3001) and 0.04 < (Gm == 3).mean() < 0.06
    for i, j in KO.PED_PARENT_CHILD + KO.PED_SIBS:
        assert abs(phi[i, j] - 0.25) <= 0.06, (i, j, phi[i, j])
    for i, j in KO.PED_DUPLICATE:
        assert abs(phi[i, j] - 0.5) <= 0.06, (i, j, phi[i, j])
    for i in range(F):
        assert abs(phi[i, i] - 0.5) <= 0.07, (i, phi[i, i])
        for j in range(i + 1, F):
            assert abs(phi[i, j]) < 0.0625, (i, j, phi[i, j])
    assert np.array_equal(phi, phi.T) and np.array_equal(n, ((Gm != 3).astype(np.int64) @ (Gm != 3).astype(np.int64).T))


def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_kinship", "nadm_kinship_ranges", "nadm_kinship_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "#define NADM_KINSHIP_MAX_ROWS 4096" in header


def test_ranges_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    rg, f = lib.nadm_kinship_ranges, lib.nadm_kinship_scratch_floats
    Ms = (1, 255, 256, 257, 513, 1027, 3001, 70000, 500000, 600000, 5000000)
    bs = (1, 15, 16, 17, 63, 64, 65, 70, 128, 130, 1024, 4096)
    assert int(rg(16, 16, 256)) == 1 and int(rg(16, 16, 257)) == 2            # one tile: a range per chunk while that fills the chip
    assert int(rg(1024, 1024, 500000)) >= 2 and int(rg(4096, 4096, 500000)) >= 2 and int(rg(16, 16, 5000000)) >= 2
    for M in Ms:
        chunks = (M + 255) // 256
        for ba in bs:
            for bb in bs:
                r = int(rg(ba, bb, M))
                tiles = ((ba + 63) // 64) * ((bb + 63) // 64)
                assert 1 <= r <= chunks and -(-chunks // r) <= 1024            # at most 2^18 SNPs in one fp32 accumulator
                assert int(f(ba, bb, M)) >= r * tiles * 3 * 64 * 64
    for ba in bs:
        for bb in bs:
            v = [int(f(ba, bb, M)) for M in Ms]
            assert v[0] > 0 and all(y >= x for x, y in zip(v, v[1:]))
    for M in Ms:
        for bb in (1, 70, 1024):
            v = [int(f(b, bb, M)) for b in range(1, 1400, 3)] + [int(f(4096, bb, M))]
            assert all(y >= x for x, y in zip(v, v[1:]))
            w = [int(f(bb, b, M)) for b in range(1, 1400, 3)] + [int(f(bb, 4096, M))]
            assert all(y >= x for x, y in zip(w, w[1:]))
    for M in range(1, 9000, 7):                                                # the wobble of ceil(512 / tiles) * tiles is not in the size
        assert int(f(130, 70, M + 7)) >= int(f(130, 70, M)) and int(f(16, 16, M + 7)) >= int(f(16, 16, M))
    for bad in ((0, 4, 100), (4, 0, 100), (4, 4, 0), (4097, 4, 100), (4, 4097, 100), (-1, 4, 100)):
        assert int(f(*bad)) == 0 and int(rg(*bad)) == 0


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 4), 0.25)
    P = torch.full((50, 4), 0.25)
    num, den = torch.empty((4, 4), dtype=torch.float64), torch.empty((4, 4), dtype=torch.float64)
    nobs = torch.empty((4, 4), dtype=torch.int32)
    scratch = torch.empty(3 * 4096)
    keep = (xp, P, Q, num, den, nobs, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idxA=None, ba=4, idxB=None, bb=4, M=50, P=P.data_ptr(), k=3, kp=4, QA=Q.data_ptr(), QB=Q.data_ptr(),
             q_stride=4, pimin=0.0, num=num.data_ptr(), den=den.data_ptr(), nobs=nobs.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(P=None), "null pointer"), (dict(QA=None), "null pointer"), (dict(QB=None), "null pointer"),
    (dict(num=None), "null pointer"), (dict(den=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(ba=0), "empty block"), (dict(bb=-3), "empty block"), (dict(M=0), "empty block"),
    (dict(ba=4097), "must be <= NADM_KINSHIP_MAX_ROWS"), (dict(bb=100000), "must be <= NADM_KINSHIP_MAX_ROWS"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(pimin=-1e-3), "pimin must be in [0, 0.5)"), (dict(pimin=0.5), "pimin must be in [0, 0.5)"), (dict(pimin=float("nan")), "pimin must be in [0, 0.5)"),
    (dict(unaligned="QA"), "must be 16-byte aligned"), (dict(unaligned="P"), "must be 16-byte aligned"), (dict(unaligned="num"), "8-byte"),
])
def test_kinship_refuses_before_any_launch(change, message):
    """Every refusal of nadm_kinship is decided on the host: it is reported with its message on a machine without a GPU (where a launch
    would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    else:
        a.update(change)
    status = lib.nadm_kinship(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_kinship"):
        check(status, "kinship")
    del keep


def test_cli_kinship_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing or misshapen .P / .Q files end the run with the file named, before the genotypes are read: the .bed
    named here does not exist, and the reader is a stand-in that fails the test when called."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "absent.bed"
    base = ["kinship", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_kinship_args(base[1:])
    assert a.min_phi == 2.0 ** -4.5 and a.pimin == 0.0 and a.out_name is None and a.threads == 1
    a = cli.parse_kinship_args(base[1:] + ["--out_name", "o", "--min_phi", "0.1", "--pimin", "0.01", "--threads", "4"])
    assert (a.out_name, a.min_phi, a.pimin, a.threads) == ("o", 0.1, 0.01, 4)

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(SystemExit):
        cli.main(["kinship", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)])          # no --k
    with pytest.raises(SystemExit, match=r"--pimin must be in \[0, 0.5\)"):
        cli.main(base + ["--pimin", "0.5"])
    with pytest.raises(SystemExit, match=r"--k must be in 1..64"):
        cli.main(base[:2] + ["65"] + base[3:])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "absent.pgen")])
    with pytest.raises(SystemExit, match=r"run\.3\.P not found"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q not found"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((6, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"absent\.fam not found"):
        cli.main(base)
    (tmp_path / "absent.fam").write_text("\n".join(["s"] * 5) + "\n")
    with pytest.raises(SystemExit, match=r"absent\.bed not found"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10 + 1))                   # 5 samples = 2 bytes per SNP: 10 SNPs and a byte too many
    with pytest.raises(SystemExit, match=r"absent\.bed does not hold whole SNPs of the 5 samples"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10))                       # N = 5, M = 10 from the sizes alone
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 6 x 3 matrix, the data needs 5 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 2), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 5 x 2 matrix, the data needs 5 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))   # a misshapen .P: a row short, then a column short
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 9 x 3 matrix, the model needs 10 x 3"):
        cli.main(base)
    np.savetxt(tmp_path / "run.3.P", np.full((10, 2), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 2 matrix, the model needs 10 x 3"):
        cli.main(base)
    # a VCF tells N and M only once it is parsed: the widths are still checked before it is read
    vcf = ["kinship", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "absent.vcf")]
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 10 x 2 matrix"):
        cli.main(vcf)
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 4), 0.25))
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 5 x 4 matrix"):
        cli.main(vcf)
    # train and infer keep their dispatch
    with pytest.raises(AssertionError, match='Please provide either the argument "train" or "infer"'):
        cli.main(["relate"])


def test_sharded_engines_refuse_kinship():
    """Engine.kinship is single-GPU; the check comes first, so a stand-in without any device state shows it."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan = "dp", 2, None
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.kinship()
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.kinship(0, 0.1)


def test_band_counts():
    from neural_admixture_amd import relate
    got = relate.band_counts([0.5, 0.36, 0.25, 0.2, 0.1, 0.05, 0.045])
    assert [c for _, _, c in got] == [2, 2, 1, 2] and [round(e, 4) for _, e, _ in got] == [0.3536, 0.1768, 0.0884, 0.0442]


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS resident rows with the planted cases of kinship_oracle.make_edge_case; the tests leave them as they are."""
    Gm, P, Q, dead = KO.make_edge_case(ROWS, M, K)
    return Gm, P, Q, dead, _packed(Gm)


@functools.lru_cache(maxsize=None)
def _terms(M, K, pimin):
    Gm, P, Q, _, _ = _case(M, K)
    return KO.terms(Gm, P, Q, pimin)


def _rows(b, salt=0):
    """Rows of one side of a block: a permutation of the resident rows with the one-hot row 2, the all-missing row 4 and the 7-call
    row 5 in it, cut to b, the last entry a duplicate of the first; b = 1 is row 7."""
    if b == 1:
        return np.asarray([7], dtype=np.int32)
    perm = np.random.default_rng(100 * b + salt).permutation(ROWS)
    perm = np.concatenate([[2, 4, 5], perm[(perm != 2) & (perm != 4) & (perm != 5)]])[:b - 1]
    perm = perm[np.random.default_rng(100 * b + salt + 1).permutation(b - 1)]
    perm = np.concatenate([perm, perm[:1]])
    return perm.astype(np.int32)


def _gpu_block(xp, M, P, Q, idxA, idxB, pimin=0.0, same_list=False):
    """One nadm_kinship call -> (num, den float64, n int32) numpy [ba, bb]; Q [ROWS, K] are the resident rows' fractions."""
    from neural_admixture_amd import project, relate
    dev = xp.device
    K = Q.shape[1]
    Pp = project.pad_P(P, dev)
    kp = Pp.shape[1]
    ia = None if idxA is None else torch.from_numpy(idxA).to(dev)
    QA = project.pad_Q(Q[idxA] if idxA is not None else Q, len(idxA) if idxA is not None else len(Q), K, kp, dev)
    if same_list:
        ib, QB = ia, QA
    else:
        ib = None if idxB is None else torch.from_numpy(idxB).to(dev)
        QB = project.pad_Q(Q[idxB] if idxB is not None else Q, len(idxB) if idxB is not None else len(Q), K, kp, dev)
    num, den, n = relate.kinship_block(xp, M, Pp, K, ia, QA, ib, QB, pimin)
    torch.cuda.synchronize()
    return num.cpu().numpy(), den.cpu().numpy(), n.cpu().numpy()


def _check_block(got, want, what):
    """n exact, |num - num64| <= 2^-15 abs_ab, |den - den64| <= 2^-15 den64; prints the two largest ratios before it asserts."""
    num, den, n = got
    num64, den64, n64, ab = want
    en, ed = np.abs(num - num64), np.abs(den - den64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = float(np.nanmax(np.where(ab > 0, en / ab, 0.0)))
        rd = float(np.nanmax(np.where(den64 > 0, ed / den64, 0.0)))
    print(f"{what}: max |num - num64| / abs_ab = {rn:.3e} (2^{np.log2(max(rn, 1e-300)):.1f}), max |den - den64| / den64 = {rd:.3e} "
          f"(2^{np.log2(max(rd, 1e-300)):.1f}); bound 2^-15 = {TOL:.3e}")
    assert np.array_equal(n, n64)
    assert (en <= TOL * ab).all()
    assert (ed <= TOL * den64).all()
    return rn, rd


@pytest.mark.gpu
@pytest.mark.parametrize("ba, bb, M, K, pimin", BLOCKS)
def test_block_against_float64(ba, bb, M, K, pimin):
    """n exact, num and den within the derived bounds (module docstring); every case prints its two ratios before it asserts.
    OBSERVED on an MI355X over BLOCKS: max |num - num64| / abs_ab 2.0e-6 .. 1.0e-5 (the largest at 70 x 130, M = 257, K = 9),
    max |den - den64| / den64 1.7e-6 .. 4.1e-6; bound 3.05e-5; 2, 5 and 12 ranges."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    Gm, P, Q, dead, xph = _case(M, K)
    idxA, idxB = _rows(ba), _rows(bb, salt=7)
    if ba > 2:
        assert Q[idxA].max(axis=1).max() == 1.0 and (Gm[idxA] == 3).all(axis=1).any() and ((Gm[idxA] != 3).sum(axis=1) == 7).any()
        assert idxA[-1] == idxA[0] and (P[0] == 0).all() and (P[1] == 1).all()
    t = _terms(M, K, pimin)
    want = KO.from_terms(KO.gather(t, idxA), KO.gather(t, idxB))
    got = _gpu_block(xph.to(dev), M, P, Q, idxA, idxB, pimin)
    _check_block(got, want, f"ba={ba} bb={bb} M={M} K={K} pimin={pimin} ranges={int(lib.nadm_kinship_ranges(ba, bb, M))}")
    if ba > 2:                                               # the all-missing sample: its row and column are num = den = 0, n = 0
        for a in np.nonzero(idxA == 4)[0]:
            assert not got[0][a].any() and not got[1][a].any() and not got[2][a].any()
        for b in np.nonzero(idxB == 4)[0]:
            assert not got[0][:, b].any() and not got[1][:, b].any() and not got[2][:, b].any()
        if pimin > 0:                                        # the mask did drop calls
            assert (want[2] < (Gm[idxA] != 3).astype(np.int64) @ (Gm[idxB] != 3).astype(np.int64).T).any()


@pytest.mark.gpu
def test_same_list_on_both_sides_and_rows_without_a_gather_list():
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead, xph = _case(M, K)
    xp = xph.to(dev)
    idx = _rows(70)
    t = KO.gather(_terms(M, K, 0.0), idx)
    got = _gpu_block(xp, M, P, Q, idx, None, same_list=True)
    _check_block(got, KO.from_terms(t, t), "idxA is idxB (70 rows)")
    two = _gpu_block(xp, M, P, Q, idx, idx.copy())
    assert all(np.array_equal(a, b) for a, b in zip(got, two))
    t = _terms(M, K, 0.0)
    _check_block(_gpu_block(xp, M, P, Q, None, None), KO.from_terms(t, t), f"rows 0..{ROWS} without a gather list")


@pytest.mark.gpu
def test_more_than_one_range():
    from neural_admixture_amd._lib import lib
    dev = _dev()
    M = next(m for m in range(1, 100000) if int(lib.nadm_kinship_ranges(16, 16, m)) >= 2)
    K = 3
    Gm, P, Q, dead, xph = _case(M, K)
    idxA, idxB = _rows(16), _rows(16, salt=7)
    t = _terms(M, K, 0.0)
    got = _gpu_block(xph.to(dev), M, P, Q, idxA, idxB)
    _check_block(got, KO.from_terms(KO.gather(t, idxA), KO.gather(t, idxB)), f"M={M}: ranges={int(lib.nadm_kinship_ranges(16, 16, M))}")


def _repeated(b, salt):
    """b rows drawn with repeats from the resident ones, the planted rows 2, 4 and 5 among them."""
    idx = np.random.default_rng(salt).integers(0, ROWS, size=b).astype(np.int32)
    idx[[3, b // 2, b - 2]] = [2, 4, 5]
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("K, pimin", [(8, 0.0), (33, 0.05)])
def test_ranges_of_several_chunks(K, pimin):
    """The steady state of a real call: a range that covers several chunks, so that the chunk loop hands the prefetched bytes over,
    stages P again over the previous chunk's rows and accumulates across chunks.  1024 x 1024 rows (the resident ones with repeats) fill
    the chip with their 256 tiles, which leaves M = 3001 in 2 ranges of 6 chunks; the same bounds against float64, n exact.
    OBSERVED on an MI355X: num 6.2e-6 (K = 8) and 1.1e-5 (K = 33) of abs_ab, den 3.9e-6 and 4.2e-6 of den64; bound 3.05e-5."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    b, M = 1024, 3001
    ranges, chunks = int(lib.nadm_kinship_ranges(b, b, M)), (M + 255) // 256
    assert ranges >= 2 and -(-chunks // ranges) >= 2
    Gm, P, Q, dead, xph = _case(M, K)
    idxA, idxB = _repeated(b, 11), _repeated(b, 12)
    t = _terms(M, K, pimin)
    got = _gpu_block(xph.to(dev), M, P, Q, idxA, idxB, pimin)
    _check_block(got, KO.from_terms(KO.gather(t, idxA), KO.gather(t, idxB)),
                 f"ba=bb={b} M={M} K={K} pimin={pimin}: {ranges} ranges of {-(-chunks // ranges)} chunks")
    for a in np.nonzero(idxA == 4)[0]:
        assert not got[0][a].any() and not got[1][a].any() and not got[2][a].any()


@pytest.mark.gpu
@pytest.mark.parametrize("ba, bb, M, K, pimin", [(70, 130, 1027, 30, 0.0), (15, 17, 257, 33, 0.0), (130, 70, 1027, 64, 0.05)])
def test_the_widest_heads(ba, bb, M, K, pimin):
    """kp = 32, 48 and 64: the instantiations with 72, 88 and 104 KB of LDS a block.  OBSERVED on an MI355X: num 6.0e-6, 7.0e-6 and
    1.2e-5 of abs_ab, den 3.6e-6, 2.2e-6 and 2.7e-6 of den64; bound 3.05e-5."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    assert int(lib.nadm_pad_k(K)) in (32, 48, 64)
    Gm, P, Q, dead, xph = _case(M, K)
    idxA, idxB = _rows(ba), _rows(bb, salt=7)
    t = _terms(M, K, pimin)
    got = _gpu_block(xph.to(dev), M, P, Q, idxA, idxB, pimin)
    _check_block(got, KO.from_terms(KO.gather(t, idxA), KO.gather(t, idxB)), f"ba={ba} bb={bb} M={M} K={K} (kp={int(lib.nadm_pad_k(K))}) pimin={pimin}")


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    dev = _dev()
    M, K = 3001, 9
    Gm, P, Q, dead, xph = _case(M, K)
    xp = xph.to(dev)
    idxA, idxB = _rows(130), _rows(70, salt=7)
    a = _gpu_block(xp, M, P, Q, idxA, idxB, 0.05)
    b = _gpu_block(xp, M, P, Q, idxA, idxB, 0.05)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
def test_masked_terms_are_exactly_zero():
    """Ones in the pad bits of every row's last byte (and in the bytes behind it), and another P at the SNPs where every sample of the
    block is missing, leave num, den and n bit-identical."""
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead, xph = _case(M, K)
    idxA, idxB = _rows(70), _rows(130, salt=7)
    clean = _gpu_block(xph.to(dev), M, P, Q, idxA, idxB)
    dirty = _gpu_block(_packed(Gm, dirty=True).to(dev), M, P, Q, idxA, idxB)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    assert (Gm[:, dead] == 3).all()
    P2 = P.copy()
    P2[dead[0]] = np.float32(np.nan)
    P2[dead[1]] = 0.731
    other = _gpu_block(xph.to(dev), M, P2, Q, idxA, idxB)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, other))


@pytest.mark.gpu
def test_transposed_block():
    dev = _dev()
    M, K = 3001, 16
    Gm, P, Q, dead, xph = _case(M, K)
    xp = xph.to(dev)
    idxA, idxB = _rows(70), _rows(130, salt=7)
    t = _terms(M, K, 0.0)
    ab = _gpu_block(xp, M, P, Q, idxA, idxB)
    ba = _gpu_block(xp, M, P, Q, idxB, idxA)
    assert np.array_equal(ab[2], ba[2].T)
    want = KO.from_terms(KO.gather(t, idxA), KO.gather(t, idxB))
    _check_block(ab, want, "block (A, B)")
    _check_block((ba[0].T, ba[1].T, ba[2].T), want, "block (B, A) transposed")


def _close(phi, num64, den64, ab, what):
    """phi against float64 within what the two tolerances allow: |d phi| <= (2^-15 abs_ab + 2^-15 |num64|) / (4 den64) to first order
    (x 1.001 for the second)."""
    want = KO.phi_of(num64, den64)
    assert np.array_equal(np.isnan(phi), np.isnan(want))
    ok = ~np.isnan(want)
    bound = 1.001 * TOL * (ab[ok] + np.abs(num64[ok])) / (4.0 * den64[ok])
    err = np.abs(phi[ok] - want[ok])
    print(f"{what}: max |phi - phi64| = {err.max():.3e}")
    assert (err <= bound).all()


@pytest.mark.gpu
def test_dense_and_pair_forms():
    """kinship() with 64-row blocks on N = 130 agrees with ONE 130 x 130 block within the tolerances, phi is symmetric, its diagonal is
    (1 + f) / 2 for the f that kinship_pairs returns, and kinship_pairs lists exactly the pairs of kinship() at or above the threshold."""
    from neural_admixture_amd import relate
    dev = _dev()
    M, K, N = 1027, 3, 130
    Gm, P, Q, dead, xph = _case(M, K)
    xp = xph[:N].contiguous().to(dev)
    t = KO.gather(_terms(M, K, 0.0), np.arange(N))
    num64, den64, n64, ab = KO.from_terms(t, t)
    one = _gpu_block(xp, M, P, Q[:N], None, None)
    _check_block(one, (num64, den64, n64, ab), "one 130 x 130 block")
    phi, n = relate.kinship(xp, M, P, Q[:N], rows=64)
    phi, n = phi.cpu().numpy(), n.cpu().numpy()
    assert phi.shape == (N, N) and phi.dtype == np.float64 and n.dtype == np.int32
    assert np.array_equal(n, n64) and np.array_equal(n, one[2])
    assert np.array_equal(phi, phi.T, equal_nan=True)
    _close(phi, num64, den64, ab, "dense form, rows = 64")
    _close(KO.phi_of(one[0], one[1]), num64, den64, ab, "one block")
    for thr in (relate.MIN_PHI, 0.0):
        i, j, p, nn, f = relate.kinship_pairs(xp, M, P, Q[:N], min_phi=thr, rows=64)
        i, j, p, nn, f = (x.cpu().numpy() for x in (i, j, p, nn, f))
        wi, wj = np.nonzero(np.triu(phi >= thr, 1))
        assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(p, phi[wi, wj]) and np.array_equal(nn, n[wi, wj])
        assert np.array_equal(np.diagonal(phi), (1.0 + f) / 2.0, equal_nan=True) and f.shape == (N,)
    assert len(wi) > 100 and np.isnan(f[4])                  # (the all-missing sample has no coefficient)
    i2, j2, p2, nn2, f2 = relate.kinship_pairs(xp, M, P, Q[:N], min_phi=0.0)           # one block of all 130 rows
    assert np.array_equal(i2.cpu().numpy(), np.nonzero(np.triu(KO.phi_of(one[0], one[1]) >= 0.0, 1))[0])


@pytest.mark.gpu
def test_pedigree_on_the_gpu():
    """The pedigree packed with the project's packer: every pair falls in the oracle's band, phi is within 2e-5 of the oracle's."""
    from neural_admixture_amd import relate
    dev = _dev()
    Gm, P, Q, (phi64, num64, den64, n64, ab) = _pedigree()
    phi, n = relate.kinship(_packed(Gm).to(dev), Gm.shape[1], P, Q)
    phi, n = phi.cpu().numpy(), n.cpu().numpy()
    err = np.abs(phi - phi64)
    print(f"pedigree: max |phi - phi64| = {err.max():.3e}")
    assert np.array_equal(n, n64)
    assert err.max() <= 2e-5
    for a in range(15):
        for b in range(15):
            assert KO.band(phi[a, b]) == KO.band(phi64[a, b]), (a, b, phi[a, b], phi64[a, b])
    i, j, p, nn, f = relate.kinship_pairs(_packed(Gm).to(dev), Gm.shape[1], P, Q)
    pairs = set(zip(i.cpu().tolist(), j.cpu().tolist()))
    assert pairs >= set(KO.PED_PARENT_CHILD + KO.PED_SIBS + KO.PED_DUPLICATE)
    assert [c for _, _, c in relate.band_counts(p.cpu().numpy())][:2] == [1, 5]


@pytest.mark.gpu
def test_engine_kinship_equals_the_library_free_form_and_leaves_the_parameters():
    import neural_admixture_amd as na
    from neural_admixture_amd import relate
    from oracle import nadm_oracle as O
    dev = _dev()
    N, M, ks, Hd, C_ = 96, 3001, [3, 5], 32, 8
    Gm = O.synth_genotypes(N, M, 5, seed=3, missing=0.05)
    Gm[17] = Gm[3]                                                                # a duplicate: a pair to find
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
        got = e.kinship(head=head, min_phi=0.0, pimin=0.01)
        want = relate.kinship_pairs(e.xp, M, e.P(head).clone(), Qh, min_phi=0.0, pimin=0.01)
        assert all(torch.equal(a, b) or (a.dtype.is_floating_point and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))) for a, b in zip(got, want))
        assert got[0].numel() > 10 and got[4].shape == (N,)
        k = (got[0] == 3) & (got[1] == 17)
        assert int(k.sum()) == 1 and float(got[2][k]) > 0.3
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_kinship_end_to_end(tmp_path, caplog):
    """The `kinship` mode on the bundled demo .bed (its first sample written over the second: a duplicate to find) with .Q and .P files
    written here: .kin and .inbreed hold what kinship_pairs returns, the bands and the warning are logged."""
    from neural_admixture_amd import cli, relate
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    d = np.load(f"{G}/demo_k3.npz")
    N, M, K = int(d["N"]), int(d["M"]), 3
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    bed = np.array(d["bed_bytes"], dtype=np.uint8, copy=True)
    body = bed[3:].reshape(M, (N + 3) // 4)
    body[:, 0] = (body[:, 0] & ~np.uint8(0x0C)) | ((body[:, 0] & np.uint8(0x03)) << 2)       # sample 1 := sample 0
    bed.tofile(tmp_path / "demo.bed")
    rng = np.random.default_rng(5)
    Q = rng.dirichlet(np.full(K, 0.8), size=N).astype(np.float32)
    Q[1] = Q[0]
    P = rng.uniform(0.05, 0.95, size=(M, K)).astype(np.float32)
    np.savetxt(tmp_path / "run.3.Q", Q, delimiter=" ")
    np.savetxt(tmp_path / "run.3.P", P, delimiter=" ")
    caplog.set_level(logging.INFO)
    assert cli.main(["kinship", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(tmp_path), "--name", "run", "--k", "3",
                     "--out_name", "rel", "--min_phi", "0.1"]) == 0
    Qr = np.loadtxt(tmp_path / "run.3.Q", dtype=np.float32, ndmin=2)
    Pr = np.loadtxt(tmp_path / "run.3.P", dtype=np.float32, ndmin=2)
    again = read_bed_packed(str(tmp_path / "demo.bed"), dev, keep_on_device=True)
    i, j, p, n, f = relate.kinship_pairs(again.packed, M, Pr, Qr, min_phi=0.1)
    kin = np.loadtxt(tmp_path / "rel.3.kin", ndmin=2)
    inb = np.loadtxt(tmp_path / "rel.3.inbreed")
    assert kin.shape == (i.numel(), 4) and i.numel() >= 1
    assert np.array_equal(kin[:, 0], i.cpu().numpy()) and np.array_equal(kin[:, 1], j.cpu().numpy())
    assert np.array_equal(kin[:, 2], p.cpu().numpy()) and np.array_equal(kin[:, 3], n.cpu().numpy())
    assert np.array_equal(inb, f.cpu().numpy(), equal_nan=True) and inb.shape == (N,)
    assert (kin[0, 0], kin[0, 1]) == (0, 1) and kin[0, 2] > 0.354
    first = (tmp_path / "rel.3.kin").read_text().splitlines()[0].split()
    assert first[:2] == ["0", "1"] and first[3] == str(int(n[0])) and float(first[2]) == float(p[0])      # integers as integers
    msgs = [r.getMessage() for r in caplog.records]
    assert any("duplicate or twin (>= 0.3536)" in m for m in msgs) and any("third degree (>= 0.0442)" in m for m in msgs)
    assert any("second-degree relatives or closer" in m for m in msgs)
