"""IBD-sharing probabilities given ancestry (nadm_ibd, relate.ibd_block / ibd_of / ibd_pairs / relation / write_ibd, Engine.ibd, the
`kinship --ibd` mode of the command line).  The float64 numpy restatement lives in tests/ibd_oracle.py, the shared data (pedigree,
edge-case matrix) in tests/kinship_oracle.py.

The bounds of a block against float64 are derived, not measured, with eps = 2^-15 as for nadm_kinship:
    ibs0 exact;  |k2num - k2num64| <= eps abs2;  |k2den - k2den64| <= eps k2den64;  |exp0 - exp0_64| <= eps exp0_64
abs2_ab = sum_j mag_a mag_b with mag = m (|gD| + v (1 + |f|)), the UN-CANCELLED magnitude of e = gD - v (1 + f): e is a difference
formed in fp32, and where it nearly cancels its rounding error is relative to mag, not to |e|.  The terms of k2den and exp0 are all
>= 0, so the float64 value is its own sum of magnitudes.  Two round-to-nearest bf16 pieces carry a value to 2^-17 relative; the three
kept products hi.hi + hi.lo + lo.hi therefore miss at most 3 * 2^-17 ~ 2.3e-5 of a term's magnitude, the rest of 2^-15 ~ 3.05e-5 is
room for forming the operand in fp32 and for the fp32 accumulation inside a range.
OBSERVED on an MI355X over all block tests (each case prints its three ratios before it asserts): k2num at
most 2.2e-6 of abs2, k2den at most 3.7e-6 of k2den64, exp0 at most 5.3e-6 of exp0_64, against the bound 3.05e-5."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ibd_oracle as IO  # noqa: E402
import kinship_oracle as KO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2.0 ** -15
ROWS = 140                   # resident rows of the GPU cases
# (ba, bb, M, K, pimin): a lone pair, ragged tiles on each side, a ragged last chunk, one and several ranges, kp = 4 / 8 / 12 / 16, the mask
BLOCKS = [(1, 1, 257, 2, 0.0), (16, 16, 1027, 3, 0.0), (15, 17, 3001, 8, 0.05), (70, 130, 257, 9, 0.0), (130, 70, 1027, 16, 0.05),
          (130, 70, 3001, 2, 0.0)]


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_on_a_case_worked_out_by_hand():
    """Two samples, three SNPs, K = 2, f = 0.  Q_a = (1, 0), Q_b = (1/2, 1/2); P = (1/2, 1/2), (1/4, 3/4), (1/2, 0).
        pi_a = 1/2, 1/4, 1/2         pi_b = 1/2, 1/2, 1/4
        g_a  = 2, 1, missing         g_b  = 2, 0, 1
        v_a  = 1/4, 3/16, -          v_b  = 1/4, 1/4, 3/16
        gD_a = 1/2, 0, -             gD_b = 1/2, 1/2, 0
        e_a  = 1/4, -3/16, 0         e_b  = 1/4, 1/4, -3/16
    k2num_ab = 1/16 - 3/64 = 1/64, k2den_ab = 1/16 + 3/64 = 7/64, k2 = 1/7; no opposite homozygotes: ibs0_ab = 0;
    exp0_ab = (1/16 + 1/16) + (1/16 * 1/4 + 9/16 * 1/4) = 1/8 + 10/64 = 9/32.  phi_ab = 0.26795 >= 2^-2.5: k0 = 0 / (9/32) = 0, k1 = 6/7.
    k2num_aa = 1/16 + 9/256 = 25/256, k2den_aa = 1/16 + 9/256.  With pimin = 0.3 the two pi = 1/4 drop out: only SNP 0 is left to the
    pair, k2num_ab = k2den_ab = 1/16, k2 = 1, exp0_ab = 1/8, phi_ab = 1, k0 = 0, k1 = 0."""
    Gm = np.asarray([[2, 1, 3], [2, 0, 1]], dtype=np.uint8)
    Q = np.asarray([[1.0, 0.0], [0.5, 0.5]], dtype=np.float32)
    P = np.asarray([[0.5, 0.5], [0.25, 0.75], [0.5, 0.0]], dtype=np.float32)
    f = np.zeros(2, dtype=np.float32)
    phi = KO.kinship(Gm, P, Q)[0]
    e, vm, u, w, z0, z2, mag = IO.terms(Gm, P, Q, f)
    assert np.array_equal(e, [[0.25, -3 / 16, 0.0], [0.25, 0.25, -3 / 16]])
    (k0, k1, k2), (k2num, k2den, ibs0, exp0, abs2) = IO.ibd(Gm, P, Q, f, phi)
    assert abs(k2num[0, 1] - 1 / 64) <= 1e-15 and abs(k2den[0, 1] - 7 / 64) <= 1e-15 and abs(k2[0, 1] - 1 / 7) <= 1e-15
    assert ibs0[0, 1] == 0 and abs(exp0[0, 1] - 9 / 32) <= 1e-15
    assert phi[0, 1] >= 2.0 ** -2.5 and k0[0, 1] == 0.0 and abs(k1[0, 1] - 6 / 7) <= 1e-15
    assert abs(k2num[0, 0] - 25 / 256) <= 1e-15 and abs(k2den[0, 0] - 25 / 256) <= 1e-15 and np.array_equal(k2num, k2num.T)
    assert abs(abs2[0, 1] - ((0.5 + 0.25) ** 2 + (3 / 16) * (0.5 + 0.25))) <= 1e-15
    phi = KO.kinship(Gm, P, Q, pimin=0.3)[0]
    (k0, k1, k2), (k2num, k2den, ibs0, exp0, abs2) = IO.ibd(Gm, P, Q, f, phi, pimin=0.3)
    assert k2num[0, 1] == 1 / 16 and k2den[0, 1] == 1 / 16 and k2[0, 1] == 1.0 and exp0[0, 1] == 1 / 8 and ibs0[0, 1] == 0
    assert phi[0, 1] == 1.0 and k0[0, 1] == 0.0 and k1[0, 1] == 0.0
    none = np.full((2, 3), 3, dtype=np.uint8)
    (k0, k1, k2), sums = IO.ibd(none, P, Q, np.asarray([np.nan, 0.0], dtype=np.float32), KO.kinship(none, P, Q)[0])
    assert np.isnan(k0).all() and np.isnan(k1).all() and np.isnan(k2).all() and not any(s.any() for s in sums)


def test_library_free_ibd_of_is_the_oracles():
    """relate.ibd_of (torch) against the oracle's on values that take every branch: phi either side of the first-degree edge, k2den = 0,
    exp0 = 0."""
    from neural_admixture_amd import relate
    phi = np.asarray([0.5, 0.25, 2.0 ** -2.5, 0.17, 0.0, 0.3, 0.01, np.nan])
    k2num = np.asarray([1.0, 0.2, -0.01, 0.0, 0.03, 0.1, 0.5, 0.1])
    k2den = np.asarray([1.1, 0.9, 1.0, 2.0, 0.0, 1.0, 0.0, 1.0])
    ibs0 = np.asarray([0, 3, 0, 7, 1, 2, 0, 1], dtype=np.int32)
    exp0 = np.asarray([9.0, 11.0, 8.0, 9.5, 2.0, 0.0, 1.0, 2.0])
    want = IO.ibd_of(phi, k2num, k2den, ibs0, exp0)
    got = relate.ibd_of(*(torch.from_numpy(a) for a in (phi, k2num, k2den, ibs0, exp0)))
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and np.array_equal(g.numpy(), w, equal_nan=True)
    assert np.isnan(want[2][4]) and np.isnan(want[0][5]) and np.isnan(want[0][7]) and want[0][3] == 1.0 - 4 * 0.17


@functools.lru_cache(maxsize=None)
def _pedigree():
    Gm, P, Q = KO.make_pedigree(0)
    phi = KO.kinship(Gm, P, Q)[0]
    f = (2.0 * np.diagonal(phi) - 1.0).astype(np.float32)
    return Gm, P, Q, phi, f, IO.ibd(Gm, P, Q, f, phi)


def test_oracle_on_the_pedigree():
    """The estimators themselves, in float64, with the true Q and P and f from the float64 kinship.  Bands (values observed with this
    script in brackets): parent-child ibs0 = 0 so k0 = 0 exactly, |k2| <= 0.06 [-0.019 .. -0.022]; sibs k0, k2 in 0.25 +- 0.08
    [0.204, 0.214]; duplicate k0 = 0, k2 = 1 +- 0.06 [1.004]; the 99 unrelated pairs k0 in 1 +- 0.15 [0.902 .. 1.123], |k2| <= 0.08
    [-0.062 .. 0.059]; `relation` labels the five first-degree pairs."""
    from neural_admixture_amd import relate
    Gm, P, Q, phi, f, ((k0, k1, k2), (k2num, k2den, ibs0, exp0, abs2)) = _pedigree()
    for i, j in KO.PED_PARENT_CHILD:
        assert ibs0[i, j] == 0 and k0[i, j] == 0.0 and abs(k2[i, j]) <= 0.06, (i, j, k0[i, j], k2[i, j])
    for i, j in KO.PED_SIBS:
        assert abs(k0[i, j] - 0.25) <= 0.08 and abs(k2[i, j] - 0.25) <= 0.08, (i, j, k0[i, j], k2[i, j])
    for i, j in KO.PED_DUPLICATE:
        assert k0[i, j] == 0.0 and abs(k2[i, j] - 1.0) <= 0.06, (i, j, k0[i, j], k2[i, j])
    related = set(KO.PED_PARENT_CHILD + KO.PED_SIBS + KO.PED_DUPLICATE)
    unrelated = [(i, j) for i in range(15) for j in range(i + 1, 15) if (i, j) not in related]
    assert len(unrelated) == 99
    for i, j in unrelated:
        assert abs(k0[i, j] - 1.0) <= 0.15 and abs(k2[i, j]) <= 0.08, (i, j, k0[i, j], k2[i, j])
    assert np.allclose(k0 + k1 + k2, 1.0, rtol=0, atol=1e-12)
    first = KO.PED_PARENT_CHILD + KO.PED_SIBS
    labels = relate.relation([phi[i, j] for i, j in first], [k0[i, j] for i, j in first])
    assert labels == ["parent-offspring"] * 4 + ["full siblings"]
    assert relate.relation([phi[2, 14]], [k0[2, 14]]) == ["duplicate or twin"]


def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_ibd", "nadm_ibd_ranges", "nadm_ibd_scratch_floats"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "#define NADM_IBD_MAX_ROWS 4096" in header


def test_ranges_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    rg, f = lib.nadm_ibd_ranges, lib.nadm_ibd_scratch_floats
    Ms = (1, 255, 256, 257, 513, 1027, 3001, 70000, 500000, 600000, 5000000)
    bs = (1, 15, 16, 17, 63, 64, 65, 70, 128, 130, 1024, 4096)
    assert int(rg(16, 16, 256)) == 1 and int(rg(16, 16, 257)) == 2            # one tile: a range per chunk while that fills the chip
    assert int(rg(1024, 1024, 500000)) >= 2 and int(rg(16, 16, 5000000)) >= 2
    for M in Ms:
        chunks = (M + 255) // 256
        for ba in bs:
            for bb in bs:
                r = int(rg(ba, bb, M))
                tiles = ((ba + 63) // 64) * ((bb + 63) // 64)
                assert 1 <= r <= chunks and -(-chunks // r) <= 1024            # at most 2^18 SNPs in one fp32 accumulator: ibs0 exact
                assert int(f(ba, bb, M)) >= r * tiles * 4 * 64 * 64
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
    for M in range(1, 9000, 7):
        assert int(f(130, 70, M + 7)) >= int(f(130, 70, M)) and int(f(16, 16, M + 7)) >= int(f(16, 16, M))
    for bad in ((0, 4, 100), (4, 0, 100), (4, 4, 0), (4097, 4, 100), (4, 4097, 100), (-1, 4, 100)):
        assert int(f(*bad)) == 0 and int(rg(*bad)) == 0


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 4), 0.25)
    P = torch.full((50, 4), 0.25)
    fv = torch.zeros(4)
    outs = [torch.empty((4, 4), dtype=torch.float64) for _ in range(3)]
    ibs0 = torch.empty((4, 4), dtype=torch.int32)
    scratch = torch.empty(4 * 4096)
    keep = (xp, P, Q, fv, outs, ibs0, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idxA=None, ba=4, idxB=None, bb=4, M=50, P=P.data_ptr(), k=3, kp=4, QA=Q.data_ptr(), QB=Q.data_ptr(),
             q_stride=4, fA=fv.data_ptr(), fB=fv.data_ptr(), pimin=0.0, k2num=outs[0].data_ptr(), k2den=outs[1].data_ptr(),
             ibs0=ibs0.data_ptr(), exp0=outs[2].data_ptr(), scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(P=None), "null pointer"), (dict(QA=None), "null pointer"), (dict(QB=None), "null pointer"),
    (dict(fA=None), "null pointer"), (dict(fB=None), "null pointer"), (dict(k2num=None), "null pointer"), (dict(k2den=None), "null pointer"),
    (dict(ibs0=None), "null pointer"), (dict(exp0=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(ba=0), "empty block"), (dict(bb=-3), "empty block"), (dict(M=0), "empty block"),
    (dict(ba=4097), "must be <= NADM_IBD_MAX_ROWS"), (dict(bb=100000), "must be <= NADM_IBD_MAX_ROWS"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(k=17, kp=24, q_stride=24), "K must be <= 16 (a sample's Q row lives in"),
    (dict(pimin=-1e-3), "pimin must be in [0, 0.5)"), (dict(pimin=0.5), "pimin must be in [0, 0.5)"), (dict(pimin=float("nan")), "pimin must be in [0, 0.5)"),
    (dict(unaligned="QA"), "must be 16-byte aligned"), (dict(unaligned="P"), "must be 16-byte aligned"), (dict(unaligned="k2num"), "8-byte"),
    (dict(unaligned="exp0"), "8-byte"), (dict(unaligned="fA", by=2), "4-byte aligned"), (dict(unaligned="ibs0", by=2), "4-byte aligned"),
])
def test_ibd_refuses_before_any_launch(change, message):
    """Every refusal of nadm_ibd is decided on the host: it is reported with its message on a machine without a GPU (where a launch
    would fail with another one)."""
    from neural_admixture_amd._lib import lib, check
    assert int(lib.nadm_pad_k(17)) == 24
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += change.get("by", 4)
    else:
        a.update(change)
    status = lib.nadm_ibd(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_ibd"):
        check(status, "ibd")
    del keep


def test_cli_ibd_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """`kinship --ibd --k 17` and a --po_k0 outside (0, 0.25) end the run, naming the limit, before a file is looked for: the .bed named
    here does not exist, and the reader is a stand-in that fails the test when called.  Without --ibd the mode parses as before."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "absent.bed"
    base = ["kinship", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_kinship_args(base[1:])
    assert a.min_phi == 2.0 ** -4.5 and a.pimin == 0.0 and a.out_name is None and a.threads == 1 and a.ibd is False and a.po_k0 == 0.1
    a = cli.parse_kinship_args(base[1:] + ["--ibd", "--po_k0", "0.05"])
    assert a.ibd is True and a.po_k0 == 0.05

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(SystemExit, match=r"kinship --ibd needs K <= 16"):
        cli.main(base[:2] + ["17"] + base[3:] + ["--ibd"])
    for bad in ("0", "0.25", "-0.1", "nan"):
        with pytest.raises(SystemExit, match=r"--po_k0 must be in \(0, 0.25\)"):
            cli.main(base + ["--ibd", "--po_k0", bad])
    with pytest.raises(SystemExit, match=r"run\.17\.P not found"):            # without --ibd a wide head goes as far as it did
        cli.main(base[:2] + ["17"] + base[3:])
    with pytest.raises(SystemExit, match=r"run\.3\.P not found"):
        cli.main(base + ["--ibd"])


def test_sharded_engines_refuse_ibd():
    """Engine.ibd is single-GPU; the check comes first, so a stand-in without any device state shows it."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan = "dp", 2, None
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.ibd()
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.ibd(0, 0.1)


def test_relation_and_write_ibd(tmp_path):
    from neural_admixture_amd import relate
    assert relate.PO_MAX_K0 == 0.1
    phi = [0.5, 0.25, 0.26, 0.2, 0.1, 0.05, 0.01, 0.25]
    k0 = [0.0, 0.02, 0.21, 0.0999, 0.5, 0.7, 1.0, 0.1]
    labels = relate.relation(phi, k0)
    assert labels == ["duplicate or twin", "parent-offspring", "full siblings", "parent-offspring", "second degree", "third degree",
                      "unrelated", "full siblings"]
    assert relate.relation(phi[1:3], k0[1:3], 0.22) == ["parent-offspring"] * 2
    assert dict(relate.relation_counts(labels)) == {"duplicate or twin": 1, "parent-offspring": 2, "full siblings": 2, "second degree": 1,
                                                    "third degree": 1, "unrelated": 1}
    path = tmp_path / "x.ibd"
    i, j = np.asarray([0, 3]), np.asarray([1, 7])
    k = [np.asarray(v) for v in ([0.0, 0.1 + 0.2], [-0.004, 0.5], [1.004, 1 / 3])]
    relate.write_ibd(path, i, j, np.asarray([0.5, 0.25]), np.asarray([2900, 17], dtype=np.int32), *k, np.asarray([0, 5], dtype=np.int32),
                     ["duplicate or twin", "full siblings"])
    lines = path.read_text().splitlines()
    assert lines[0] == "0 1 0.5 2900 0 -0.0040000000000000001 1.004 0 duplicate_or_twin"
    cols = lines[1].split()
    assert cols[:2] == ["3", "7"] and cols[3] == "17" and cols[7] == "5" and cols[8] == "full_siblings" and len(lines) == 2
    assert [float(c) for c in cols[4:7]] == [0.1 + 0.2, 0.5, 1 / 3] and float(cols[2]) == 0.25


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS resident rows with the planted cases of kinship_oracle.make_edge_case, their inbreeding coefficients (seeded uniform(-0.2,
    0.5), NaN for the all-missing row 4) and the packed rows; the tests leave them as they are."""
    Gm, P, Q, dead = KO.make_edge_case(ROWS, M, K)
    f = np.random.default_rng(7 * M + K).uniform(-0.2, 0.5, size=ROWS).astype(np.float32)
    f[4] = np.float32(np.nan)
    return Gm, P, Q, dead, f, _packed(Gm)


@functools.lru_cache(maxsize=None)
def _terms(M, K, pimin):
    Gm, P, Q, _, f, _ = _case(M, K)
    return IO.terms(Gm, P, Q, f, pimin)


def _rows(b, salt=0):
    """test_kinship._rows, restated: a permutation of the resident rows with the one-hot row 2, the all-missing row 4 and the 7-call
    row 5 in it, cut to b, the last entry a duplicate of the first; b = 1 is row 7."""
    if b == 1:
        return np.asarray([7], dtype=np.int32)
    perm = np.random.default_rng(100 * b + salt).permutation(ROWS)
    perm = np.concatenate([[2, 4, 5], perm[(perm != 2) & (perm != 4) & (perm != 5)]])[:b - 1]
    perm = perm[np.random.default_rng(100 * b + salt + 1).permutation(b - 1)]
    perm = np.concatenate([perm, perm[:1]])
    return perm.astype(np.int32)


def _gpu_block(xp, M, P, Q, f, idxA, idxB, pimin=0.0, same_list=False):
    """One nadm_ibd call -> (k2num, k2den float64, ibs0 int32, exp0 float64) numpy [ba, bb]; Q [rows, K] and f [rows] belong to the
    resident rows."""
    from neural_admixture_amd import project, relate
    dev = xp.device
    K = Q.shape[1]
    Pp = project.pad_P(P, dev)
    kp = Pp.shape[1]

    def side(idx):
        i = None if idx is None else torch.from_numpy(idx).to(dev)
        Qs, fs = (Q, f) if idx is None else (Q[idx], f[idx])
        return i, project.pad_Q(Qs, len(Qs), K, kp, dev), torch.from_numpy(np.ascontiguousarray(fs)).to(dev)
    ia, QA, fA = side(idxA)
    ib, QB, fB = (ia, QA, fA) if same_list else side(idxB)
    k2num, k2den, exp0, ibs0 = relate.ibd_block(xp, M, Pp, K, ia, QA, fA, ib, QB, fB, pimin)
    torch.cuda.synchronize()
    return k2num.cpu().numpy(), k2den.cpu().numpy(), ibs0.cpu().numpy(), exp0.cpu().numpy()


def _check_block(got, want, what):
    """ibs0 exact and the three bounds of the module docstring; prints the three largest ratios before it asserts."""
    k2num, k2den, ibs0, exp0 = got
    n64, d64, i64, x64, abs2 = want
    en, ed, ex = np.abs(k2num - n64), np.abs(k2den - d64), np.abs(exp0 - x64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = float(np.nanmax(np.where(abs2 > 0, en / abs2, 0.0)))
        rd = float(np.nanmax(np.where(d64 > 0, ed / d64, 0.0)))
        rx = float(np.nanmax(np.where(x64 > 0, ex / x64, 0.0)))
    print(f"{what}: max |k2num - k2num64| / abs2 = {rn:.3e}, max |k2den - k2den64| / k2den64 = {rd:.3e}, "
          f"max |exp0 - exp0_64| / exp0_64 = {rx:.3e}; bound 2^-15 = {TOL:.3e}")
    assert np.array_equal(ibs0, i64)
    assert (en <= TOL * abs2).all()
    assert (ed <= TOL * d64).all()
    assert (ex <= TOL * x64).all()
    return rn, rd, rx


def _all_zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ba, bb, M, K, pimin", BLOCKS)
def test_block_against_float64(ba, bb, M, K, pimin):
    """ibs0 exact, k2num, k2den and exp0 within the derived bounds (module docstring); the row and the column of the all-missing
    sample, whose f is NaN, are all zero bits.  OBSERVED on an MI355X over BLOCKS: max |k2num - k2num64| / abs2 3.5e-7 .. 1.9e-6,
    max |k2den - k2den64| / k2den64 1.4e-6 .. 3.7e-6, max |exp0 - exp0_64| / exp0_64 3.3e-7 .. 5.0e-6; bound 3.05e-5; 2, 5 and 12 ranges."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    Gm, P, Q, dead, f, xph = _case(M, K)
    idxA, idxB = _rows(ba), _rows(bb, salt=7)
    if ba > 2:
        assert Q[idxA].max(axis=1).max() == 1.0 and (Gm[idxA] == 3).all(axis=1).any() and ((Gm[idxA] != 3).sum(axis=1) == 7).any()
        assert idxA[-1] == idxA[0] and (P[0] == 0).all() and (P[1] == 1).all() and np.isnan(f[4])
    t = _terms(M, K, pimin)
    want = IO.from_terms(IO.gather(t, idxA), IO.gather(t, idxB))
    got = _gpu_block(xph.to(dev), M, P, Q, f, idxA, idxB, pimin)
    _check_block(got, want, f"ba={ba} bb={bb} M={M} K={K} pimin={pimin} ranges={int(lib.nadm_ibd_ranges(ba, bb, M))}")
    if ba > 2:
        assert (idxA == 4).any() and (idxB == 4).any() and want[2].any()
        for a in np.nonzero(idxA == 4)[0]:
            assert all(_all_zero_bits(g[a]) for g in got)
        for b in np.nonzero(idxB == 4)[0]:
            assert all(_all_zero_bits(g[:, b]) for g in got)


def _repeated(b, salt):
    """b rows drawn with repeats from the resident ones, the planted rows 2, 4 and 5 among them."""
    idx = np.random.default_rng(salt).integers(0, ROWS, size=b).astype(np.int32)
    idx[[3, b // 2, b - 2]] = [2, 4, 5]
    return idx


@pytest.mark.gpu
def test_ranges_of_several_chunks():
    """The steady state of the chunk loop: 1024 x 1024 rows (the resident ones with repeats) fill the chip with their 256 tiles, which
    leaves M = 3001 in ranges of several chunks.  The same bounds against float64.  OBSERVED on an MI355X (2 ranges of 6 chunks):
    k2num 1.7e-6 of abs2, k2den 3.2e-6 of k2den64, exp0 3.4e-6 of exp0_64; bound 3.05e-5."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    b, M, K = 1024, 3001, 8
    ranges, chunks = int(lib.nadm_ibd_ranges(b, b, M)), (M + 255) // 256
    assert ranges >= 2 and -(-chunks // ranges) >= 2
    Gm, P, Q, dead, f, xph = _case(M, K)
    idxA, idxB = _repeated(b, 11), _repeated(b, 12)
    t = _terms(M, K, 0.0)
    got = _gpu_block(xph.to(dev), M, P, Q, f, idxA, idxB)
    _check_block(got, IO.from_terms(IO.gather(t, idxA), IO.gather(t, idxB)),
                 f"ba=bb={b} M={M} K={K}: {ranges} ranges of {-(-chunks // ranges)} chunks")
    for a in np.nonzero(idxA == 4)[0]:
        assert all(_all_zero_bits(g[a]) for g in got)


@pytest.mark.gpu
def test_more_than_one_range():
    from neural_admixture_amd._lib import lib
    dev = _dev()
    M = next(m for m in range(1, 100000) if int(lib.nadm_ibd_ranges(16, 16, m)) >= 2)
    K = 3
    Gm, P, Q, dead, f, xph = _case(M, K)
    idxA, idxB = _rows(16), _rows(16, salt=7)
    t = _terms(M, K, 0.0)
    got = _gpu_block(xph.to(dev), M, P, Q, f, idxA, idxB)
    _check_block(got, IO.from_terms(IO.gather(t, idxA), IO.gather(t, idxB)), f"M={M}: ranges={int(lib.nadm_ibd_ranges(16, 16, M))}")


@pytest.mark.gpu
def test_same_list_on_both_sides_rows_without_a_gather_list_and_the_transposed_block():
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead, f, xph = _case(M, K)
    xp = xph.to(dev)
    idx = _rows(70)
    t = IO.gather(_terms(M, K, 0.0), idx)
    got = _gpu_block(xp, M, P, Q, f, idx, None, same_list=True)
    _check_block(got, IO.from_terms(t, t), "idxA is idxB, QA is QB, fA is fB (70 rows)")
    assert np.array_equal(got[2], got[2].T) and not np.diagonal(got[2]).any()
    two = _gpu_block(xp, M, P, Q, f, idx, idx.copy())
    assert all(np.array_equal(a, b) for a, b in zip(got, two))
    t = _terms(M, K, 0.0)
    full = _gpu_block(xp, M, P, Q, f, None, None)
    _check_block(full, IO.from_terms(t, t), f"rows 0..{ROWS} without a gather list")
    assert np.array_equal(full[2], full[2].T) and not np.diagonal(full[2]).any()
    idxA, idxB = _rows(70), _rows(130, salt=7)
    want = IO.from_terms(IO.gather(t, idxA), IO.gather(t, idxB))
    ab = _gpu_block(xp, M, P, Q, f, idxA, idxB)
    ba = _gpu_block(xp, M, P, Q, f, idxB, idxA)
    assert np.array_equal(ab[2], ba[2].T)
    _check_block(ab, want, "block (A, B)")
    _check_block(tuple(x.T for x in ba), want, "block (B, A) transposed")


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    dev = _dev()
    M, K = 3001, 9
    Gm, P, Q, dead, f, xph = _case(M, K)
    xp = xph.to(dev)
    idxA, idxB = _rows(130), _rows(70, salt=7)
    a = _gpu_block(xp, M, P, Q, f, idxA, idxB, 0.05)
    b = _gpu_block(xp, M, P, Q, f, idxA, idxB, 0.05)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].any() and a[3].any()


@pytest.mark.gpu
def test_masked_terms_are_exactly_zero():
    """Ones in the pad bits of every row's last byte (and in the bytes behind it), another P (a NaN among it) at the SNPs where every
    sample is missing, and another f for the all-missing row leave the four outputs bit-identical."""
    dev = _dev()
    M, K = 1027, 8
    Gm, P, Q, dead, f, xph = _case(M, K)
    idxA, idxB = _rows(70), _rows(130, salt=7)
    clean = _gpu_block(xph.to(dev), M, P, Q, f, idxA, idxB)
    dirty = _gpu_block(_packed(Gm, dirty=True).to(dev), M, P, Q, f, idxA, idxB)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, dirty))
    assert (Gm[:, dead] == 3).all()
    P2 = P.copy()
    P2[dead[0]] = np.float32(np.nan)
    P2[dead[1]] = 0.731
    other = _gpu_block(xph.to(dev), M, P2, Q, f, idxA, idxB)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, other))
    for v in (0.3, np.inf, -7.0):
        f2 = f.copy()
        f2[4] = np.float32(v)
        again = _gpu_block(xph.to(dev), M, P, Q, f2, idxA, idxB)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(clean, again))


@pytest.mark.gpu
def test_rows_past_4_gib_and_a_side_stream():
    """The compact 140-row matrix against the same rows 2^25 bytes apart (rows 64.. start beyond 2^31 bytes, rows 128.. beyond 2^32; the
    4096 bytes at a row's start are 0xFF with the compact row over them, so the slack next to the data holds set pad bits), called on a
    side stream: bit-identical, with a gather list and without one.  Built the way tests/test_placement.py builds its wide matrix."""
    dev = _dev()
    M, K = 1027, 8
    wide_ld, head = 1 << 25, 4096
    Gm, P, Q, dead, f, xph = _case(M, K)
    assert 127 * wide_ld < 2 ** 32 <= 128 * wide_ld < (ROWS - 1) * wide_ld and xph.shape[1] <= head
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = ROWS * wide_ld
    if free < need + (2 << 30):
        pytest.skip(f"the wide matrix needs {need / 2 ** 30:.2f} GiB + 2 GiB of free HBM, {free / 2 ** 30:.2f} GiB are free")
    xp = xph.to(dev)
    idx = _rows(130)
    assert (idx >= 128).any() and (idx < 64).any()
    want = [_gpu_block(xp, M, P, Q, f, idx, _rows(70, salt=7)), _gpu_block(xp, M, P, Q, f, None, None)]
    _check_block(want[1], IO.from_terms(_terms(M, K, 0.0), _terms(M, K, 0.0)), "compact, rows 0..140")
    buf = torch.empty((ROWS, wide_ld), dtype=torch.uint8, device=dev)
    assert buf.is_contiguous() and buf.stride(0) == wide_ld
    buf[:, :head] = 0xFF
    buf[:, : xp.shape[1]] = xp
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = [_gpu_block(buf, M, P, Q, f, idx, _rows(70, salt=7)), _gpu_block(buf, M, P, Q, f, None, None)]
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g, w))
    del buf
    torch.cuda.empty_cache()


def _f32(inb):
    """The f ibd_pairs hands the library: float32, NaN (a sample without an observed call) replaced by 0."""
    f = np.asarray(inb, dtype=np.float64).copy()
    f[np.isnan(f)] = 0.0
    return f.astype(np.float32)


@pytest.mark.gpu
def test_pedigree_on_the_gpu():
    """ibd_pairs on the pedigree packed with the project's packer: the first five results are kinship_pairs' bit for bit; k0 and k2 are
    within 1e-4 of the float64 oracle evaluated at the GPU's own f and phi (so that the comparison measures the new sums, not
    nadm_kinship's); the five first-degree labels are right and the duplicate has k2 > 0.9.  OBSERVED on an MI355X: max |k0 - k0_64|
    7.4e-9, max |k2 - k2_64| 4.0e-7 over the 6 listed pairs."""
    from neural_admixture_amd import relate
    dev = _dev()
    Gm, P, Q, phi64, f64, _ = _pedigree()
    xp = _packed(Gm).to(dev)
    want5 = relate.kinship_pairs(xp, Gm.shape[1], P, Q)
    got = relate.ibd_pairs(xp, Gm.shape[1], P, Q)
    assert len(got) == 9
    for a, b in zip(got[:5], want5):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    i, j, phi, n, inb, k0, k1, k2, ibs0 = (x.cpu().numpy() for x in got)
    assert k0.dtype == np.float64 and k2.dtype == np.float64 and ibs0.dtype == np.int32 and len(i) >= 6
    phi_at = np.zeros((15, 15))
    phi_at[i, j] = phi
    (k0w, k1w, k2w), sums = IO.ibd(Gm, P, Q, _f32(inb), phi_at)
    d0, d2 = np.abs(k0 - k0w[i, j]).max(), np.abs(k2 - k2w[i, j]).max()
    print(f"pedigree: max |k0 - k0_64| = {d0:.3e}, max |k2 - k2_64| = {d2:.3e} over {len(i)} listed pairs")
    assert np.array_equal(ibs0, sums[2][i, j])
    assert d0 <= 1e-4 and d2 <= 1e-4 and np.array_equal(k1, 1.0 - k0 - k2)
    at = {(int(a), int(b)): s for s, (a, b) in enumerate(zip(i, j))}
    labels = relate.relation(phi, k0)
    assert [labels[at[p]] for p in KO.PED_PARENT_CHILD + KO.PED_SIBS] == ["parent-offspring"] * 4 + ["full siblings"]
    dup = at[KO.PED_DUPLICATE[0]]
    assert labels[dup] == "duplicate or twin" and k2[dup] > 0.9 and k0[dup] == 0.0


@pytest.mark.gpu
def test_pair_form_in_blocks_skips_the_blocks_without_a_listed_pair(monkeypatch):
    """ibd_pairs with rows = 64 on N = 130 (six blocks), sample 70 a copy of sample 3 and min_phi = 0.3: every nadm_ibd call is for a
    block that holds a listed pair and no other block is computed; each computed block is within the bounds of the float64 oracle, as
    is ONE 130 x 130 block, whose ibs0 at the listed pairs is what ibd_pairs returns; k0, k1, k2 are ibd_of of the computed blocks'
    sums at the listed pairs."""
    from neural_admixture_amd import relate
    dev = _dev()
    M, K, N = 1027, 3, 130
    Gm, P, Q, dead, _, _ = _case(M, K)
    Gm, Q = Gm[:N].copy(), Q[:N].copy()
    Gm[70], Q[70] = Gm[3], Q[3]
    xp = _packed(Gm).to(dev)
    calls = []
    real = relate.ibd_block

    def counted(xp_, M_, Pp, k, idxA, QA, fA, idxB, QB, fB, pimin=0.0, scratch=None):
        out = real(xp_, M_, Pp, k, idxA, QA, fA, idxB, QB, fB, pimin, scratch)
        calls.append((idxA.cpu().numpy(), idxB.cpu().numpy(), tuple(o.clone() for o in out)))
        return out
    monkeypatch.setattr(relate, "ibd_block", counted)
    i, j, phi, n, inb, k0, k1, k2, ibs0 = (x.cpu().numpy() for x in relate.ibd_pairs(xp, M, P, Q, min_phi=0.3, rows=64))
    monkeypatch.undo()
    listed = {(int(a) // 64, int(b) // 64) for a, b in zip(i, j)}
    assert (3, 70) in set(zip(i.tolist(), j.tolist())) and (0, 1) in listed
    assert len(calls) == len(listed) and 1 <= len(calls) < 6
    assert {(int(a[0]) // 64, int(b[0]) // 64) for a, b, _ in calls} == listed
    f = _f32(inb)
    t = IO.terms(Gm, P, Q, f, 0.0)
    sums_at = {}
    for ra, rb, (k2num, k2den, exp0, s0) in calls:
        blk = tuple(x.cpu().numpy() for x in (k2num, k2den, s0, exp0))
        _check_block(blk, IO.from_terms(IO.gather(t, ra), IO.gather(t, rb)), f"block rows {ra[0]}.. x {rb[0]}..")
        for s, (a, b) in enumerate(zip(i, j)):
            if ra[0] <= a < ra[0] + len(ra) and rb[0] <= b < rb[0] + len(rb):
                sums_at[s] = tuple(x[a - ra[0], b - rb[0]] for x in blk)
    assert sorted(sums_at) == list(range(len(i)))
    cols = [np.asarray([sums_at[s][c] for s in range(len(i))]) for c in range(4)]
    assert np.array_equal(ibs0, cols[2])
    w0, w1, w2 = IO.ibd_of(phi, *cols)
    assert np.array_equal(k0, w0, equal_nan=True) and np.array_equal(k1, w1, equal_nan=True) and np.array_equal(k2, w2, equal_nan=True)
    one = _gpu_block(xp, M, P, Q, f, None, None)
    _check_block(one, IO.from_terms(t, t), "one 130 x 130 block")
    assert np.array_equal(ibs0, one[2][i, j])
    s = int(np.nonzero((i == 3) & (j == 70))[0][0])
    assert k2[s] > 0.9 and k0[s] == 0.0


@pytest.mark.gpu
def test_engine_ibd_equals_the_library_free_form_and_leaves_the_parameters():
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
        got = e.ibd(head=head, min_phi=0.0, pimin=0.01)
        want = relate.ibd_pairs(e.xp, M, e.P(head).clone(), Qh, min_phi=0.0, pimin=0.01)
        assert len(got) == 9
        assert all(torch.equal(a, b) or (a.dtype.is_floating_point and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))) for a, b in zip(got, want))
        assert got[0].numel() > 10 and got[4].shape == (N,) and got[5].shape == got[0].shape
        k = (got[0] == 3) & (got[1] == 17)
        assert int(k.sum()) == 1 and float(got[2][k]) > 0.3 and float(got[5][k]) == 0.0 and int(got[8][k]) == 0
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


@pytest.mark.gpu
def test_cli_kinship_ibd_end_to_end(tmp_path, caplog):
    """The `kinship` mode on the bundled demo .bed (its first sample written over the second: a duplicate to find), once without and
    once with --ibd: .kin and .inbreed are the same bytes both ways, .ibd holds what ibd_pairs returns, its first line is the duplicate."""
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
    base = ["kinship", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(tmp_path), "--name", "run", "--k", "3", "--min_phi", "0.1"]
    assert cli.main(base + ["--out_name", "plain"]) == 0
    assert not (tmp_path / "plain.3.ibd").exists()
    assert cli.main(base + ["--out_name", "rel", "--ibd"]) == 0
    for ext in ("kin", "inbreed"):
        assert (tmp_path / f"rel.3.{ext}").read_bytes() == (tmp_path / f"plain.3.{ext}").read_bytes()
    Qr = np.loadtxt(tmp_path / "run.3.Q", dtype=np.float32, ndmin=2)
    Pr = np.loadtxt(tmp_path / "run.3.P", dtype=np.float32, ndmin=2)
    again = read_bed_packed(str(tmp_path / "demo.bed"), dev, keep_on_device=True)
    i, j, phi, n, f, k0, k1, k2, ibs0 = (x.cpu().numpy() for x in relate.ibd_pairs(again.packed, M, Pr, Qr, min_phi=0.1))
    lines = [ln.split() for ln in (tmp_path / "rel.3.ibd").read_text().splitlines()]
    assert len(lines) == len(i) >= 1 and all(len(c) == 9 for c in lines)
    assert [int(c[0]) for c in lines] == i.tolist() and [int(c[1]) for c in lines] == j.tolist()
    assert [int(c[3]) for c in lines] == n.tolist() and [int(c[7]) for c in lines] == ibs0.tolist()
    for col, want in ((2, phi), (4, k0), (5, k1), (6, k2)):
        assert np.array_equal(np.asarray([float(c[col]) for c in lines]), want, equal_nan=True)
    assert [c[8] for c in lines] == [s.replace(" ", "_") for s in relate.relation(phi, k0)]
    assert lines[0][:2] == ["0", "1"] and float(lines[0][6]) > 0.9 and lines[0][8] == "duplicate_or_twin"
    msgs = [r.getMessage() for r in caplog.records]
    assert any("duplicate or twin: " in m for m in msgs) and any("parent-offspring:" in m for m in msgs) and any("full siblings:" in m for m in msgs)
