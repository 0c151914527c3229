"""LD pruning (nadm_snp_counts, nadm_ld_band, nadm_select_snps, nadm_ld_sweep; ld.snp_counts / ld_band / prune / select_snps; the
`prune` mode and `--extract` of the command line).  The int64 / float64 numpy restatement and the data live in tests/ld_oracle.py.

Every comparison with the oracle is an EQUALITY: the moments are sums of products of integers in {0, 1, 2, 4} accumulated in int32
(at most 4 rows), r^2 is two float64 products and one float64 division of exactly representable integers below 2^53 -- the same
IEEE operations on both sides."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_oracle as LO  # noqa: E402
from packed_rows import dev as _dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WMAX = 130
# (rows, M, W): every value of the three at least twice, not their product.  rows 1 / 37 / 131: a sample tail of the k axis, 64: none;
# M 5 / 257 / 1027: a last byte with pad bits; W 64 / 130: a window that crosses SNP tiles and 64-SNP blocks (130: and the second
# group of eight b-tiles), M 1027 with them: 512-SNP boundaries; W >= M at M = 5 and (64, 64, 64)
SHAPES = [(1, 5, 1), (1, 64, 7), (37, 5, 7), (37, 257, 64), (37, 1027, 130), (64, 64, 1), (64, 64, 64), (64, 257, 7),
          (64, 1027, 64), (131, 5, 130), (131, 257, 130), (131, 1027, 7)]


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_on_a_case_worked_out_by_hand():
    """Four samples (rows), three SNPs, 3 = missing:
            SNP0 SNP1 SNP2
        s0    0    1    2
        s1    1    2    0
        s2    2    3    2
        s3    3    0    1
    pair (0, 1): jointly observed s0 (0, 1), s1 (1, 2): n = 2, Sa = 1, Sb = 3, Sab = 2, Saa = 1, Sbb = 5;
                 cov = 2*2 - 1*3 = 1, va = 2*1 - 1 = 1, vb = 2*5 - 9 = 1, r2 = 1
    pair (0, 2): s0 (0, 2), s1 (1, 0), s2 (2, 2): n = 3, Sa = 3, Sb = 4, Sab = 4, Saa = 5, Sbb = 8;
                 cov = 12 - 12 = 0, va = 15 - 9 = 6, vb = 24 - 16 = 8, r2 = 0
    pair (1, 2): s0 (1, 2), s1 (2, 0), s3 (0, 1): n = 3, Sa = 3, Sb = 3, Sab = 2, Saa = 5, Sbb = 5;
                 cov = 6 - 9 = -3, va = 6, vb = 6, r2 = 9 / 36 = 0.25
    counts: SNP0 (3, 3, 5), SNP1 (3, 3, 5), SNP2 (4, 5, 9); maf = 3/6, 3/6, min(5, 3)/8 = 0.5, 0.5, 0.375.
    Sweep at thr 0.2: i = 0 meets j = 1 (r2 1 > 0.2, a tie in maf: j goes), j = 2 (r2 0); i = 1 is gone; kept = 1 0 1.
    With maf = 0.1, 0.5, 0.375: i = 0 is the rarer of (0, 1) and goes; i = 1 meets j = 2 (0.25 > 0.2, j rarer: goes); kept = 0 1 0.
    At thr = 1.0 nothing exceeds the threshold; at thr = 0.25 the pair (1, 2) stays (r2 == thr is kept)."""
    G = np.asarray([[0, 1, 2], [1, 2, 0], [2, 3, 2], [3, 0, 1]], dtype=np.uint8)
    r2, mom = LO.band(G, 2)
    assert mom[0, 0].tolist() == [2, 1, 3, 2, 1, 5] and mom[0, 1].tolist() == [3, 3, 4, 4, 5, 8] and mom[1, 0].tolist() == [3, 3, 3, 2, 5, 5]
    assert not mom[1, 1].any() and not mom[2].any()
    assert r2.tolist() == [[1.0, 0.0], [0.25, 0.0], [0.0, 0.0]]
    cnt = LO.counts(G)
    assert cnt.tolist() == [[3, 3, 5], [3, 3, 5], [4, 5, 9]] and LO.maf(cnt).tolist() == [0.5, 0.5, 0.375]
    one = lambda thr, maf: LO.sweep(r2, 0, 3, 2, 3, np.asarray(maf), None, thr, np.ones(3, dtype=np.uint8)).tolist()  # noqa: E731
    assert one(0.2, [0.5, 0.5, 0.375]) == [1, 0, 1]
    assert one(0.2, [0.1, 0.5, 0.375]) == [0, 1, 0]
    assert one(1.0, [0.5, 0.5, 0.375]) == [1, 1, 1]
    assert one(0.25, [0.1, 0.6, 0.5]) == [0, 1, 1]
    assert LO.prune(G, 3, 0.2).tolist() == [True, False, True]
    assert np.array_equal(LO.unpack(LO.pack(G), 3), G) and LO.pack(G, dirty=True)[0, 0] == 0b11100100 and LO.pack(G).shape == (4, 16)


def test_header_declares_the_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    import neural_admixture_amd as na
    header = open(os.path.join(ROOT, "include", "nadm.h")).read()
    for name in ("nadm_snp_counts", "nadm_ld_band", "nadm_select_snps", "nadm_ld_sweep"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_LD_MAX_WINDOW 1024" in header
    for name in ("snp_counts", "ld_band", "prune", "select_snps"):
        assert callable(getattr(na, name)) and name in na.__all__


def _band_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    idx = torch.zeros(4, dtype=torch.int32)
    r2 = torch.empty((50, 7), dtype=torch.float64)
    mom = torch.empty((50, 7, 6), dtype=torch.int32)
    a = dict(xp=xp.data_ptr(), ld=16, idx=idx.data_ptr(), rows=4, M=50, m0=0, m1=50, W=7, r2=r2.data_ptr(), mom=mom.data_ptr(), stream=None)
    return a, (xp, idx, r2, mom)


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(r2=None), "null pointer"),
    (dict(rows=0), "rows must be in 1..2^24"), (dict(rows=(1 << 24) + 1), "rows must be in 1..2^24"), (dict(M=0), "M must be >= 1"),
    (dict(W=0), "W must be in 1..NADM_LD_MAX_WINDOW"), (dict(W=1025), "W must be in 1..NADM_LD_MAX_WINDOW"),
    (dict(m0=-1), "need 0 <= m0 < m1 <= M"), (dict(m0=20, m1=20), "need 0 <= m0 < m1 <= M"), (dict(m0=30, m1=10), "need 0 <= m0 < m1 <= M"),
    (dict(m1=51), "need 0 <= m0 < m1 <= M"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(unaligned="xp"), "xp must be 16-byte aligned"), (dict(unaligned="idx", by=2), "idx must be 4-byte aligned"),
    (dict(unaligned="r2"), "r2 must be 8-byte and mom 4-byte aligned"), (dict(unaligned="mom", by=2), "r2 must be 8-byte and mom 4-byte aligned"),
])
def test_ld_band_refuses_before_any_launch(change, message):
    """Every refusal is decided on the host: it comes back with its message on a machine without a GPU, where a launch would fail
    with another one."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _band_args()
    if "unaligned" in change:
        a[change["unaligned"]] += change.get("by", 4)
    else:
        a.update(change)
    status = lib.nadm_ld_band(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_ld_band"):
        check(status, "ld_band")
    del keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(cnt=None), "null pointer"), (dict(rows=0), "rows must be in 1..2^24"),
    (dict(rows=(1 << 24) + 1), "rows must be in 1..2^24"), (dict(M=0), "M must be >= 1"), (dict(ld=12), "ld < ceil(M/4)"),
    (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(unaligned="xp"), "xp must be 16-byte aligned"), (dict(unaligned="cnt"), "cnt must be 4-byte aligned"),
])
def test_snp_counts_refuses_before_any_launch(change, message):
    from neural_admixture_amd._lib import lib
    xp, cnt = torch.zeros((4, 16), dtype=torch.uint8), torch.empty((50, 3), dtype=torch.int32)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, rows=4, M=50, cnt=cnt.data_ptr(), stream=None)
    if "unaligned" in change:
        a[change["unaligned"]] += 2
    else:
        a.update(change)
    assert lib.nadm_snp_counts(*a.values()) != 0 and message in lib.nadm_last_error().decode()
    assert "nadm_snp_counts" in lib.nadm_last_error().decode()


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(keep=None), "null pointer"), (dict(out=None), "null pointer"),
    (dict(rows=0), "empty selection"), (dict(M_out=0), "empty selection"), (dict(ld_in=0), "ld_in and ld_out must be in 1..2^32-1"),
    (dict(ld_out=1 << 32), "ld_in and ld_out must be in 1..2^32-1"), (dict(ld_out=2), "ld_out < ceil(M_out/4)"),
    (dict(unaligned="keep"), "keep must be 8-byte aligned"),
])
def test_select_snps_refuses_before_any_launch(change, message):
    from neural_admixture_amd._lib import lib
    xp, out, keep = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros((4, 16), dtype=torch.uint8), torch.arange(9, dtype=torch.int64)
    a = dict(xp=xp.data_ptr(), ld_in=16, rows=4, keep=keep.data_ptr(), M_out=9, flip=0, out=out.data_ptr(), ld_out=16, stream=None)
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    else:
        a.update(change)
    assert lib.nadm_select_snps(*a.values()) != 0 and message in lib.nadm_last_error().decode()
    assert "nadm_select_snps" in lib.nadm_last_error().decode()


def test_ld_sweep_refusals():
    from neural_admixture_amd._lib import lib
    r2, maf, kept = np.zeros((5, 3)), np.zeros(5), np.ones(5, dtype=np.uint8)
    ok = dict(r2=r2.ctypes.data, m0=0, m1=5, W=3, M=5, maf=maf.ctypes.data, chrom=None, thr=0.1, kept=kept.ctypes.data)
    assert lib.nadm_ld_sweep(*ok.values()) == 0
    for change, message in ((dict(r2=None), "null pointer"), (dict(maf=None), "null pointer"), (dict(kept=None), "null pointer"),
                            (dict(W=0), "W must be in 1..NADM_LD_MAX_WINDOW"), (dict(W=1025), "W must be in 1..NADM_LD_MAX_WINDOW"),
                            (dict(m0=3, m1=3), "need 0 <= m0 < m1 <= M"), (dict(m1=6), "need 0 <= m0 < m1 <= M"), (dict(m0=-1), "need 0 <= m0 < m1 <= M"),
                            (dict(thr=float("nan")), "thr must be a number")):
        a = dict(ok)
        a.update(change)
        assert lib.nadm_ld_sweep(*a.values()) != 0 and message in lib.nadm_last_error().decode()


@pytest.mark.parametrize("M, W, seed", [(300, 7, 0), (300, 49, 1), (41, 64, 2), (5, 130, 3), (1000, 20, 4)])
def test_sweep_against_the_oracle(M, W, seed):
    """Random bands on a grid of r2 values (so that r2 == thr occurs: such a pair is kept) and of maf values (ties), with and without
    chromosome breaks, W larger than M among the cases; the range-by-range calls equal the one call."""
    from neural_admixture_amd import ld
    rng = np.random.default_rng(seed)
    r2 = rng.integers(0, 11, size=(M, W)).astype(np.float64) / 10.0
    r2[rng.random((M, W)) < 0.6] = 0.0
    maf = rng.integers(0, 6, size=M).astype(np.float64) / 10.0
    chrom = np.sort(rng.integers(0, 4, size=M)).astype(np.int32)
    for thr in (0.3, 0.0, 1.0):
        assert (r2 == thr).any()
        for ch in (None, chrom):
            want = LO.sweep(r2, 0, M, W, M, maf, ch, thr, np.ones(M, dtype=np.uint8))
            got = np.ones(M, dtype=np.uint8)
            ld.sweep(r2, 0, M, M, maf, ch, thr, got)
            assert np.array_equal(got, want)
            parts = np.ones(M, dtype=np.uint8)
            step = max(1, M // 7 + 1)
            for m0 in range(0, M, step):
                m1 = min(M, m0 + step)
                ld.sweep(np.ascontiguousarray(r2[m0:m1]), m0, m1, M, maf, ch, thr, parts)
            assert np.array_equal(parts, want)
            if thr == 0.3:
                assert 0 < want.sum() < M or M <= 5
    one = np.full((2, 1), 0.3)                               # r2 == thr is kept; one ulp above it is not
    k = np.ones(2, dtype=np.uint8)
    ld.sweep(one, 0, 2, 2, np.asarray([0.2, 0.1]), None, 0.3, k)
    assert k.tolist() == [1, 1]
    ld.sweep(np.nextafter(one, 1.0), 0, 2, 2, np.asarray([0.2, 0.1]), None, 0.3, k)
    assert k.tolist() == [1, 0]


def test_id_lists_and_bim(tmp_path):
    from neural_admixture_amd import ld
    (tmp_path / "a.bim").write_text("1\trs1\t0\t10\tA\tG\n1 rs2 0 20 A G\nX\trs3\t0\t5\tC\tT\nX\trs2\t0\t9\tC\tT\n")
    ids, chroms = ld.read_bim(tmp_path / "a.bim")
    assert ids == ["rs1", "rs2", "rs3", "rs2"] and chroms == ["1", "1", "X", "X"]
    assert ld.chrom_codes(chroms).tolist() == [0, 0, 1, 1] and ld.chrom_codes(chroms).dtype == np.int32
    (tmp_path / "l.txt").write_text("rs3\n\n  rs1  extra\n")
    assert ld.read_id_list(tmp_path / "l.txt") == ["rs3", "rs1"]
    assert ld.resolve_ids(ids, ["rs3", "rs1"]).tolist() == [True, False, True, False]
    with pytest.raises(SystemExit, match="SNP ID rs9 of the list is not in the .bim"):
        ld.resolve_ids(ids, ["rs1", "rs9"])
    with pytest.raises(SystemExit, match="SNP ID rs2 of the list occurs more than once in the .bim"):
        ld.resolve_ids(ids, ["rs2"])
    with pytest.raises(SystemExit, match="lists no SNP"):
        ld.resolve_ids(ids, [])
    ld.write_id_list(tmp_path / "w.in", ["rs1", "rs3"])
    assert (tmp_path / "w.in").read_text() == "rs1\nrs3\n" and ld.read_id_list(tmp_path / "w.in") == ["rs1", "rs3"]
    (tmp_path / "bad.bim").write_text("1\trs1\t0\t10\tA\tG\nlonely\n")
    with pytest.raises(SystemExit, match="line 2 has fewer than two columns"):
        ld.read_bim(tmp_path / "bad.bim")
    assert ld.maf_from_counts(np.asarray([[3, 3, 5], [4, 5, 9], [0, 0, 0]])).tolist() == [0.5, 0.375, 0.0]


def test_python_argument_checks_name_the_argument():
    from neural_admixture_amd import ld
    from neural_admixture_amd.io import PackedGenotypes
    host = torch.zeros((4, 16), dtype=torch.uint8)
    for fn in (lambda: ld.snp_counts(host, 50), lambda: ld.ld_band(host, 50, 5), lambda: ld.prune(host, 50)):
        with pytest.raises(RuntimeError, match="packed matrix must be on a ROCm GPU"):
            fn()
    with pytest.raises(RuntimeError, match="keep must be a bool vector with one entry per SNP"):
        ld.select_snps(PackedGenotypes(host, 4, 50), np.ones(49, dtype=bool))
    with pytest.raises(RuntimeError, match="keep must be a bool vector"):
        ld.select_snps(PackedGenotypes(host, 4, 50), np.ones(50, dtype=np.uint8))
    with pytest.raises(RuntimeError, match="keep selects no SNP"):
        ld.select_snps(PackedGenotypes(host, 4, 50), np.zeros(50, dtype=bool))
    with pytest.raises(RuntimeError, match="data must be a PackedGenotypes"):
        ld.select_snps(host, np.ones(50, dtype=bool))
    with pytest.raises(RuntimeError, match="r2 must be a contiguous float64 array"):
        ld.sweep(np.zeros((5, 3), dtype=np.float32), 0, 5, 5, np.zeros(5), None, 0.1, np.ones(5, dtype=np.uint8))
    with pytest.raises(RuntimeError, match="chrom must be a contiguous int32 array"):
        ld.sweep(np.zeros((5, 3)), 0, 5, 5, np.zeros(5), np.zeros(5, dtype=np.int64), 0.1, np.ones(5, dtype=np.uint8))


def test_cli_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """`prune` and `--extract`: argument errors, VCF input, a missing .bim, a .bim that does not match the .bed, an unknown and a
    duplicated SNP ID end the run with the offender named before a genotype is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["prune", "--name", "run", "--save_dir", str(tmp_path / "out"), "--data_path", str(bed)]
    a = cli.parse_prune_args(base[1:])
    assert (a.window, a.r2, a.threads) == (50, 0.1, 1)

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(SystemExit, match=r"--window must be in 2\.\.1025"):
        cli.main(base + ["--window", "1"])
    with pytest.raises(SystemExit, match=r"--window must be in 2\.\.1025"):
        cli.main(base + ["--window", "1026"])
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match=r"--r2 must be in \[0, 1\]"):
            cli.main(base + ["--r2", bad])
    with pytest.raises(SystemExit, match=r"prune needs the SNP IDs and chromosomes of a \.bim file: it is not available for VCF input"):
        cli.main(base[:-1] + [str(tmp_path / "x.vcf")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen")])
    with pytest.raises(SystemExit, match=r"x\.bim not found"):
        cli.main(base)
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j}\tA\tG\n" for j in range(9)))
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
    assert not (tmp_path / "out").exists()
    # --extract on train, infer and kinship
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j}\tA\tG\n" for j in range(9)) + "1\trs3\t0\t99\tA\tG\n")
    (tmp_path / "unknown.txt").write_text("rs1\nrs77\n")
    (tmp_path / "twice.txt").write_text("rs1\nrs3\n")
    train = ["train", "--k", "3", "--name", "run", "--save_dir", str(tmp_path / "out"), "--data_path", str(bed)]
    with pytest.raises(SystemExit, match=r"SNP ID rs77 of .*unknown\.txt is not in .*x\.bim"):
        cli.main(train + ["--extract", str(tmp_path / "unknown.txt")])
    with pytest.raises(SystemExit, match=r"SNP ID rs3 of .*twice\.txt occurs more than once in .*x\.bim"):
        cli.main(train + ["--extract", str(tmp_path / "twice.txt")])
    with pytest.raises(SystemExit, match=r"absent\.txt not found"):
        cli.main(train + ["--extract", str(tmp_path / "absent.txt")])
    with pytest.raises(SystemExit, match=r"--extract resolves SNP IDs through a \.bim file: it is not available for VCF input"):
        cli.main(train[:-1] + [str(tmp_path / "x.vcf"), "--extract", str(tmp_path / "unknown.txt")])
    infer = ["infer", "--out_name", "o", "--name", "run", "--save_dir", str(tmp_path / "out"), "--data_path", str(bed)]
    with pytest.raises(SystemExit, match=r"SNP ID rs77 of .*unknown\.txt is not in"):
        cli.main(infer + ["--extract", str(tmp_path / "unknown.txt")])
    np.savetxt(tmp_path / "run.3.P", np.full((2, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    kin = ["kinship", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    with pytest.raises(SystemExit, match=r"SNP ID rs77 of .*unknown\.txt is not in"):
        cli.main(kin + ["--extract", str(tmp_path / "unknown.txt")])
    (tmp_path / "three.txt").write_text("rs1\nrs5\nrs8\n")     # kinship's row-count check uses the number of listed SNPs
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 2 x 3 matrix, the model needs 3 x 3"):
        cli.main(kin + ["--extract", str(tmp_path / "three.txt")])
    with pytest.raises(AssertionError, match='Please provide either the argument "train" or "infer"'):
        cli.main(["thin"])


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(rows, M, gather):
    """(resident genotypes, idx or None, the genotypes of the listed rows, the oracle's band at W = WMAX, its counts).  gather: 30 %
    missing, rows + 9 resident rows of which a shuffled `rows` are listed; else 5 % missing and every row.  Left unchanged."""
    seed = 1000 * rows + M
    if gather:
        res = LO.random_genotypes(rows + 9, M, seed, missing=0.3)
        idx = np.random.default_rng(seed + 1).permutation(rows + 9)[:rows].astype(np.int32)
        G = res[idx]
    else:
        res = LO.random_genotypes(rows, M, seed + 2, missing=0.05)
        idx, G = None, res
    r2, mom = LO.band(G, WMAX)
    return res, idx, G, r2, mom, LO.counts(G)


def _gpu_band(res, idx, M, W, m0=0, m1=None, **pack):
    from neural_admixture_amd import ld
    dev = _dev()
    xp = torch.from_numpy(LO.pack(res, **pack)).to(dev)
    it = None if idx is None else torch.from_numpy(idx).to(dev)
    r2, mom = ld.ld_band(xp, M, W + 1, m0, m1, it, with_moments=True)
    torch.cuda.synchronize()
    return r2.cpu().numpy(), mom.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("gather", [True, False], ids=["gather", "all_rows"])
@pytest.mark.parametrize("rows, M, W", SHAPES)
def test_band_bit_for_bit(rows, M, W, gather):
    res, idx, G, r2w, momw, _ = _case(rows, M, gather)
    r2, mom = _gpu_band(res, idx, M, W)
    assert r2.shape == (M, W) and mom.shape == (M, W, 6) and r2.dtype == np.float64 and mom.dtype == np.int32
    bad = np.argwhere(mom != momw[:, :W])
    assert bad.size == 0, f"{len(bad)} moments differ, the first at (j, d, moment) = {bad[0].tolist()}: {mom[tuple(bad[0])]} != {momw[:, :W][tuple(bad[0])]}"
    assert r2.tobytes() == r2w[:, :W].tobytes()
    if M > W + 1 and rows > 4:
        assert (r2 > 0).any() and (momw[:, :W, 1] != momw[:, :W, 2]).any()


@pytest.mark.gpu
def test_sub_range_is_the_slice_of_the_full_band():
    rows, M, W = 131, 1027, 64
    res, idx, G, r2w, momw, _ = _case(rows, M, True)
    full = _gpu_band(res, idx, M, W)
    for m0, m1 in ((70, 900), (1, 2), (512, 1027), (63, 65)):
        r2, mom = _gpu_band(res, idx, M, W, m0, m1)
        assert r2.shape == (m1 - m0, W)
        assert r2.tobytes() == full[0][m0:m1].tobytes() == r2w[m0:m1, :W].tobytes()
        assert np.array_equal(mom, full[1][m0:m1]) and np.array_equal(mom, momw[m0:m1, :W])


@pytest.mark.gpu
def test_exactly_zero_cases_and_bits_that_hold_no_call():
    """A monomorphic SNP (1), a SNP missing in every row (3), a pair with no jointly observed row (40, 42): r2 exactly 0.0.  A packed
    buffer whose pad bits, padding bytes and rows beyond `rows` are all ones gives the same bits as the clean one."""
    from neural_admixture_amd._lib import lib, check, ptr
    rows, M, W = 37, 257, 64
    res, idx, G, r2w, momw, _ = _case(rows, M, False)
    r2, mom = _gpu_band(res, None, M, W)
    assert (G[:, 1][G[:, 1] != 3] == 1).all() and (G[:, 3] == 3).all() and not ((G[:, 40] != 3) & (G[:, 42] != 3)).any()
    zero = np.zeros(1).tobytes()
    assert r2[1].tobytes() == zero * W and r2[0, 0].tobytes() == zero and mom[1, :, 0].any()          # monomorphic: counted, r2 0
    assert r2[3].tobytes() == zero * W and not mom[3].any() and not mom[2, 0].any() and not mom[0, 2].any()
    assert r2[40, 1].tobytes() == zero and not mom[40, 1].any()
    assert r2[M - 1].tobytes() == zero * W and not mom[M - 1].any() and not mom[M - 3, 2:].any()   # b >= M
    dev = _dev()
    dirty = torch.from_numpy(LO.pack(res, dirty=True, extra_rows=70)).to(dev)
    assert dirty.shape[0] == rows + 70 and int(dirty[rows:].min()) == 0xFF
    r2d = torch.empty((M, W), dtype=torch.float64, device=dev)
    momd = torch.empty((M, W, 6), dtype=torch.int32, device=dev)
    check(lib.nadm_ld_band(ptr(dirty), dirty.shape[1], None, rows, M, 0, M, W, ptr(r2d), ptr(momd), None), "ld_band")
    cnt = torch.empty((M, 3), dtype=torch.int32, device=dev)
    check(lib.nadm_snp_counts(ptr(dirty), dirty.shape[1], None, rows, M, ptr(cnt), None), "snp_counts")
    torch.cuda.synchronize()
    assert r2d.cpu().numpy().tobytes() == r2.tobytes() and np.array_equal(momd.cpu().numpy(), mom)
    assert np.array_equal(cnt.cpu().numpy(), LO.counts(G))


@pytest.mark.gpu
def test_orientation_of_the_pair():
    """SNP a = 0 and SNP b = 2 with different missingness and different values: Sa != Sb and Saa != Sbb, n < rows.  A swapped A / B
    operand or a row / column mix-up in the write of the result cannot pass; neither can a transposed (j, d) index."""
    rows, M = 37, 64
    G = LO.random_genotypes(rows, M, 5, missing=0.0)
    G[:, 0] = np.where(np.arange(rows) < 10, 2, np.arange(rows) % 3)
    G[::5, 0] = 3
    G[:, 2] = np.where(np.arange(rows) % 7 < 2, 2, np.arange(rows) % 2)
    G[1::4, 2] = 3
    r2w, momw = LO.band(G, 7)
    n, Sa, Sb, Sab, Saa, Sbb = momw[0, 1]
    assert Sa != Sb and Saa != Sbb and n < rows and len({int(n), int(Sa), int(Sb), int(Sab), int(Saa), int(Sbb)}) == 6
    assert not np.array_equal(momw[0, 1], momw[1, 0]) and not np.array_equal(momw[0, 1], momw[2, 1])
    r2, mom = _gpu_band(G, None, M, 7)
    assert mom[0, 1].tolist() == momw[0, 1].tolist()
    assert np.array_equal(mom, momw) and r2.tobytes() == r2w.tobytes()


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    res, idx, G, r2w, momw, _ = _case(131, 1027, True)
    a = _gpu_band(res, idx, 1027, 130)
    b = _gpu_band(res, idx, 1027, 130)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("rows, M, gather", [(1, 5, False), (37, 257, True), (131, 1027, True), (64, 64, False), (300, 4100, False)])
def test_snp_counts_against_numpy(rows, M, gather):
    from neural_admixture_amd import ld
    dev = _dev()
    res, idx, G, _, _, cntw = _case(rows, M, gather) if M <= 1027 else (LO.random_genotypes(rows, M, 9), None, None, None, None, None)
    if cntw is None:
        cntw = LO.counts(res)
    xp = torch.from_numpy(LO.pack(res, dirty=True)).to(dev)
    cnt = ld.snp_counts(xp, M, None if idx is None else torch.from_numpy(idx).to(dev))
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (M, 3)
    assert np.array_equal(cnt.cpu().numpy(), cntw)
    assert np.array_equal(ld.maf_from_counts(cnt), LO.maf(cntw))


def _two_frequency_file(low_first):
    """Raw file codes [50, 203]: 120 SNPs around frequency 0.1 and 83 around 0.9 (the file as a whole is not flipped), or 83 and 120
    (it is), 4 % missing."""
    rng = np.random.default_rng(11 + low_first)
    n_low = 120 if low_first else 83
    f = np.concatenate([np.full(n_low, 0.1), np.full(203 - n_low, 0.9)])
    G = rng.binomial(2, f, size=(50, 203)).astype(np.uint8)
    G[rng.random(G.shape) < 0.04] = 3
    return G, n_low


@pytest.mark.gpu
@pytest.mark.parametrize("low_first", [1, 0], ids=["file_as_is", "file_flipped"])
@pytest.mark.parametrize("subset", ["low", "high", "mixed"])
def test_select_snps_equals_the_reader_on_a_file_of_the_kept_snps(tmp_path, low_first, subset):
    """select_snps(read(full file), keep) is byte for byte read(a file that holds only the kept SNPs): packed bytes, stride, M and
    `flipped`.  The low-frequency subset is not flipped by the reader's rule, the high-frequency one is; M_out % 4 != 0."""
    from neural_admixture_amd import ld
    from neural_admixture_amd.io import read_bed_packed
    from neural_admixture_amd.layout import ModelLayout
    dev = _dev()
    G, n_low = _two_frequency_file(low_first)
    rng = np.random.default_rng(3)
    keep = np.zeros(203, dtype=bool)
    if subset == "low":
        keep[rng.choice(n_low, size=41, replace=False)] = True
    elif subset == "high":
        keep[n_low + rng.choice(203 - n_low, size=37, replace=False)] = True
    else:
        keep[rng.choice(203, size=101, replace=False)] = True
    assert keep.sum() % 4 != 0
    LO.write_bed(tmp_path / "full", G)
    LO.write_bed(tmp_path / "sub", G[:, keep])
    full = read_bed_packed(str(tmp_path / "full.bed"), dev, keep_on_device=True)
    want = read_bed_packed(str(tmp_path / "sub.bed"), dev, keep_on_device=True)
    assert full.flipped == (not low_first)
    if subset != "mixed":
        assert want.flipped == (subset == "high")
    got = ld.select_snps(full, keep)
    assert (got.N, got.M, got.flipped) == (want.N, want.M, want.flipped) and got.M == int(keep.sum())
    assert got.packed.device == full.packed.device and got.packed.shape == want.packed.shape == (50, ModelLayout.row_stride(got.M))
    assert torch.equal(got.packed, want.packed)
    raw = G[:, keep]
    assert np.array_equal(LO.unpack(got.packed.cpu().numpy(), got.M), np.where(raw == 3, 3, 2 - raw) if got.flipped else raw)
    host = ld.select_snps(read_bed_packed(str(tmp_path / "full.bed")), keep)         # a host-resident input comes back on the host
    assert host.packed.device.type == "cpu" and torch.equal(host.packed, want.packed.cpu()) and host.flipped == want.flipped


@functools.lru_cache(maxsize=None)
def _panel():
    G = LO.make_panel()
    chrom = np.where(np.arange(G.shape[1]) < 1400, 0, 1).astype(np.int32)
    return G, chrom, LO.prune(G, 50, 0.1, chrom)


@pytest.mark.gpu
def test_prune_equals_the_oracle():
    from neural_admixture_amd import ld
    dev = _dev()
    G, chrom, want = _panel()
    M = G.shape[1]
    assert 0.3 * M < want.sum() < 0.9 * M
    xp = torch.from_numpy(LO.pack(G, ld_round=128)).to(dev)
    keep, stats = ld.prune(xp, M, 50, 0.1, chrom=chrom, range_snps=700)
    assert keep.dtype == np.bool_ and keep.shape == (M,) and stats["ranges"] == 5 and stats["kept"] == int(want.sum())
    assert stats["removed"] == M - stats["kept"] and stats["rows"] == 200
    assert np.array_equal(keep, want)
    one, _ = ld.prune(xp, M, 50, 0.1, chrom=chrom)            # one range
    assert np.array_equal(one, want)
    idx = torch.arange(199, -1, -1, dtype=torch.int32, device=dev)
    rev, _ = ld.prune(xp, M, 50, 0.1, chrom=chrom, idx=idx, range_snps=1000)      # integer sums: the order of the rows does not matter
    assert np.array_equal(rev, want)
    assert not np.array_equal(ld.prune(xp, M, 50, 0.1)[0], want) or (chrom == chrom[0]).all()         # (the chromosome break counts)


@pytest.mark.gpu
def test_cli_prune_then_train_with_extract(tmp_path, caplog):
    from neural_admixture_amd import cli, ld
    _dev()
    G, chrom, want = _panel()
    M = G.shape[1]
    ids = [f"snp_{j}" for j in range(M)]
    LO.write_bed(tmp_path / "panel", G, ids, [str(1 + c) for c in chrom])
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    assert cli.main(["prune", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(out), "--name", "thin"]) == 0
    kept, gone = ld.read_id_list(out / "thin.prune.in"), ld.read_id_list(out / "thin.prune.out")
    assert kept == [s for s, k in zip(ids, want) if k] and gone == [s for s, k in zip(ids, want) if not k]
    assert sorted(kept + gone, key=lambda s: int(s[4:])) == ids and 0 < len(kept) < M
    msgs = [r.getMessage() for r in caplog.records]
    assert any(f"{len(kept)} SNPs kept, {len(gone)} removed" in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    assert cli.main(["train", "--epochs", "2", "--k", "3", "--name", "run", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--extract", str(out / "thin.prune.in")]) == 0
    P, Q = np.loadtxt(out / "run.3.P", ndmin=2), np.loadtxt(out / "run.3.Q", ndmin=2)
    assert P.shape == (len(kept), 3) and Q.shape == (200, 3)
    assert any(f"Using the {len(kept)} SNPs of --extract" in r.getMessage() for r in caplog.records)
