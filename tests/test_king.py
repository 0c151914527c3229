"""KING-robust kinship before the fit (nadm_king, king.king_block / king / king_pairs / unrelated_set / select_samples, Engine.king,
the `king` mode and --keep / --remove of the command line).  The int64 / float64 numpy restatement and the shared data live in
tests/king_oracle.py.  The counts are integers and are compared with ==; phi is ONE float64 division from them, compared as
king.phi_from_counts of the oracle's counts to 1e-15 (it is the same expression on the same integers)."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import king_oracle as KO  # noqa: E402
import ld_oracle as LO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

ROWS = 150                   # resident rows of the GPU cases
SHAPES = [(1, 1), (16, 17), (70, 37), (130, 64)]
MS = [1, 3, 63, 64, 65, 257, 1027]


# ------------------------------------------------------------------------------------------------ CPU
def test_header_declares_the_three_symbols_and_the_library_exports_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_king", "nadm_king_ranges", "nadm_king_scratch_ints"):
        assert name + "(" in header and name in EXPORTS and hasattr(lib, name)
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "#define NADM_KING_MAX_ROWS 4096" in header


def test_shape_queries_refuse_and_the_scratch_covers_every_block():
    from neural_admixture_amd._lib import lib
    rg, f = lib.nadm_king_ranges, lib.nadm_king_scratch_ints
    for bad in ((0, 4, 100), (4, 0, 100), (4097, 4, 100), (4, 4097, 100), (4, 4, 0), (4, 4, 1 << 31), (4, 4, 1 << 40), (-1, 4, 100)):
        assert int(f(*bad)) <= 0 and int(rg(*bad)) <= 0
    assert int(rg(4096, 4096, (1 << 31) - 1)) >= 1 and int(f(1, 1, (1 << 31) - 1)) > 0
    assert int(rg(16, 17, 64)) == 1 and int(rg(37, 70, 70001)) > 1
    for M in (1, 255, 256, 257, 1027, 3001, 70001, 600000):
        chunks = (M + 255) // 256
        for ba in (1, 16, 64, 65, 130, 1024, 4096):
            for bb in (1, 17, 64, 70, 1024, 4096):
                r = int(rg(ba, bb, M))
                tiles = ((ba + 63) // 64) * ((bb + 63) // 64)
                assert 1 <= r <= chunks and int(f(ba, bb, M)) >= r * tiles * 5 * 64 * 64


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(counts=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(ba=0), "empty block"), (dict(bb=-3), "empty block"), (dict(M=0), "empty block"),
    (dict(ba=4097), "must be <= NADM_KING_MAX_ROWS"), (dict(bb=100000), "must be <= NADM_KING_MAX_ROWS"),
    (dict(M=1 << 31, ld=1 << 30), "M must be < 2^31"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(unaligned="xp"), "must be 16-byte aligned"), (dict(unaligned="scratch"), "must be 16-byte aligned"), (dict(unaligned="counts", by=2), "4-byte"),
])
def test_king_refuses_before_any_launch(change, message):
    """Every refusal of nadm_king is decided on the host: it is reported with its message on a machine without a GPU."""
    from neural_admixture_amd._lib import lib, check
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    counts, scratch = torch.empty((5, 4, 4), dtype=torch.int32), torch.empty(5 * 4096 + 4, dtype=torch.int32)
    a = dict(xp=xp.data_ptr(), ld=16, idxA=None, ba=4, idxB=None, bb=4, M=50, counts=counts.data_ptr(), scratch=scratch.data_ptr(), stream=None)
    if "unaligned" in change:
        a[change["unaligned"]] += change.get("by", 4)
    else:
        a.update(change)
    status = lib.nadm_king(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_king"):
        check(status, "king")


def test_oracle_agrees_with_the_double_loop():
    from neural_admixture_amd import king
    G = KO.random_genotypes(9, 37, seed=5, missing=0.2)
    GA, GB = G[:7], G
    c, phi = KO.brute(GA, GB)
    assert np.array_equal(KO.counts(GA, GB), c)
    got = king.phi_from_counts(c)
    assert got.dtype == np.float64 and np.array_equal(got, phi, equal_nan=True)
    assert np.isnan(phi[3]).all() and np.isnan(phi[2]).all() and phi[0, 1] == 0.5 and phi[0, 0] == 0.5 and phi[0, 4] < 0
    # the same expression on a torch tensor gives the same bits
    assert np.array_equal(king.phi_from_counts(torch.from_numpy(c)).numpy(), phi, equal_nan=True)
    assert np.array_equal(KO.counts(KO.flip(GA), KO.flip(GB)), c)


def _check_set(N, i, j, keep):
    adj = [set() for _ in range(N)]
    for a, b in zip(i, j):
        adj[a].add(b)
        adj[b].add(a)
    for v in range(N):
        if keep[v]:
            assert not any(keep[u] for u in adj[v]), v           # independent
        else:
            assert any(keep[u] for u in adj[v]), v               # maximal: every removed sample is related to a kept one


def test_unrelated_set():
    from neural_admixture_amd.king import unrelated_set
    assert unrelated_set(5, [0, 1, 2, 3], [1, 2, 3, 4]).tolist() == [True, False, True, False, True]          # the path keeps {0, 2, 4}
    # a triangle 0-1-2 with the pendant 3 on 2: 2 has three partners and goes; then 0 and 1 tie at one, the higher index goes; the
    # second pass finds 1 related to 0 and 2 related to 0: neither comes back
    assert unrelated_set(4, [0, 0, 1, 2], [1, 2, 2, 3]).tolist() == [True, False, False, True]
    # the second pass: star centre 0 with leaves 1, 2 and the edge 1-2 ... 0 goes (3 partners: 1, 2, 3), then 2 (tie of 1 and 2 at one);
    # 0 stays out (related to 1), 2 stays out
    assert unrelated_set(4, [0, 0, 0, 1], [1, 2, 3, 2]).tolist() == [False, True, False, True]
    assert unrelated_set(6, [], []).tolist() == [True] * 6
    assert unrelated_set(3, torch.tensor([0]), torch.tensor([2])).tolist() == [True, True, False]
    with pytest.raises(RuntimeError, match="unrelated_set"):
        unrelated_set(3, [0], [3])
    rng = np.random.default_rng(0)
    for _ in range(200):
        N = int(rng.integers(1, 40))
        m = int(rng.integers(0, 3 * N))
        i, j = rng.integers(0, N, size=m), rng.integers(0, N, size=m)
        i, j = i[i != j], j[i != j]
        keep = unrelated_set(N, i, j)
        assert keep.dtype == np.bool_ and keep.shape == (N,)
        _check_set(N, i.tolist(), j.tolist(), keep)
        assert np.array_equal(keep, unrelated_set(N, j, i))      # deterministic, and a rule of the graph


def test_fam_reader_and_sample_lists(tmp_path):
    from neural_admixture_amd import io
    fam = tmp_path / "x.fam"
    fam.write_text("f0 s0 0 0 0 -9\nf1\ts1\t0\t0\t0\t-9\nlonely\nf1 s0 0 0\n")
    ids = io.read_fam(fam)
    assert ids == [("f0", "s0"), ("f1", "s1"), ("", "lonely"), ("f1", "s0")]
    io.check_unique_samples(ids, "x.fam")
    lst = tmp_path / "keep.txt"
    lst.write_text("f1 s1\n\nlonely\nf0 s0 extra columns\n")
    want = io.read_sample_list(lst)
    assert want == [("f1", "s1"), (None, "lonely"), ("f0", "s0")]
    assert io.resolve_samples(ids, want, "x.fam", "keep.txt").tolist() == [True, True, True, False]
    assert io.resolve_samples(ids, [(None, "s1")]).tolist() == [False, True, False, False]
    with pytest.raises(SystemExit, match=r"Sample f9 s0 of keep\.txt is not in x\.fam"):
        io.resolve_samples(ids, [("f9", "s0")], "x.fam", "keep.txt")
    with pytest.raises(SystemExit, match=r"Sample nobody of keep\.txt is not in x\.fam"):
        io.resolve_samples(ids, [(None, "nobody")], "x.fam", "keep.txt")
    with pytest.raises(SystemExit, match=r"Sample s0 of keep\.txt is in more than one family"):
        io.resolve_samples(ids, [(None, "s0")], "x.fam", "keep.txt")
    with pytest.raises(SystemExit, match=r"Sample f1 s1 occurs more than once in x\.fam"):
        io.resolve_samples(ids + [("f9", "z"), ("f1", "s1"), ("f9", "z")], want, "x.fam", "keep.txt")
    (tmp_path / "gap.fam").write_text("f0 s0\n\nf1 s1\n")
    with pytest.raises(SystemExit, match=r"gap\.fam: line 2 names no sample"):
        io.read_fam(tmp_path / "gap.fam")
    io.write_sample_list(tmp_path / "out.txt", ids[:3])
    assert (tmp_path / "out.txt").read_text() == "f0 s0\nf1 s1\nlonely\n"
    assert io.read_sample_list(tmp_path / "out.txt") == [("f0", "s0"), ("f1", "s1"), (None, "lonely")]


def test_cli_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors, missing files, unknown and non-unique names end the run with the offender named, before the genotypes are
    read: the reader is a stand-in that fails the test when called."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "absent.bed"
    base = ["king", "--name", "rel", "--save_dir", str(tmp_path / "out"), "--data_path", str(bed)]
    a = cli.parse_king_args(base[1:])
    assert a.cutoff == 2.0 ** -3.5 and a.rows == 1024 and a.keep is None and a.remove is None and a.extract is None and a.threads == 1
    a = cli.parse_king_args(base[1:] + ["--cutoff", "0.2", "--rows", "64", "--remove", "r.txt", "--extract", "e.txt"])
    assert (a.cutoff, a.rows, a.remove, a.extract) == (0.2, 64, "r.txt", "e.txt")
    for parse, extra in ((cli.parse_train_args, []), (cli.parse_infer_args, ["--out_name", "o"]), (cli.parse_pca_args, []),
                         (cli.parse_prune_args, []), (cli.parse_kinship_args, ["--k", "3"]), (cli.parse_cv_args, ["--k", "3"])):
        a = parse(base[1:] + extra + ["--keep", "k.txt"])
        assert a.keep == "k.txt" and a.remove is None

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    both = ["--keep", str(tmp_path / "k.txt"), "--remove", str(tmp_path / "r.txt")]
    for mode in (base, ["train", "--k", "3"] + base[1:], ["pca"] + base[1:]):
        with pytest.raises(SystemExit):                          # (argparse: not allowed with argument)
            cli.main(mode + both)
    with pytest.raises(SystemExit, match=r"--rows must be in 1..4096"):
        cli.main(base + ["--rows", "4097"])
    with pytest.raises(SystemExit, match=r"--cutoff must be a number"):
        cli.main(base + ["--cutoff", "nan"])
    with pytest.raises(SystemExit, match=r"not available for VCF input"):
        cli.main(base[:-1] + [str(tmp_path / "absent.vcf")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "absent.pgen")])
    for mode in (["train", "--k", "3"], ["pca"], ["infer", "--out_name", "o"]):
        with pytest.raises(SystemExit, match=r"--keep resolves sample IDs through a \.fam file: it is not available for VCF input"):
            cli.main(mode + base[1:-1] + [str(tmp_path / "absent.vcf"), "--keep", str(tmp_path / "k.txt")])
    with pytest.raises(SystemExit, match=r"absent\.fam not found"):
        cli.main(base)
    (tmp_path / "absent.fam").write_text("".join(f"f{i} s{i} 0 0 0 -9\n" for i in range(5)))
    with pytest.raises(SystemExit, match=r"absent\.bed not found"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10 + 1))                   # 5 samples = 2 bytes per SNP: 10 SNPs and a byte too many
    with pytest.raises(SystemExit, match=r"absent\.bed does not hold whole SNPs of the 5 samples"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 10))
    with pytest.raises(SystemExit, match=r"k\.txt not found"):
        cli.main(base + ["--keep", str(tmp_path / "k.txt")])
    with pytest.raises(SystemExit, match=r"e\.txt not found"):
        cli.main(base + ["--extract", str(tmp_path / "e.txt")])
    (tmp_path / "k.txt").write_text("f1 s1\ns3\nf7 s7\n")
    (tmp_path / "absent.bim").write_text("".join(f"1\trs{j}\t0\t{j}\tA\tG\n" for j in range(10)))
    for mode in (base, ["pca"] + base[1:], ["prune"] + base[1:], ["train", "--k", "3"] + base[1:]):
        with pytest.raises(SystemExit, match=r"Sample f7 s7 of .*k\.txt is not in .*absent\.fam"):
            cli.main(mode + ["--keep", str(tmp_path / "k.txt")])
    (tmp_path / "all.txt").write_text("".join(f"s{i}\n" for i in range(5)))
    with pytest.raises(SystemExit, match=r"--remove .*all\.txt leaves no sample"):
        cli.main(base + ["--remove", str(tmp_path / "all.txt")])
    # a run-file mode: the .Q must have one row per KEPT sample
    (tmp_path / "k.txt").write_text("f1 s1\ns3\n")
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    kin = ["kinship", "--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed), "--keep", str(tmp_path / "k.txt")]
    with pytest.raises(SystemExit, match=r"run\.3\.Q holds a 5 x 3 matrix, the data needs 2 x 3"):
        cli.main(kin)
    # train --pops_path: one line per sample of the .fam, filtered with the same mask
    assert cli._filter_lines(list("abcde"), np.asarray([0, 1, 0, 1, 0], dtype=bool), "pops") == ["b", "d"]
    assert cli._filter_lines(list("abc"), None, "pops") == list("abc")
    with pytest.raises(SystemExit, match=r"pops holds 3 lines, the \.fam 5 samples"):
        cli._filter_lines(list("abc"), np.ones(5, dtype=bool), "pops")
    # non-unique IDs end king, --keep and --remove, naming the first duplicate
    (tmp_path / "absent.fam").write_text("f0 s0\nf1 s1\nf2 s2\nf1 s1\nf2 s2\n")
    with pytest.raises(SystemExit, match=r"Sample f1 s1 occurs more than once in .*absent\.fam"):
        cli.main(base)
    with pytest.raises(SystemExit, match=r"Sample f1 s1 occurs more than once in .*absent\.fam"):
        cli.main(["pca"] + base[1:] + ["--remove", str(tmp_path / "k.txt")])
    assert not (tmp_path / "out").exists()
    with pytest.raises(AssertionError, match='Please provide either the argument "train" or "infer"'):
        cli.main(["kings"])


def test_sharded_engines_refuse_king():
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan = "dp", 2, None
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.king()
    e.mode, e.world, e.xp = "single", 1, None
    with pytest.raises(RuntimeError, match="needs the HIP engine"):
        e.king(0.1)


def test_estimator_on_the_planted_panel():
    """The estimator itself, float64 oracle only, on one fixed seed: every planted duplicate, first- and second-degree pair falls in
    its own band, no unrelated pair reaches the third-degree edge, and unrelated_set at the second-degree cutoff leaves no planted
    pair of degree <= 2 among the kept samples.  SEEN in numpy over seeds 0..3 (124 x 12000): unrelated max 0.023 .. 0.032, second
    degree 0.096 .. 0.137, first degree 0.235 .. 0.261, duplicates exactly 0.5, between-population pairs down to -0.16; 76 kept."""
    from neural_admixture_amd import king, relate
    G, degree = KO.make_panel(0)
    assert G.shape == (124, 12000) and 0.04 < (G == 3).mean() < 0.06
    assert [e for e, _ in relate.BANDS] == list(KO.EDGES)
    phi = king.phi_from_counts(KO.counts(G, G))
    iu = np.triu_indices(len(G), 1)
    assert [(degree[iu] == d).sum() for d in (0, 1, 2)] == [12, 120, 36]
    for a, b in zip(*iu):
        if degree[a, b] <= 2:
            assert KO.band(phi[a, b]) == degree[a, b], (a, b, degree[a, b], phi[a, b])
        else:
            assert phi[a, b] < KO.EDGES[3], (a, b, phi[a, b])
    assert (phi[iu][degree[iu] == 0] == 0.5).all() and phi[iu].min() < -0.1
    assert np.array_equal(np.diagonal(phi), np.full(len(G), 0.5)) and np.array_equal(phi, phi.T)
    i, j = np.nonzero(np.triu(phi >= KO.EDGES[2], 1))
    keep = king.unrelated_set(len(G), i, j)
    assert not any(keep[a] and keep[b] for a, b in zip(*iu) if degree[a, b] <= 2)
    assert keep[12 * 7:].all() and 12 * 3 + 40 <= keep.sum()      # the 40 unrelated samples stay, and at least three of every family
    _check_set(len(G), i.tolist(), j.tolist(), keep)


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(M):
    """ROWS resident rows with the planted rows of king_oracle.random_genotypes, their packed form and the oracle's counts of every
    pair of them; the tests leave them as they are."""
    G = KO.random_genotypes(ROWS, M, seed=M)
    full = KO.counts(G, G)
    G.setflags(write=False)
    full.setflags(write=False)
    return G, _packed(G), full


def _want(M, idxA, idxB):
    full = _case(M)[2]
    ia = np.arange(ROWS) if idxA is None else idxA
    ib = np.arange(ROWS) if idxB is None else idxB
    return full[:, ia][:, :, ib]


def _rows(b, salt=0):
    """Rows of one side of a block: a permutation of the resident rows with the planted rows 0..4 in it, cut to b, the last entry a
    duplicate of the first; b = 1 is row 7 (+ salt)."""
    if b == 1:
        return np.asarray([7 + salt], dtype=np.int32)
    perm = np.random.default_rng(100 * b + salt).permutation(ROWS)
    perm = np.concatenate([np.arange(5), perm[perm >= 5]])[:b - 1]
    perm = perm[np.random.default_rng(100 * b + salt + 1).permutation(b - 1)]
    return np.concatenate([perm, perm[:1]]).astype(np.int32)


def _gpu_block(xp, M, idxA, idxB, ba=None, bb=None):
    from neural_admixture_amd import king
    dev = xp.device
    ia = None if idxA is None else torch.from_numpy(idxA).to(dev)
    ib = None if idxB is None else torch.from_numpy(idxB).to(dev)
    c = king.king_block(xp, M, ia, ib, len(idxA) if idxA is not None else (ba or xp.shape[0]), len(idxB) if idxB is not None else (bb or xp.shape[0]))
    torch.cuda.synchronize()
    return c


def _check(c, want, what):
    """counts equal, phi = phi_from_counts of the oracle's counts to 1e-15 with the same NaNs."""
    from neural_admixture_amd import king
    got = c.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    phi, phi64 = king.phi_from_counts(c).cpu().numpy(), king.phi_from_counts(want)
    assert np.array_equal(np.isnan(phi), np.isnan(phi64)), what
    ok = ~np.isnan(phi64)
    assert (np.abs(phi[ok] - phi64[ok]) <= 1e-15).all(), what
    return phi


@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("ba, bb", SHAPES)
def test_block_against_the_oracle(ba, bb, M):
    dev = _dev()
    G, xph, _ = _case(M)
    idxA, idxB = _rows(ba), _rows(bb, salt=7)
    if ba > 5:
        assert set(range(5)) <= set(idxA.tolist()) and idxA[-1] == idxA[0] and (np.diff(idxA) < 0).any() and not np.array_equal(idxA[:16], idxB[:16])
    c = _gpu_block(xph.to(dev), M, idxA, idxB)
    phi = _check(c, _want(M, idxA, idxB), f"ba={ba} bb={bb} M={M}")
    if ba > 5:                                               # the all-missing row 3: zero counts; it and the het-free row 2: NaN against everyone
        got = c.cpu().numpy()
        for a in np.nonzero(idxA == 3)[0]:
            assert not got[:, a].any()
        for b in np.nonzero(idxB == 3)[0]:
            assert not got[:, :, b].any()
        assert np.isnan(phi[np.isin(idxA, (2, 3))]).all() and np.isnan(phi[:, np.isin(idxB, (2, 3))]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ba, bb, M, one_range", [(37, 70, 70001, False), (16, 17, 64, True), (130, 64, 3001, False)])
def test_one_range_and_several(ba, bb, M, one_range):
    """(37, 70) at M = 70001: 137 ranges of two chunks; (16, 17) at M = 64: one; (130, 64) at 3001: a range per chunk, the last ragged."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    r = int(lib.nadm_king_ranges(ba, bb, M))
    assert (r == 1) if one_range else (r > 1)
    if M == 70001:
        assert -(-((M + 255) // 256) // r) == 2
    G, xph, _ = _case(M)
    idxA, idxB = _rows(ba), _rows(bb, salt=7)
    _check(_gpu_block(xph.to(dev), M, idxA, idxB), _want(M, idxA, idxB), f"ba={ba} bb={bb} M={M}: {r} ranges")


@pytest.mark.gpu
def test_ranges_of_several_chunks():
    """The steady state of a real call: 1024 x 1024 rows (the resident ones with repeats) fill the chip with their 256 tiles, which
    leaves M = 3001 in 2 ranges of 6 chunks: the chunk loop hands the prefetched bytes over and accumulates across chunks."""
    from neural_admixture_amd._lib import lib
    dev = _dev()
    b, M = 1024, 3001
    ranges, chunks = int(lib.nadm_king_ranges(b, b, M)), (M + 255) // 256
    assert ranges >= 2 and -(-chunks // ranges) >= 2
    G, xph, _ = _case(M)
    idxA = np.random.default_rng(11).integers(0, ROWS, size=b).astype(np.int32)
    idxB = np.random.default_rng(12).integers(0, ROWS, size=b).astype(np.int32)
    _check(_gpu_block(xph.to(dev), M, idxA, idxB), _want(M, idxA, idxB), f"ba=bb={b} M={M}: {ranges} ranges")


@pytest.mark.gpu
def test_rows_without_a_gather_list_and_the_same_list_on_both_sides():
    dev = _dev()
    M = 1027
    G, xph, _ = _case(M)
    xp = xph.to(dev)
    none = _gpu_block(xp, M, None, None)
    _check(none, _want(M, None, None), f"rows 0..{ROWS} without a gather list")
    c = none.cpu().numpy()                                   # the diagonal: hethet == het_a == het_b, ibs0 == 0, phi exactly 0.5
    d = np.arange(ROWS)
    assert np.array_equal(c[1, d, d], c[3, d, d]) and np.array_equal(c[1, d, d], c[4, d, d]) and not c[2, d, d].any()
    from neural_admixture_amd import king
    phi = king.phi_from_counts(none).cpu().numpy()
    het = c[1, d, d] > 0
    assert het.sum() == ROWS - 2 and (phi[d, d][het] == 0.5).all() and np.isnan(phi[d, d][~het]).all()
    assert phi[0, 1] == 0.5 and phi[0, 4] < 0                # the duplicate; the mirrored row
    _check(_gpu_block(xp, M, None, _rows(70), ba=37), _want(M, np.arange(37), _rows(70)), "the first 37 rows against a list")
    idx = _rows(70)
    dev_idx = torch.from_numpy(idx).to(dev)
    same = king.king_block(xp, M, dev_idx, dev_idx, 70, 70)
    _check(same, _want(M, idx, idx), "idxA is idxB")


@pytest.mark.gpu
def test_what_must_not_matter_and_reproducibility():
    """Ones in the pad fields of every row's last byte and in the bytes behind it leave the counts identical; counts(A, B) is
    counts(B, A) transposed with het_a / het_b exchanged; two calls give the same bits; the 0 <-> 2 flip of the whole matrix changes
    no count."""
    dev = _dev()
    M = 1027
    G, xph, _ = _case(M)
    assert M % 4 and xph.shape[1] > (M + 3) // 4
    idxA, idxB = _rows(70), _rows(130, salt=7)
    clean = _gpu_block(xph.to(dev), M, idxA, idxB)
    _check(clean, _want(M, idxA, idxB), "clean")
    dirty_h = _packed(G, dirty=True)
    assert not torch.equal(dirty_h, xph)
    rnd = np.random.default_rng(3)                           # random garbage rather than ones
    a = dirty_h.numpy()
    a[:, (M + 3) // 4:] = rnd.integers(0, 256, size=a[:, (M + 3) // 4:].shape, dtype=np.uint8)
    a[:, M // 4] = (a[:, M // 4] & ((1 << (2 * (M % 4))) - 1)) | (rnd.integers(0, 256, size=len(a), dtype=np.uint8) & (0xFF << (2 * (M % 4)) & 0xFF))
    dirty = _gpu_block(dirty_h.to(dev), M, idxA, idxB)
    assert torch.equal(clean, dirty)
    again = _gpu_block(xph.to(dev), M, idxA, idxB)
    assert clean.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    t = _gpu_block(xph.to(dev), M, idxB, idxA)
    assert torch.equal(clean, t[[0, 1, 2, 4, 3]].transpose(1, 2))
    flipped = _gpu_block(_packed(KO.flip(G)).to(dev), M, idxA, idxB)
    assert torch.equal(clean, flipped)


@pytest.mark.gpu
def test_rows_beyond_4_gib_and_a_side_stream():
    """Three rows with ld = 2^31 (rows at byte 0, 2^31 and 2^32; 6 GiB of address space of which the head of every row is touched)
    give the counts of the compact rows; the same call on a side stream, enqueued behind a delay and behind the copy that makes its
    operand true (until then the matrix holds the missing code everywhere), gives the same counts."""
    from neural_admixture_amd import king
    dev = _dev()
    M = 1027
    G, xph, _ = _case(M)
    idx = np.asarray([2, 0, 1, 2, 0], dtype=np.int32)
    want = KO.counts(G[idx], G[[1, 0, 2]])
    compact = xph[:3].contiguous().to(dev)
    dev_idx, dev_idb = torch.from_numpy(idx).to(dev), torch.from_numpy(np.asarray([1, 0, 2], dtype=np.int32)).to(dev)
    ref = king.king_block(compact, M, dev_idx, dev_idb, 5, 3)
    _check(ref, want, "compact")
    free, _ = torch.cuda.mem_get_info()
    if free < (3 << 31) + (2 << 30):
        pytest.skip(f"the huge matrix needs 6 GiB + 2 GiB of free HBM, {free / 2 ** 30:.2f} GiB are free")
    huge = torch.empty((3, 1 << 31), dtype=torch.uint8, device=dev)
    huge[:, :4096] = 0xFF
    huge[:, : compact.shape[1]] = compact
    got = king.king_block(huge, M, dev_idx, dev_idb, 5, 3)
    none = king.king_block(huge, M, None, None, 3, 3)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    _check(none, KO.counts(G[:3], G[:3]), "huge, no gather list")
    del huge, got, none
    torch.cuda.empty_cache()
    # side stream
    live = xph.to(dev)
    decoy = torch.full_like(live, 0xFF)
    scratch = king.king_scratch(70, 130, M, dev)
    idxA, idxB = _rows(70), _rows(130, salt=7)
    dA, dB = torch.from_numpy(idxA).to(dev), torch.from_numpy(idxB).to(dev)
    first = king.king_block(live, M, dA, dB, 70, 130, scratch).clone()
    assert not king.king_block(decoy, M, dA, dB, 70, 130, scratch).any()      # (the scratch now holds another call's partial sums)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        decoy.copy_(live, non_blocking=True)
        out = king.king_block(decoy, M, dA, dB, 70, 130, scratch)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(out, first) and first.any()


@pytest.mark.gpu
def test_dense_pair_and_engine_forms():
    """king() with 64-row blocks on N = 150 equals ONE 150 x 150 block, king_pairs lists exactly the oracle's pairs in (i, j) order, and
    Engine.king equals king_pairs on the same matrix and leaves the parameters as they are."""
    import neural_admixture_amd as na
    from neural_admixture_amd import king
    from oracle import nadm_oracle as O
    dev = _dev()
    M, N = 1027, ROWS
    G, xph, full = _case(M)
    xp = xph.to(dev)
    one = _gpu_block(xp, M, None, None)
    phi, counts = king.king(xp, M, rows=64)
    assert phi.shape == (N, N) and phi.dtype == torch.float64 and counts.shape == (5, N, N) and counts.dtype == torch.int32
    assert torch.equal(counts, one) and np.array_equal(counts.cpu().numpy(), full)
    phi = phi.cpu().numpy()
    phi64 = king.phi_from_counts(full)
    assert np.array_equal(phi, phi64, equal_nan=True) and np.array_equal(phi, phi.T, equal_nan=True)
    idx = torch.from_numpy(_rows(70)).to(dev)
    sub, csub = king.king(xp, M, idx=idx, rows=33)
    assert np.array_equal(csub.cpu().numpy(), _want(M, _rows(70), _rows(70)))
    for thr in (king.MIN_PHI, 0.0, -1.0):
        for rows in (64, 1024):
            i, j, p, n, hh, i0 = (v.cpu().numpy() for v in king.king_pairs(xp, M, min_phi=thr, rows=rows))
            wi, wj = np.nonzero(np.triu(phi64 >= thr, 1))
            assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(p, phi64[wi, wj])
            assert np.array_equal(n, full[0][wi, wj]) and np.array_equal(hh, full[1][wi, wj]) and np.array_equal(i0, full[2][wi, wj])
            assert i.dtype == np.int64 and p.dtype == np.float64 and n.dtype == np.int32
    assert (0, 1) in set(zip(wi.tolist(), wj.tolist())) and len(wi) > 1000
    # the engine
    C_, Hd, ks = 8, 32, [3]
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, C_)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(sum(ks), M)).astype(np.float32)
    p_ = O.make_params(42, V0, P0, Hd, ks)
    small = np.concatenate([p_.g, p_.W1.reshape(-1), p_.b1] + [x for h in range(len(ks)) for x in (p_.Wk[h].reshape(-1), p_.bk[h])])
    e = na.Engine(M, C_, Hd, ks, dev, 64)
    e.load_params(V0, P0, small)
    e.pack_from_host(torch.from_numpy(np.ascontiguousarray(G)))
    e.sync()
    before = [t.clone() for t in (e.pflat, e.mflat, e.vflat)]
    for thr in (None, 0.0):
        got = e.king(min_phi=thr, rows=64)
        want = king.king_pairs(e.xp, M, min_phi=king.MIN_PHI if thr is None else thr, rows=64)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].numel() >= 1
        ref = king.king_pairs(xp, M, min_phi=king.MIN_PHI if thr is None else thr)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


def _orient_case(subset_heavy):
    """40 x 101 genotypes whose first 10 samples carry mostly 2s and the rest mostly 0s (``subset_heavy``), or the other way round: the
    file's mean code and the subset's lie on different sides of 1."""
    rng = np.random.default_rng(9)
    G = rng.binomial(2, 0.1, size=(40, 101)).astype(np.uint8)
    G[:10] = rng.binomial(2, 0.9, size=(10, 101))
    if not subset_heavy:
        G = KO.flip(G)
    G[rng.random(G.shape) < 0.05] = 3
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("subset_heavy", [True, False])
def test_select_samples_is_the_reader_on_a_smaller_file(tmp_path, subset_heavy):
    from neural_admixture_amd import king
    from neural_admixture_amd.io import read_bed_packed
    dev = _dev()
    G = _orient_case(subset_heavy)
    keep = np.zeros(40, dtype=bool)
    keep[[0, 2, 3, 5, 6, 7, 9, 17]] = True                   # seven of the first ten and one of the rest
    assert (G.mean() < 1) == subset_heavy and (G[keep].mean() >= 1) == subset_heavy
    LO.write_bed(tmp_path / "full", G)
    LO.write_bed(tmp_path / "part", G[keep])
    for on_device in (True, False):
        full = read_bed_packed(str(tmp_path / "full.bed"), dev, keep_on_device=on_device)
        part = read_bed_packed(str(tmp_path / "part.bed"), dev, keep_on_device=on_device)
        assert full.flipped != part.flipped
        got = king.select_samples(full, keep)
        assert (got.N, got.M, got.flipped) == (part.N, part.M, part.flipped) == (8, 101, part.flipped)
        assert got.packed.device == part.packed.device and got.packed.shape == part.packed.shape
        assert torch.equal(got.packed, part.packed)
        same = king.select_samples(full, np.ones(40, dtype=bool))
        assert torch.equal(same.packed, full.packed) and same.flipped == full.flipped
    with pytest.raises(RuntimeError, match="selects no sample"):
        king.select_samples(full, np.zeros(40, dtype=bool))
    with pytest.raises(RuntimeError, match="one entry per sample"):
        king.select_samples(full, np.ones(39, dtype=bool))


@pytest.mark.gpu
def test_cli_king_end_to_end(tmp_path, caplog):
    """The `king` mode on a written BED of the planted panel (3000 SNPs; compared with the oracle's own answer at that M): .king,
    .king.in and .king.out hold the oracle's pairs and unrelated_set's lists; `train --keep` on the kept samples writes a .Q with one
    row per kept sample; `pca --remove` of the removed equals `pca --keep` of the kept."""
    from neural_admixture_amd import cli, king
    from neural_admixture_amd.io import read_sample_list
    G = np.ascontiguousarray(KO.make_panel(0)[0][:, :3000])
    N, M = G.shape
    LO.write_bed(tmp_path / "panel", G)
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    bed = str(tmp_path / "panel.bed")
    assert cli.main(["king", "--data_path", bed, "--save_dir", str(out), "--name", "rel", "--rows", "64"]) == 0
    phi64 = king.phi_from_counts(KO.counts(G, G))
    full = KO.counts(G, G)
    wi, wj = np.nonzero(np.triu(phi64 >= 2.0 ** -3.5, 1))
    lines = [ln.split() for ln in (out / "rel.king").read_text().splitlines()]
    assert len(lines) == len(wi) >= 12 * 11
    assert [(int(f[0]), int(f[1])) for f in lines] == list(zip(wi.tolist(), wj.tolist()))
    assert [float(f[2]) for f in lines] == phi64[wi, wj].tolist()
    for k, col in ((0, 3), (1, 4), (2, 5)):
        assert [int(f[col]) for f in lines] == full[k][wi, wj].tolist()
    assert all(f[2] == format(p, ".17g") for f, p in zip(lines, phi64[wi, wj].tolist()))
    keep = king.unrelated_set(N, wi, wj)
    ids = [(f"f{i}", f"s{i}") for i in range(N)]
    assert read_sample_list(out / "rel.king.in") == [s for s, k in zip(ids, keep) if k]
    assert read_sample_list(out / "rel.king.out") == [s for s, k in zip(ids, keep) if not k]
    msgs = [r.getMessage() for r in caplog.records]
    from neural_admixture_amd import relate
    for label, edge, count in relate.band_counts(phi64[wi, wj]):
        assert any(f"{label} (>= {edge:.4f}): {count}" in m for m in msgs), label
    assert any(f"{int((~keep).sum())} samples removed, {int(keep.sum())} kept" in m for m in msgs)
    # train on the kept samples
    assert cli.main(["train", "--epochs", "2", "--k", "3", "--name", "run", "--data_path", bed, "--save_dir", str(out), "--seed", "42",
                     "--batch_size", "800", "--hidden_size", "128", "--keep", str(out / "rel.king.in")]) == 0
    Q, P = np.loadtxt(out / "run.3.Q", ndmin=2), np.loadtxt(out / "run.3.P", ndmin=2)
    assert Q.shape == (int(keep.sum()), 3) and P.shape == (M, 3)
    assert any(f"Using the {int(keep.sum())} samples of --keep / --remove" in r.getMessage() for r in caplog.records)
    # pca --remove of the removed == pca --keep of the kept
    for name, flag, lst in (("a", "--keep", "rel.king.in"), ("b", "--remove", "rel.king.out")):
        assert cli.main(["pca", "--data_path", bed, "--save_dir", str(out), "--name", name, "--pcs", "4", flag, str(out / lst)]) == 0
    assert (out / "a.eigenval").read_text() == (out / "b.eigenval").read_text() and len((out / "a.eigenval").read_text().split()) == 4
    assert (out / "a.eigenvec").read_text() == (out / "b.eigenvec").read_text()
    assert len((out / "a.eigenvec").read_text().splitlines()) == int(keep.sum())
