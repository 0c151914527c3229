"""Admixture dating, the part that needs no GPU: nadm_wld's symbol, limits and host refusals, the grid and the reach, the .bim map
reader, the decay fit and its jackknife, the `date` parser's refusals, and the calibration of the whole procedure in float64 on the
CPU (the restatement of tests/wld_oracle.py on a simulated panel of known age)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wld_oracle as WO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_limits_are_in_the_library_and_the_header():
    from neural_admixture_amd import _lib, admixdate
    hdr = open(os.path.join(ROOT, "include", "nadm.h")).read()
    for name, value in (("NADM_WLD_MAX_CURVES", 32), ("NADM_WLD_MAX_BINS", 4096), ("NADM_WLD_MAX_SPAN", 65536)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert re.search(r"\bint nadm_wld\(", hdr)
    assert "nadm_wld" in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), "nadm_wld")
    assert (admixdate.MAX_CURVES, admixdate.MAX_BINS, admixdate.MAX_SPAN) == (32, 4096, 65536)
    assert "nadm_wld.hip" in open(os.path.join(ROOT, "neural-admixture_amd", "csrc", "build.sh")).read()


def test_every_host_refusal_comes_with_its_reason_and_without_a_launch():
    """The pointers are fakes that are never followed: every refusal is decided from the arguments alone."""
    from neural_admixture_amd._lib import lib, check
    ok = C.c_void_p(0x10000)

    def call(xp=ok, ld=64, idx=None, rows=8, M=200, m0=0, m1=200, W=10, cell=ok, wt=ok, Cn=2, nbins=16, nmin=2, sum_=ok, cnt=ok):
        return lib.nadm_wld(xp, ld, idx, rows, M, m0, m1, W, cell, wt, Cn, nbins, nmin, sum_, cnt, None)

    at = lambda a: C.c_void_p(0x10000 + a)      # noqa: E731
    cases = [
        (dict(xp=None), "null pointer"), (dict(cell=None), "null pointer"), (dict(wt=None), "null pointer"),
        (dict(sum_=None), "null pointer"), (dict(cnt=None), "null pointer"),
        (dict(xp=at(8)), "xp must be 16-byte aligned"),
        (dict(wt=at(4)), "wt, sum and cnt must be 8-byte aligned"), (dict(sum_=at(4)), "wt, sum and cnt must be 8-byte aligned"),
        (dict(cnt=at(4)), "wt, sum and cnt must be 8-byte aligned"),
        (dict(cell=at(2)), "cell and idx must be 4-byte aligned"), (dict(idx=at(2)), "cell and idx must be 4-byte aligned"),
        (dict(rows=1), "rows must be in 2..2^24"), (dict(rows=(1 << 24) + 1), "rows must be in 2..2^24"),
        (dict(Cn=0), "C must be in 1..NADM_WLD_MAX_CURVES"), (dict(Cn=33), "C must be in 1..NADM_WLD_MAX_CURVES"),
        (dict(nbins=0), "nbins must be in 1..NADM_WLD_MAX_BINS"), (dict(nbins=4097), "nbins must be in 1..NADM_WLD_MAX_BINS"),
        (dict(W=0), "W must be in 1..NADM_WLD_MAX_SPAN"), (dict(W=65537), "W must be in 1..NADM_WLD_MAX_SPAN"),
        (dict(nmin=1), "nmin must be >= 2"),
        (dict(m0=-1), "need 0 <= m0 < m1 <= M"), (dict(m0=5, m1=5), "need 0 <= m0 < m1 <= M"), (dict(m1=201), "need 0 <= m0 < m1 <= M"),
        (dict(ld=48), "ld < ceil(M/4)"), (dict(ld=72), "ld must be a multiple of 16 and < 2^32"),
        (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
        (dict(M=1 << 38, m1=1 << 38, ld=1 << 36), "ld must be a multiple of 16 and < 2^32"),
    ]
    for kw, msg in cases:
        with pytest.raises(RuntimeError, match=re.escape("nadm_wld: " + msg)):
            check(call(**kw), "wld")


def test_grid_cells_gaps_refusal_and_reach():
    from neural_admixture_amd import admixdate as ad
    rng = np.random.default_rng(3)
    cm = np.concatenate([np.sort(rng.uniform(0, 3.0, 70)), np.sort(rng.uniform(10.0, 12.0, 45)), np.sort(rng.uniform(0, 0.3, 9))])
    chrom = np.concatenate([np.full(70, 4), np.full(45, 7), np.full(9, 9)])
    nbins = 12
    cell, ranges = ad.grid_cells(cm, chrom, 0.05, nbins)
    assert cell.dtype == np.int32 and ranges == [(0, 70), (70, 115), (115, 124)]
    assert np.all(np.diff(cell.astype(np.int64)) >= 0)
    for m0, m1 in ranges:
        assert np.array_equal(cell[m0:m1] - cell[m0], np.floor((cm[m0:m1] - cm[m0]) / 0.05).astype(np.int64))
    assert cell[0] == 0 and cell[70] - cell[69] == nbins + 1 and cell[115] - cell[114] == nbins + 1     # more than nbins between chromosomes
    # the reach against a brute-force count
    want = 1
    for m0, m1 in ranges:
        for a in range(m0, m1):
            for b in range(a + 1, m1):
                if cell[b] - cell[a] < nbins:
                    want = max(want, b - a)
    assert ad.reach(cell, nbins, ranges) == want and want > 1
    assert ad.reach(np.arange(0, 500, 50), 12, [(0, 10)]) == 1                      # nothing within reach: still 1
    bad = cm.copy()
    bad[80], bad[81] = bad[81] + 0.001, bad[80] - 0.001
    with pytest.raises(RuntimeError, match=r"decreases within a chromosome at SNP 81 "):
        ad.grid_cells(bad, chrom, 0.05, nbins)
    w = ad.component_weights(np.asarray([[0.25, 0.5, 1.0], [0.75, 0.5, 0.0]], dtype=np.float32), [(0, 2), (1, 0)])
    assert w.dtype == np.float64 and np.array_equal(w, [[-0.75, 0.75], [0.25, -0.25]])
    with pytest.raises(RuntimeError, match="two different components"):
        ad.component_weights(np.zeros((2, 3)), [(1, 1)])
    assert ad.choose_pairs(np.asarray([[0.5, 0.46, 0.04], [0.5, 0.46, 0.04]])) == [(0, 1)]


def test_read_bim_map_centimorgans_morgans_and_the_rate_fallback(tmp_path):
    from neural_admixture_amd.io import genetic_map, read_bim, read_bim_map
    p = tmp_path / "x.bim"
    p.write_text("1 rs1 0.5 1000 A G\n1 rs2 1.25 2500000 A G\n2 rs3 0 700 C T\n")
    cm, bp = read_bim_map(p)
    assert cm.dtype == np.float64 and bp.dtype == np.int64
    assert np.array_equal(cm, [0.5, 1.25, 0.0]) and np.array_equal(bp, [1000, 2500000, 700])
    assert read_bim(p) == (["rs1", "rs2", "rs3"], ["1", "1", "2"])                   # (the ID reader is what it was)
    got, from_rate = genetic_map(cm, bp)
    assert not from_rate and np.array_equal(got, cm)
    got, from_rate = genetic_map(cm, bp, morgans=True)
    assert not from_rate and np.array_equal(got, [50.0, 125.0, 0.0])
    p.write_text("1 rs1 0 1000 A G\n1 rs2 0 2500000 A G\n")
    cm, bp = read_bim_map(p)
    got, from_rate = genetic_map(cm, bp, rate=2.0)
    assert from_rate and np.allclose(got, [0.002, 5.0], rtol=1e-15)
    got, from_rate = genetic_map(cm, bp, morgans=True)
    assert from_rate and np.allclose(got, [0.001, 2.5], rtol=1e-15)
    p.write_text("1 rs1 0\n")
    with pytest.raises(SystemExit, match="line 1 has fewer than four columns"):
        read_bim_map(p)
    p.write_text("1 rs1 x 5 A G\n")
    with pytest.raises(SystemExit, match="line 1 holds a genetic or base-pair position that is not a number"):
        read_bim_map(p)


def test_fit_decay_recovers_a_planted_curve_and_identical_chromosomes_have_no_spread():
    from neural_admixture_amd import admixdate as ad
    d = np.arange(400) * 0.05
    rng = np.random.default_rng(0)
    cnt = rng.integers(1000, 5000, size=400)
    for A, n, c in ((3e-3, 20.0, 1e-5), (-2e-4, 147.3, 0.0), (1.0, 1.7, -0.25), (5e-3, 600.0, 2e-4)):
        y = A * np.exp(-n * d / 100.0) + c
        got = ad.fit_decay(d, y, cnt, 0.5, 20.0)
        for g, w in zip(got, (n, A, c)):
            assert abs(g - w) <= 1e-9 * max(abs(w), abs(A)), (got, (n, A, c))
    y = 3e-3 * np.exp(-20.0 * d / 100.0)
    y[:10] = 1.0                                           # below dmin: not fitted
    assert abs(ad.fit_decay(d, y, cnt, 0.5, 20.0)[0] - 20.0) < 1e-7
    assert all(v != v for v in ad.fit_decay(d[:12], y[:12], cnt[:12], 0.5, 20.0))        # two bins: nothing to fit
    # the jackknife of identical chromosomes: every leave-one-out curve is the full curve
    nb = 100
    dd = np.arange(nb) * 0.05
    cnt1 = rng.integers(100, 200, size=nb).astype(np.int64)
    noise = 1.0 + 0.05 * rng.standard_normal(nb)
    s1 = np.rint(cnt1 * (2e-3 * np.exp(-30.0 * dd / 100.0) * noise + 1e-5) * ad.SCALE).astype(np.int64)
    res = ad.date_from_curves(np.stack([s1[None]] * 4), np.stack([cnt1] * 4), 0.05, 0.5, 5.0, [(0, 1)])
    r = res.results[0]
    assert 20.0 < r.generations < 40.0 and (r.a, r.b) == (0, 1)
    assert 0.0 <= r.se <= 1e-9 * r.generations and 0.0 <= r.se_A <= 1e-9 * abs(r.A) and 0.0 <= r.se_c <= 1e-9 * abs(r.A)
    one = ad.date_from_curves(s1[None, None], cnt1[None], 0.05, 0.5, 5.0, [(0, 1)]).results[0]
    assert one.generations == r.generations and all(v != v for v in (one.se, one.se_A, one.se_c, one.z))    # one chromosome: nan
    assert ad.jackknife(1.0, [0.9, 1.1, 1.0], [10, 10, 10]) == pytest.approx(np.sqrt(2.0 / 3.0 * 0.02), rel=1e-12)  # the delete-one formula at equal weights


def test_cli_date_refuses_before_the_gpu_check(tmp_path, monkeypatch):
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["date", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_date_args(base[1:] + ["--k", "3"])
    assert (a.binsize, a.mindist, a.maxdist, a.min_share, a.pairs, a.target, a.pops_path, a.morgans, a.rate, a.nmin, a.extract) == \
        (0.05, 0.5, 20.0, 0.05, None, None, None, False, 1.0, 2, None)
    assert "date" in cli._ANALYSIS_MODES

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    k3 = ["--k", "3"]
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    for extra, msg in ((["--binsize", "0"], r"--binsize must be > 0"), (["--mindist", "20"], r"--mindist must be >= 0 and below --maxdist"),
                       (["--maxdist", "500"], r"gives 10000 bins, more than 4096: use a larger bin or a smaller --maxdist"),
                       (["--min_share", "0.7"], r"--min_share must be in \[0, 0.5\]"), (["--rate", "0"], r"--rate must be > 0"),
                       (["--nmin", "1"], r"--nmin must be >= 2"), (["--target", "A"], r"--target names a label of --pops_path"),
                       (["--pairs", "1-4"], r"--pairs takes component pairs like 1-2,1-3"), (["--pairs", "2-2"], r"--pairs takes component pairs"),
                       (["--pairs", "a-b"], r"--pairs takes component pairs"),
                       (["--pops_path", str(tmp_path / "nopops")], r"nopops not found")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + k3 + extra)
    with pytest.raises(SystemExit, match=r"not available for VCF input"):
        cli.main(base[:-1] + [str(tmp_path / "x.vcf")] + k3)
    with pytest.raises(SystemExit, match=r"date needs the .*run\.3\.P not found"):
        cli.main(base + k3)
    np.savetxt(tmp_path / "run.3.P", np.full((6, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"x\.bim not found"):
        cli.main(base + k3)
    (tmp_path / "x.fam").write_text("".join(f"f s{i} 0 0 0 -9\n" for i in range(5)))
    bed.write_bytes(bytes(3 + 2 * 6))                        # N = 5, M = 6
    (tmp_path / "x.bim").write_text("".join(f"1 rs{j} {c} {1000 * j} A G\n" for j, c in enumerate((0.0, 0.1, 0.3, 0.2, 0.4, 0.5))))
    with pytest.raises(SystemExit, match=r"x\.bim: grid_cells: the genetic map decreases within a chromosome at SNP 3 "):
        cli.main(base + k3)
    (tmp_path / "x.bim").write_text("".join(f"1 rs{j} {0.1 * j} {1000 * j} A G\n" for j in range(6)))
    (tmp_path / "pops").write_text("A\nB\nA\nB\n")
    with pytest.raises(SystemExit, match=r"--target C: 0 samples"):
        cli.main(base + k3 + ["--pops_path", str(tmp_path / "pops"), "--target", "C"])
    with pytest.raises(SystemExit, match=r"pops lists 4 labels, the data holds 5 samples"):
        cli.main(base + k3 + ["--pops_path", str(tmp_path / "pops"), "--target", "A"])
    np.savetxt(tmp_path / "run.3.P", np.full((7, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.P"):
        cli.main(base + k3)
    np.savetxt(tmp_path / "run.3.P", np.full((6, 3), 0.5))
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + k3)


def test_sharded_and_cpu_engines_refuse_admix_date_and_wld_curves_refuses_a_cpu_matrix():
    from neural_admixture_amd import admixdate as ad
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.admix_date is single-GPU"):
        e.admix_date(np.zeros(4), np.zeros(4))
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.admix_date needs the HIP engine with its packed matrix resident"):
        e.admix_date(np.zeros(4), np.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ad.wld_curves(torch.zeros((4, 16), dtype=torch.uint8), 40, np.zeros(40, dtype=np.int32), np.zeros((1, 40)), 4)


# ---- calibration of the procedure, float64 on the CPU -----------------------------------------------------------------------------
CAL = dict(N=200, chroms=4, snps=1500, spacing=0.02, n_gen=20.0, fst=0.2, miss=0.05)


@pytest.mark.parametrize("seed", range(5))
def test_the_procedure_dates_a_simulated_admixture(seed):
    """200 samples x 4 chromosomes x 1500 SNPs every 0.02 cM, 20 generations after the pulse, source frequencies with Fst 0.2, 5 % of the
    calls missing, weights from the true source frequencies; the restatement's integers (Gram products per chromosome, not a pair loop)
    through the package's own fit and jackknife.  Both must hold for every seed: |n - 20| <= 3 se, and se <= 5 (a huge error bar
    passes nothing).  Measured (n, se) for seeds 0..4: (19.68, 0.44), (20.37, 0.56), (20.39, 0.63), (19.89, 1.10), (18.96, 0.58)."""
    from neural_admixture_amd import admixdate as ad
    G, cm, chrom, pa, pb = WO.simulate(seed, CAL["N"], CAL["chroms"], CAL["snps"], CAL["spacing"], CAL["n_gen"], CAL["fst"], miss=CAL["miss"])
    nbins = ad.check_args(ad.BINSIZE, ad.DMIN, ad.MAXDIST)
    cell, ranges = ad.grid_cells(cm, chrom, ad.BINSIZE, nbins)
    s, n = WO.wld_restatement_ranges(G, ranges, ad.reach(cell, nbins, ranges), cell, (pa - pb)[None], nbins)
    r = ad.date_from_curves(s, n, ad.BINSIZE, ad.DMIN, ad.MAXDIST).results[0]
    print(f"seed {seed}: n = {r.generations:.3f}, se = {r.se:.3f}, z = {r.z:.1f}")
    assert abs(r.generations - 20.0) <= 3.0 * r.se and r.se <= 5.0
