"""Local ancestry, the part that needs no GPU: nadm_local_anc's symbol and host refusals, the properties of the recursion in the numpy
restatement (tests/localanc_oracle.py), the calibration on a simulated panel in float64, the map helpers, the host-side checks of the
device lists, the writers, the `local` parser's refusals, and the register budget of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localanc_oracle as LO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-admixture_amd", "csrc")
EPS = 1e-6


def test_symbol_is_in_the_library_the_header_and_the_build():
    from neural_admixture_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nadm.h")).read()
    assert re.search(r"\bint nadm_local_anc\(", hdr) and re.search(r"\bint64_t nadm_local_anc_scratch_floats\(", hdr)
    for name in ("nadm_local_anc", "nadm_local_anc_scratch_floats"):
        assert name in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert "nadm_local_anc.hip" in open(os.path.join(CSRC, "build.sh")).read()
    assert _lib.lib.nadm_abi_version() == 14
    f = _lib.lib.nadm_local_anc_scratch_floats
    assert f(65, 9, 8) == 9 * 36 * 256 and f(257, 9, 16) == 9 * 136 * 512 and f(1, 0, 4) == 10 * 256
    assert f(0, 9, 8) == 0 and f(5, -1, 8) == 0 and f(5, 9, 24) == 0 and f(5, 9, 6) == 0


def test_every_host_refusal_comes_with_its_reason_and_without_a_launch():
    """The pointers are fakes that are never followed: every refusal is decided from the arguments alone."""
    from neural_admixture_amd._lib import lib, check
    ok = C.c_void_p(0x10000)
    at = lambda a: C.c_void_p(0x10000 + a)      # noqa: E731

    def call(xp=ok, ld=64, idx=None, b=8, M=200, P=ok, k=3, kp=4, Q=ok, qs=4, eps=1e-6, rho=ok, seg=ok, n_seg=1, out=ok, oseg=ok, n_out=4,
             dosage=ok, cl=ok, post=ok, ll=ok, scratch=ok):
        return lib.nadm_local_anc(xp, ld, idx, b, M, P, k, kp, Q, qs, eps, rho, seg, n_seg, out, oseg, n_out, dosage, cl, post, ll, scratch, None)

    cases = [(dict(xp=None), "null pointer"), (dict(P=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(rho=None), "null pointer"),
             (dict(seg=None), "null pointer"), (dict(ll=None), "null pointer"), (dict(cl=None), "a full call needs call, post, scratch"),
             (dict(post=None), "a full call needs"), (dict(scratch=None), "a full call needs"), (dict(out=None), "a full call needs"),
             (dict(oseg=None), "a full call needs"), (dict(b=0), "empty batch"), (dict(M=0), "empty batch"), (dict(M=1 << 31, ld=1 << 30), r"M must be < 2\^31"),
             (dict(ld=48), r"ld < ceil\(M/4\)"), (dict(ld=72), "ld must be a multiple of 16"), (dict(k=0), "K must be in 1"),
             (dict(kp=8), r"kp must be nadm_pad_k\(k\)"), (dict(qs=0), "q_stride < kp"), (dict(qs=6, kp=4), "q_stride must be a multiple of 4"),
             (dict(eps=0.0), "eps must be in"), (dict(eps=0.5), "eps must be in"), (dict(k=17, kp=24, qs=24), "K must be <= 16"),
             (dict(n_seg=0), "n_seg must be >= 1"), (dict(n_out=-1), "n_out must be in"), (dict(xp=at(8)), "16-byte aligned"),
             (dict(P=at(4)), "16-byte aligned"), (dict(Q=at(8)), "16-byte aligned"), (dict(scratch=at(4)), "16-byte aligned"),
             (dict(dosage=at(8)), "16-byte aligned"), (dict(ll=at(4)), "ll must be 8-byte"), (dict(rho=at(2)), "4-byte aligned"),
             (dict(seg=at(1)), "4-byte aligned"), (dict(out=at(2)), "4-byte aligned"), (dict(oseg=at(3)), "4-byte aligned"),
             (dict(post=at(2)), "4-byte aligned"), (dict(idx=at(2)), "4-byte aligned"),
             (dict(b=(1 << 31) - 1, n_seg=1 << 20), "too many blocks for one launch")]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        with pytest.raises(RuntimeError, match=msg):
            check(call(**kw), "local_anc")


# ---- the recursion's properties, in the restatement ---------------------------------------------------------------------------------
def _small(seed, n, M, K):
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.05, 0.95, size=(M, K)).astype(np.float32)
    Q = rng.dirichlet(np.ones(K), size=n).astype(np.float32)
    codes = rng.integers(0, 4, size=(n, M)).astype(np.uint8)
    return codes, P, Q


def test_without_linkage_the_likelihood_is_the_binomial_one():
    """rho = 1 everywhere: the SNPs are independent draws from binomial(2, pi), pi = q . p (the second factor is q . (1 - p), which is
    1 - pi up to the rounding of the fp32 row of Q).  Measured difference: 8e-11 relative."""
    codes, P, Q = _small(1, 7, 400, 4)
    res = LO.local_anc(codes, P, Q, EPS, np.ones(400), [0, 150, 400])
    q, p = Q.astype(np.float64), P.astype(np.float64)
    pi, ka = q @ p.T, q @ (1.0 - p).T
    pr = np.where(codes == 0, ka * ka, np.where(codes == 1, 2.0 * pi * ka, np.where(codes == 2, pi * pi, (pi + ka) ** 2)))
    want = np.stack([np.log(pr[:, :150]).sum(axis=1), np.log(pr[:, 150:]).sum(axis=1)], axis=1)
    rel = np.abs(res["ll"] - want).max() / np.abs(want).max()
    print(f"rho = 1: relative difference {rel:.2e}")
    assert rel < 1e-9


def test_without_a_redraw_the_posterior_is_constant_along_the_segment():
    """rho = 0 after the first SNP: one ancestry pair for the whole segment.  Measured spread: 5e-15."""
    codes, P, Q = _small(2, 6, 60, 3)
    pts = np.arange(60)
    res = LO.local_anc(codes, P, Q, EPS, np.zeros(60), [0, 60], pts, [0, 60])
    spread = np.abs(res["dosage"] - res["dosage"][:, :1]).max()
    print(f"rho = 0: spread {spread:.2e}")
    assert spread < 1e-12 and np.abs(res["post"] - res["post"][:, :1]).max() < 1e-12 and (res["call"] == res["call"][:, :1]).all()


def test_a_q_with_exact_zeros_against_its_data_gives_no_nan_in_either_dtype():
    """Q = (1, 0) and 20000 calls drawn from the other component: the sup mask keeps the supported states apart from the unsupported."""
    rng = np.random.default_rng(3)
    M = 20000
    P = rng.uniform(0.05, 0.95, size=(M, 2)).astype(np.float32)
    Q = np.asarray([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]], dtype=np.float32)
    codes = np.stack([(rng.random(M) < P[:, 1]).astype(np.uint8) + (rng.random(M) < P[:, 1]) for _ in range(3)]).astype(np.uint8)
    codes[1] = (rng.random(M) < P[:, 0]).astype(np.uint8) + (rng.random(M) < P[:, 0])
    rho = np.full(M, 0.01, dtype=np.float32)
    pts = np.arange(0, M, 997)
    for dt in (np.float64, np.float32):
        res = LO.local_anc(codes, P, Q, EPS, rho, [0, M], pts, [0, len(pts)], dtype=dt)
        assert np.isfinite(res["dosage"]).all() and np.isfinite(res["post"]).all() and np.isfinite(res["ll"]).all() and (res["call"] != 255).all(), dt
        assert (res["dosage"][0, :, 0] == 2.0).all() and (res["dosage"][1, :, 1] == 2.0).all()


# ---- calibration on a simulated panel, float64 on the CPU -----------------------------------------------------------------------------
CAL = dict(seed=3, N=24, chroms=2, snps=3000, spacing=0.02, n_gen=20.0, K=3, fst=0.2, miss=0.05)
COARSE = [2, 5, 10, 14, 20, 28, 40, 80, 200]


def test_linkage_beats_no_linkage_beats_the_prior_and_the_likelihood_peaks_at_the_truth():
    """24 samples x 2 chromosomes x 3000 SNPs every 0.02 cM, K = 3, 20 generations, Fst 0.2, 5 % missing, P and Q at the truth.  The
    mean squared error of the posterior dosage against the true dosage under linkage is below that with rho = 1, which is below the
    prior 2 q's; the total log-likelihood over the nine-value grid peaks at 20.  Relations, not thresholds; the measured values are in
    DESIGN.md section 4.22."""
    from neural_admixture_amd import localanc
    G, cm, chrom, P, Q, anc = LO.simulate(CAL["seed"], CAL["N"], CAL["chroms"], CAL["snps"], CAL["spacing"], CAL["n_gen"], CAL["K"],
                                          CAL["fst"], CAL["miss"])
    M = G.shape[1]
    rho, ranges = localanc.switch_prob(cm, chrom, 20.0)
    seg = [0, 3000, 6000]
    pts = np.concatenate([np.arange(0, 3000, 10), np.arange(3000, 6000, 10)])
    oseg = [0, 300, 600]
    truth = anc[:, pts, :].astype(np.float64)
    link = LO.local_anc(G, P, Q, EPS, rho, seg, pts, oseg)
    free = LO.local_anc(G, P, Q, EPS, np.ones(M), seg, pts, oseg)
    mse = [float(((d - truth) ** 2).mean()) for d in (link["dosage"], free["dosage"], np.broadcast_to(2.0 * Q[:, None, :], truth.shape))]
    print(f"dosage mse: linkage {mse[0]:.4f}, rho = 1 {mse[1]:.4f}, prior {mse[2]:.4f}")
    assert mse[0] < mse[1] < mse[2]
    share = link["dosage"] / 2.0                             # calibration: the true share where the posterior share is in a bin
    for lo in (0.0, 0.2, 0.4, 0.6, 0.8):
        sel = (share >= lo) & (share <= lo + 0.2)
        print(f"posterior share in [{lo:.1f}, {lo + 0.2:.1f}]: mean {share[sel].mean():.3f}, true {truth[sel].mean() / 2.0:.3f}")
    tot = [float(LO.local_anc(G, P, Q, EPS, localanc.switch_prob(cm, chrom, g)[0], seg)["ll"].sum()) for g in COARSE]
    print("log-likelihood over", COARSE, ":", " ".join(f"{t:.2f}" for t in tot))
    assert COARSE[int(np.argmax(tot))] == 20


# ---- the map helpers and the host-side checks ---------------------------------------------------------------------------------------
def test_switch_prob_and_output_points():
    from neural_admixture_amd import localanc as la
    cm = np.asarray([0.0, 0.1, 0.1, 2.0, 5.0, 5.5, 5.6, 9.0])
    chrom = np.asarray([1, 1, 1, 1, 2, 2, 2, 2])
    rho, ranges = la.switch_prob(cm, chrom, 20.0)
    assert ranges == [(0, 4), (4, 8)] and rho.dtype == np.float32 and rho[0] == 1.0 and rho[4] == 1.0 and rho[2] == 0.0
    want = 1.0 - np.exp(-20.0 * np.asarray([0.1, 0.0, 1.9]) / 100.0)
    assert (rho[1:4] == want.astype(np.float32)).all()
    out, oseg = la.output_points(cm, chrom, 1.0)
    # chromosome 1: marks 0, 1, 2 -> SNPs 0, 3, 3; chromosome 2: marks 0, 1, 2, 3 (3.5 rounds in) -> SNPs 4, 7
    assert out.tolist() == [0, 3, 4, 7] and oseg.tolist() == [0, 2, 4] and out.dtype == np.int32
    assert la.output_points(cm, chrom, 100.0)[0].tolist() == [0, 4]
    with pytest.raises(RuntimeError, match=r"the genetic map decreases within a chromosome at SNP 2 \(0.05 cM after 0.1 cM\)"):
        la.switch_prob(np.asarray([0.0, 0.1, 0.05]), np.zeros(3), 5.0)
    with pytest.raises(RuntimeError, match="decreases within a chromosome at SNP 2"):
        la.output_points(np.asarray([0.0, 0.1, 0.05]), np.zeros(3))
    with pytest.raises(RuntimeError, match="generations must be > 0"):
        la.switch_prob(cm, chrom, 0.0)
    with pytest.raises(RuntimeError, match="grid must be > 0"):
        la.output_points(cm, chrom, 0.0)
    with pytest.raises(RuntimeError, match="not a number"):
        la.switch_prob(np.asarray([0.0, np.nan]), np.zeros(2), 5.0)
    assert la.block_rows(7200, 8) == (1 << 30) // (144 * 7200) // 256 * 256 and la.block_rows(7200, 8, 1) == 256
    assert la.pair_table(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def test_the_wrapper_checks_the_device_lists_on_the_host():
    from neural_admixture_amd import localanc as la
    seg, out, oseg = la.check_layout(10, [0, 4, 10], [0, 3, 4, 9], [0, 2, 4])
    assert all(a.dtype == np.int32 for a in (seg, out, oseg)) and out.tolist() == [0, 3, 4, 9]
    assert la.check_layout(10, [0, 4, 4, 10]) [1] is None     # an empty segment, no output points
    for args, msg in ((([0],), "at least one segment"), (([0, 11],), r"ascending within 0\.\.10"), (([3, 2, 10],), "ascending within"),
                      (([-1, 10],), "ascending within"), (([0, 10], [1, 1], [0, 2]), "out_snp must be strictly ascending"),
                      (([0, 10], [2, 1], [0, 2]), "strictly ascending"), (([0, 10], [1, 2], None), "go together"),
                      (([0, 4, 10], [1, 2], [0, 2]), "oseg must ascend from 0 to 2 with one entry per bound"),
                      (([0, 4, 10], [1, 2], [0, 1, 3]), "oseg must ascend"), (([0, 4, 10], [1, 2], [1, 1, 2]), "oseg must ascend"),
                      (([0, 4, 10], [1, 2], [0, 2, 1]), "oseg must ascend"),
                      (([0, 4, 10], [1, 4], [0, 2, 2]), r"segment 0 is \[0, 4\) but its output points run from 1 to 4"),
                      (([0, 4, 10], [3, 5], [0, 0, 2]), r"segment 1 is \[4, 10\) but its output points run from 3 to 5"),
                      (([0, 4, 10], [5, 10], [0, 0, 2]), r"segment 1 is \[4, 10\)")):
        with pytest.raises(RuntimeError, match=msg):
            la.check_layout(10, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        la.local_ancestry(torch.zeros((4, 16), dtype=torch.uint8), 40, np.full((40, 2), 0.5), np.full((4, 2), 0.5), np.arange(40.0), np.zeros(40), 5.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        la.loglik(torch.zeros((4, 16), dtype=torch.uint8), 40, np.full((40, 2), 0.5), np.full((4, 2), 0.5), np.arange(40.0), np.zeros(40), 5.0)


def test_tracts_the_deviation_scan_and_the_writers(tmp_path):
    from neural_admixture_amd import localanc as la
    call = np.asarray([[0, 0, 1, 1, 2, 2], [3, 3, 255, 3, 3, 4]], dtype=np.uint8)
    out, oseg, cm = np.asarray([0, 2, 4, 5, 7, 9], np.int32), np.asarray([0, 4, 6], np.int32), np.arange(10.0)
    sw, tract = la.tracts(call, out, oseg, cm)
    assert sw.tolist() == [1, 1]                             # (0 0 1 1 | 2 2) and (3 3 . 3 | 3 4): chromosomes apart, the gap skipped
    assert np.allclose(tract, 2.0 * (5.0 + 2.0) / (1 + 4))
    ps = np.asarray([[0.2, 0.8], [0.4, 0.6], [0.6, 0.4], [0.2, 0.8], [0.4, 0.6], [0.6, 0.4]])
    dev = la.point_deviation(ps)
    assert np.allclose(dev[:, 0], (ps[:, 0] - 0.4) / ps[:, 0].std()) and np.allclose(dev[:, 0], -dev[:, 1])
    assert np.isnan(la.point_deviation(np.full((4, 2), 0.5))).all()
    Q = np.asarray([[0.5, 0.3, 0.2], [0.1, 0.1, 0.8]])
    share = np.asarray([[0.52, 0.3, 0.18], [0.2, 0.1, 0.7]])
    res = la.LocalAncestry(call, np.full((2, 6), 0.9, np.float32), np.asarray([[-10.0, -5.0], [-7.0, -1.0]]), share, np.hstack([ps, ps[:, :1]]) / 1.2, 1,
                           np.zeros((2, 6, 3), np.float32), out, oseg, [(0, 5), (5, 10)], 20.0)
    la.write_results(str(tmp_path), "run", 3, res, Q, cm, ["1"] * 5 + ["2"] * 5, [f"rs{j}" for j in range(10)], 100 * np.arange(10))
    rows = (tmp_path / "run.3.lanc").read_text().splitlines()
    assert rows[0] == "1 rs0 0 0 1/1 2/2" and rows[2] == "1 rs4 400 4 1/2 ./." and rows[5] == "2 rs9 900 9 1/3 2/3" and len(rows) == 6
    rows = (tmp_path / "run.3.lanc.sample").read_text().splitlines()
    assert rows[0] == "loglik local1 Q1 local2 Q2 local3 Q3 switches tract_cM"
    assert rows[1].split() == ["-1.500000000e+01", "0.52", "0.5", "0.3", "0.3", "0.18", "0.2", "1", "2.8"] and len(rows) == 3
    rows = (tmp_path / "run.3.lanc.mean").read_text().splitlines()
    assert rows[0].split()[:6] == ["chrom", "snp_id", "bp", "cM", "share1", "dev1"] and len(rows) == 7 and rows[1].split()[:4] == ["1", "rs0", "0", "0"]
    assert np.load(tmp_path / "run.3.lanc.dosage.npy").shape == (2, 6, 3)
    # a sample far from its Q, among others that sit on theirs
    share = np.tile([0.5, 0.5], (20, 1)) + 0.001
    share[7] = [0.8, 0.2]
    assert la.far_from_q(share, np.tile([0.5, 0.5], (20, 1))).tolist() == [7]
    assert la.far_from_q(np.tile([0.5, 0.5], (20, 1)) + 0.001, np.tile([0.5, 0.5], (20, 1))).tolist() == []


def test_cli_local_refuses_before_the_gpu_check(tmp_path, monkeypatch):
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["local", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    assert "local" in cli._ANALYSIS_MODES

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    k3 = ["--k", "3"]
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    for extra, msg in ((["--generations", "0"], r"--generations takes a number > 0 or auto"), (["--generations", "x"], r"--generations takes a number"),
                       (["--grid", "0"], r"--grid must be > 0"), (["--rate", "0"], r"--rate must be > 0"),
                       (["--scan_samples", "0"], r"--scan_samples must be >= 1"), (["--warn", "0"], r"--warn must be > 0"),
                       (["--target", "A"], r"--target names a label of --pops_path"),
                       (["--pops_path", str(tmp_path / "nopops")], r"nopops not found")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + k3 + extra)
    with pytest.raises(SystemExit, match=r"local ancestry is available for K <= 16"):
        cli.main(base + ["--k", "17"])
    with pytest.raises(SystemExit, match=r"not available for VCF input"):
        cli.main(base[:-1] + [str(tmp_path / "x.vcf")] + k3)
    with pytest.raises(SystemExit, match=r"local needs the .*run\.3\.P not found"):
        cli.main(base + k3)
    np.savetxt(tmp_path / "run.3.P", np.full((6, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"x\.bim not found"):
        cli.main(base + k3)
    (tmp_path / "x.fam").write_text("".join(f"f s{i} 0 0 0 -9\n" for i in range(5)))
    bed.write_bytes(bytes(3 + 2 * 6))                        # N = 5, M = 6
    (tmp_path / "x.bim").write_text("".join(f"1 rs{j} {c} {1000 * j} A G\n" for j, c in enumerate((0.0, 0.1, 0.3, 0.2, 0.4, 0.5))))
    with pytest.raises(SystemExit, match=r"x\.bim: output_points: the genetic map decreases within a chromosome at SNP 3 "):
        cli.main(base + k3)
    (tmp_path / "x.bim").write_text("".join(f"1 rs{j} {0.1 * j} {1000 * j} A G\n" for j in range(6)))
    (tmp_path / "pops").write_text("A\nB\nA\nB\n")
    with pytest.raises(SystemExit, match=r"--target C: no sample"):
        cli.main(base + k3 + ["--pops_path", str(tmp_path / "pops"), "--target", "C"])
    with pytest.raises(SystemExit, match=r"pops lists 4 labels, the data holds 5 samples"):
        cli.main(base + k3 + ["--pops_path", str(tmp_path / "pops"), "--target", "A"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + k3 + ["--generations", "12.5"])


def test_sharded_and_cpu_engines_refuse_local_ancestry():
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.local_ancestry is single-GPU"):
        e.local_ancestry(np.zeros(4), np.zeros(4))
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.local_ancestry needs the HIP engine with its packed matrix resident"):
        e.local_ancestry(np.zeros(4), np.zeros(4))


def test_no_kernel_of_the_unit_spills():
    """The states of a sample live in registers: the resource-usage remarks of the unit's compile report a scratch size of 0 bytes per
    lane for every kernel it ships (two kernels at each of the four widths)."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "nadm_local_anc.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(sizes) == 8 and sum("local_anc_fwd" in n for n in names) == 4 and sum("local_anc_bwd" in n for n in names) == 4
    assert sizes == [0] * 8, dict(zip(names, sizes))
