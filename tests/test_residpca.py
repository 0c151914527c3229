"""Residual PCA given Q and P (nadm_resid_project / nadm_resid_project_t, residpca.resid_pca, Engine.resid_pca, the `residpca` mode of
the command line).  The float64 numpy restatement and the shared data live in tests/residpca_oracle.py.

THE PRODUCTS' TOLERANCE is measured, then fixed: |out - out64| <= TOL x (sum of |a64||w| over the terms of that output), a the
standardised residual in float64.  What enters is the fp32 error of a itself -- pi carries up to K roundings of 2^-24, g - 2 pi
cancels where g = 1 and pi is near 1/2, the reciprocal square root is 1 ulp -- and that of the fp32 sums (at most one 256-SNP chunk
or one slice of 64-sample tiles per running sum at these shapes, then float64).  The rule: the largest ratio over CASES against the
float64 oracle, times 4, rounded up to a power of two, and never above 2^-15 (tests/test_pca.py's bound).
CONDITIONING: the error of a is ABSOLUTE, about 2 |d pi| / sqrt(2 r u) = 3e-7, not relative to |a|: g - 2 pi cancels where g = 1 and pi
is near 1/2.  An output that is a sum of many terms does not see that; an output of ONE term -- the transposed product at b = 1 -- holds
a itself to a relative error, which no fp32 pi meets at any TOL (a64 may be as close to 0 as it likes).  b = 1 with K = 16, M = 1027 was
run once and gave 3.5e-5 = 2^-14.8 on the transposed product (the forward one 2.6e-8); so b = 1 is paired with K = 1, where pi = p is exact,
and K = 16 runs at b = 200 and b = 4300.
MEASURED on an MI355X (each case prints its ratios): the largest ratio over CASES is 2.5e-7 = 2^-21.9 (forward 4.0e-10 ..
1.9e-7, transposed 1.7e-8 .. 2.5e-7), so TOL = 2^-19 = 1.9e-6; ss within 6.8e-7 relative (allowed 1e-5); see DESIGN.md section 4.19.

THE END-TO-END BOUNDS are the issue's: on panel_merged(0, rounds=100) the top eigenvalue within 1e-6 relative of the float64
restatement with the same Omega and 1 - |cos| <= 1e-10 (fp32 numpy products reach 9e-9 and 4e-15 there; the test prints both)."""
import functools
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_oracle as LO  # noqa: E402
import pca_oracle as PO  # noqa: E402
import residpca_oracle as RO  # noqa: E402
from packed_rows import case_rows, dev as _dev, packed as _packed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.0 ** -19
CAP = 2.0 ** -15
RESIDENT = 200
# (b, M, K, C): every b, M, K and C of the issue at least once, not their product, and every padded width (K = 7 -> 8, 10 -> 12);
# 4300 > 4096 rows drawn with repeats from the 200 resident ones; M = 1027 is five one-chunk ranges of the forward product.  b = 1 goes
# with K = 1 (module docstring: a one-term output holds a itself to a RELATIVE error, which an fp32 pi cannot give where g = 2 pi)
CASES = [(1, 255, 1, 1), (65, 1027, 3, 8), (200, 1027, 16, 20), (4300, 1027, 3, 20), (200, 255, 16, 8), (65, 255, 3, 20), (1, 1027, 1, 8),
         (65, 1027, 7, 20), (200, 255, 10, 1), (4300, 255, 16, 8)]
NEW = ["nadm_resid_project_chunks", "nadm_resid_project_ranges", "nadm_resid_project_scratch_floats", "nadm_resid_project",
       "nadm_resid_project_t_slices", "nadm_resid_project_t_scratch_floats", "nadm_resid_project_t"]


def _lib():
    from neural_admixture_amd._lib import lib, EXPORTS
    return lib, EXPORTS


def _cp(c):
    return 16 if c <= 16 else 32


# ================================================================================================ CPU: the oracle
def test_oracle_by_hand():
    """3 samples x 4 SNPs, K = 1 (q = 1, pi_ij = p_j), pimin = 0.01, eps = 1e-6:
         G = 0 1 2 3      p = 0.5, 0.2, 0.005, 0 (clipped to eps)
             1 3 2 0      SNP0: sqrt(2 r u) = sqrt(0.5): a = (0 - 1, 1 - 1, 2 - 1) / sqrt(0.5) = -sqrt2, 0, sqrt2
             2 0 1 1      SNP1: sqrt(0.32): a = (1 - 0.4) / sqrt(0.32), missing -> 0, (0 - 0.4) / sqrt(0.32)
                          SNP2: pi = 0.005 < pimin: every call masked
    with pimin = 0 the SNPs 2 and 3 enter: SNP2 a = (g - 0.01) / sqrt(2 x 0.005 x 0.995); SNP3: pi = 0 clips to r = eps, u = 1 - eps
    (from the UNCLIPPED 1 - pi = 1): a = g / sqrt(2 eps (1 - eps)), the missing call of sample 0 gives 0."""
    G = np.asarray([[0, 1, 2, 3], [1, 3, 2, 0], [2, 0, 1, 1]], dtype=np.uint8)
    P = np.asarray([[0.5], [0.2], [0.005], [0.0]], dtype=np.float32)
    Q = np.ones((3, 1), dtype=np.float32)
    p1, p2 = float(np.float32(0.2)), float(np.float32(0.005))
    a, m = RO.resid(G, P, Q, pimin=0.01)
    s0, s1 = np.sqrt(0.5), np.sqrt(2 * p1 * (1 - p1))
    want = np.asarray([[-1 / s0, (1 - 2 * p1) / s1, 0, 0], [0, 0, 0, 0], [1 / s0, -2 * p1 / s1, 0, 0]])
    assert np.allclose(a, want, rtol=1e-15, atol=1e-15)
    assert m.tolist() == [[True, True, False, False], [True, False, False, False], [True, True, False, False]]
    assert RO.summary(a, m)[:2] == (2, 3)                                           # M_eff, N_eff
    Y, mag, ss, nobs = RO.project(G, P, Q, np.asarray([[1.0], [-2.0], [5.0], [7.0]]), pimin=0.01)
    assert np.allclose(Y[:, 0], want @ [1.0, -2.0, 5.0, 7.0]) and np.allclose(mag[:, 0], np.abs(want) @ [1.0, 2.0, 5.0, 7.0])
    assert np.allclose(ss, (want ** 2).sum(axis=1)) and nobs.tolist() == [2, 1, 2]
    O, magt, nsnp = RO.project_t(G, P, Q, np.asarray([[1.0], [3.0], [-1.0]]), pimin=0.01)
    assert np.allclose(O[:, 0], want.T @ [1.0, 3.0, -1.0]) and nsnp.tolist() == [3, 2, 0, 0]
    a0, m0 = RO.resid(G, P, Q, pimin=0.0, near=None)
    e = float(np.float32(1e-6))
    s2, s3 = np.sqrt(2 * p2 * (1 - p2)), np.sqrt(2 * e * float(np.float32(1.0) - np.float32(1e-6)))
    assert np.allclose(a0[:, 2], [(2 - 2 * p2) / s2, (2 - 2 * p2) / s2, (1 - 2 * p2) / s2], rtol=1e-15)
    assert np.allclose(a0[:, 3], [0.0, 0.0, 1 / s3], rtol=1e-15) and m0[:, 3].tolist() == [False, True, True]
    assert abs(RO.edge(6.0, 3, 12) - 2.0 * (1 + 0.5) ** 2) < 1e-15
    with pytest.raises(AssertionError, match="within"):                              # a call at the mask's bound is refused by the oracle
        RO.resid(G, np.asarray([[0.5], [0.2], [0.01], [0.0]], dtype=np.float32), Q, pimin=0.01)


def test_shared_iteration_against_the_dense_eigh():
    """pca.subspace_pcs -- the function pca.pca and residpca.resid_pca both run -- with float64 numpy operators of the residual matrix
    of panel_merged(0, rounds=100), against eigh of the dense A A^T / M_eff: top eigenvalue to 1e-10 relative, 1 - |cos| to 1e-10 (the
    restatement shows 1e-14); the oracle's own restatement of it gives the same."""
    from neural_admixture_amd import pca
    G, P, Q, _ = RO.merged(0)
    a, m = RO.resid(G, P, Q, near=None)
    m_eff = RO.summary(a, m)[0]
    lam, U, *_ = RO.dense(G, P, Q)
    N, M = G.shape
    L, CP = 20, 32
    cpu = torch.device("cpu")

    def times(Wd):
        return a @ Wd[:, :L].numpy()

    def t_times(Qh):
        out = torch.zeros((M, CP), dtype=torch.float64)
        out[:, :Qh.shape[1]] = torch.from_numpy(a.T @ Qh)
        return out
    asked = []
    values, vectors = pca.subspace_pcs(times, t_times, M, L, CP, 10, 10, 42, cpu, lambda: asked.append(1) or m_eff)
    assert asked == [1] and values.shape == (10,) and vectors.shape == (N, 10)
    ev, ang = PO.pc_errors(values, vectors, lam, U, 1)
    r = RO.rsvd(G, P, Q)
    ev2, ang2 = PO.pc_errors(r["eigenvalues"], r["eigenvectors"], lam, U, 1)
    print(f"shared iteration vs dense eigh: eigenvalue {ev[0]:.3e}, 1 - |cos| {ang[0]:.3e}; the oracle's restatement {ev2[0]:.3e}, {ang2[0]:.3e}")
    assert ev[0] <= 1e-10 and ang[0] <= 1e-10 and ev2[0] <= 1e-10 and ang2[0] <= 1e-10
    assert np.allclose(values, r["eigenvalues"], rtol=1e-12) and (np.diff(values) <= 0).all()


def test_float64_calibration():
    """The values behind --warn 1.5, in float64 (96 x 6000, 100 block-EM rounds, pimin 0.01): where the model holds the top eigenvalue
    stays below 1.2 x the trace-normalised Marchenko-Pastur edge; four populations fitted with K = 3 give one eigenvalue above 2 x the
    edge and a second below 1.2 x, and PC1 is 0 on the two well-modelled populations and of opposite sign on the two merged ones."""
    for seed in range(5):
        G, P, Q, _ = RO.admixed(seed)
        lam, _, _, _, _, ed = RO.dense(G, P, Q)
        print(f"panel_admixed({seed}): top eigenvalue / edge {lam[0] / ed:.4f}")
        assert lam[0] / ed < 1.2
    for seed in range(3):
        G, P, Q, pop = RO.merged(seed)
        lam, U, _, _, _, ed = RO.dense(G, P, Q)
        means = [float(U[pop == k, 0].mean()) for k in range(4)]
        print(f"panel_merged({seed}): eigenvalues / edge {lam[0] / ed:.4f}, {lam[1] / ed:.4f}; PC1 group means " + ", ".join(f"{x:+.4f}" for x in means))
        assert lam[0] / ed > 2 and lam[1] / ed < 1.2
        assert abs(means[0]) < 0.01 and abs(means[1]) < 0.01
        assert means[2] * means[3] < 0 and abs(means[2]) > 0.1 and abs(means[3]) > 0.1


# ================================================================================================ CPU: symbols, refusals, queries
def test_symbols_are_declared_bound_and_exported():
    import neural_admixture_amd as na
    from neural_admixture_amd import residpca
    lib, EXPORTS = _lib()
    header = open(os.path.join(ROOT, "include", "nadm.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in EXPORTS and hasattr(lib, name)
    assert lib.nadm_abi_version() == 14
    assert na.residpca is residpca and na.resid_pca is residpca.resid_pca and na.resid_project is residpca.resid_project
    assert na.resid_project_t is residpca.resid_project_t
    assert {"residpca", "resid_pca", "resid_project", "resid_project_t"} <= set(na.__all__)


def _refused(status, pattern):
    lib, _ = _lib()
    msg = lib.nadm_last_error().decode()
    assert status == 1 and re.search(pattern, msg), (status, msg)


def test_every_refusal_of_both_entries_comes_before_a_launch():
    """Every call below is refused (status 1 and the reason through nadm_last_error): none reaches a launch, so none needs a GPU.
    Pointers are made-up aligned addresses; nothing dereferences them."""
    lib, _ = _lib()
    A = 1 << 20                                              # an aligned made-up address

    def fwd(xp=A, ld=272, idx=None, b=8, M=1027, P=A, k=3, kp=4, Q=A, qs=4, eps=1e-6, pimin=0.01, W=A, c=8, cp=16, Y=A, ss=A, nobs=A, scr=A):
        return lib.nadm_resid_project(xp, ld, idx, b, M, P, k, kp, Q, qs, eps, pimin, W, c, cp, Y, ss, nobs, scr, None)

    def tr(xp=A, ld=272, idx=None, b=8, M=1027, P=A, k=3, kp=4, Q=A, qs=4, eps=1e-6, pimin=0.01, Yin=A, c=8, cp=16, O=A, nobs=A, scr=A):
        return lib.nadm_resid_project_t(xp, ld, idx, b, M, P, k, kp, Q, qs, eps, pimin, Yin, c, cp, O, nobs, scr, None)
    for f, ptrs, who in ((fwd, ("xp", "P", "Q", "W", "Y", "ss", "nobs", "scr"), "nadm_resid_project"),
                         (tr, ("xp", "P", "Q", "Yin", "O", "nobs", "scr"), "nadm_resid_project_t")):
        for p in ptrs:
            _refused(f(**{p: None}), who + ": null pointer")
        for kw in (dict(b=0), dict(b=-1), dict(M=0)):
            _refused(f(**kw), who + ": empty block")
        _refused(f(ld=256), who + r": ld < ceil\(M/4\)")
        for ld in (264, 1 << 32):
            _refused(f(ld=ld), who + ": ld must be a multiple of 16 and < 2\\^32")
        for kw in (dict(k=0), dict(k=65, kp=64, qs=64)):
            _refused(f(**kw), who + r": K must be in 1\.\.NADM_MAX_K")
        _refused(f(kp=8, qs=8), who + r": kp must be nadm_pad_k\(k\)")
        _refused(f(k=5, kp=8, qs=4), who + ": q_stride < kp")
        _refused(f(qs=6), who + ": q_stride must be a multiple of 4")
        for eps in (0.0, 0.5, float("nan")):
            _refused(f(eps=eps), who + r": eps must be in \[1e-9, 0.5\)")
        for pimin in (-0.01, 0.5, float("nan")):
            _refused(f(pimin=pimin), who + r": pimin must be in \[0, 0.5\)")
        _refused(f(k=17, kp=24, qs=24), who + ": K must be <= 16")
        for cp in (0, 8, 24, 64):
            _refused(f(cp=cp), who + ": CP must be 16 or 32")
        for kw in (dict(c=0), dict(c=17), dict(c=33, cp=32), dict(c=-1)):
            _refused(f(**kw), who + r": C must be in 1\.\.CP")
        _refused(f(xp=A + 8), who + ": xp must be 16-byte and idx 4-byte aligned")
        _refused(f(idx=A + 2), who + ": xp must be 16-byte and idx 4-byte aligned")
        for p in ptrs[1:]:
            _refused(f(**{p: A + (2 if p == "nobs" else 4)}), who + ": .* aligned")


def test_the_split_and_scratch_queries():
    """The split is a rule of the shape alone.  Forward: the plan of nadm_sample_info -- a running sum covers at most 1024 chunks =
    2^18 SNPs, the ranges cover every chunk.  Transposed: the slices of nadm_snp_hwe_slices (at most 4096 samples each).  The scratch
    sizes grow with b and with M and hold what the kernels write; a shape or a width without a kernel gives 0."""
    lib, _ = _lib()
    bs = [1, 63, 64, 65, 200, 256, 257, 4096, 4097, 4300, 32768, 100_000]
    Ms = [1, 255, 256, 257, 1027, 65_536, 600_000, 5_000_000, 300_000_000]
    for cp in (16, 32):
        prev_b = None
        for b in bs:
            row = []
            for M in Ms:
                chunks = (M + 255) // 256
                cpr, ranges = lib.nadm_resid_project_chunks(b, M), lib.nadm_resid_project_ranges(b, M)
                assert 1 <= cpr <= 1024 and ranges == (chunks + cpr - 1) // cpr == lib.nadm_sample_info_ranges(b, M)
                fs = lib.nadm_resid_project_scratch_floats(b, M, cp)
                assert fs >= ranges * ((b + 255) // 256) * 256 * (cp + 3)
                sl = lib.nadm_resid_project_t_slices(b, M)
                tiles = (b + 63) // 64
                assert sl == lib.nadm_snp_hwe_slices(b, M) and 1 <= sl <= tiles and (tiles + sl - 1) // sl <= 64
                ts = [lib.nadm_resid_project_t_scratch_floats(b, M, kp, cp) for kp in (4, 8, 12, 16)]
                assert all(t >= b * (kp + cp) + sl * chunks * 256 * (cp + 1) for t, kp in zip(ts, (4, 8, 12, 16)))
                assert ts == sorted(ts)
                row.append((fs, ts[-1]))
            assert all(a[0] <= c[0] and a[1] <= c[1] for a, c in zip(row, row[1:])), "not monotone in M"
            if prev_b is not None:
                assert all(a[0] <= c[0] and a[1] <= c[1] for a, c in zip(prev_b, row)), "not monotone in b"
            prev_b = row
    for b, M, cp in ((0, 10, 16), (10, 0, 16), (10, 10, 8), (10, 10, 64)):
        assert lib.nadm_resid_project_scratch_floats(b, M, cp) == 0 and lib.nadm_resid_project_t_scratch_floats(b, M, 4, cp) == 0
    for kp in (0, 6, 24):
        assert lib.nadm_resid_project_t_scratch_floats(10, 10, kp, 16) == 0
    assert lib.nadm_resid_project_ranges(0, 10) == 0 and lib.nadm_resid_project_chunks(10, 0) == 0 and lib.nadm_resid_project_t_slices(0, 10) == 0
    # the shapes the GPU cases use: one chunk per range, several ranges at M = 1027, more than one slice above 4096 rows
    for b, M, _, _ in CASES:
        assert lib.nadm_resid_project_chunks(b, M) == 1 and lib.nadm_resid_project_ranges(b, M) == (M + 255) // 256
    assert lib.nadm_resid_project_ranges(65, 1027) == 5 and lib.nadm_resid_project_t_slices(4300, 1027) > 1


def test_resid_pca_refuses_bad_arguments_without_a_gpu():
    """L = pcs + oversample > 32, a pimin outside [0, 0.5), non-positive counts and K > 16 are refused before the matrix is looked at
    (None stands in for it); a matrix that is not on a GPU is refused next."""
    from neural_admixture_amd import residpca
    P, Q = np.full((40, 3), 0.5, dtype=np.float32), np.full((4, 3), 1 / 3, dtype=np.float32)
    with pytest.raises(RuntimeError, match=r"resid_pca: pcs \+ oversample must be <= 32.*got 23 \+ 10"):
        residpca.resid_pca(None, 40, P, Q, pcs=23)
    assert residpca.check_args(22, 10, 10, 0.01) == 32
    for bad in (-0.01, 0.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"resid_pca: pimin must be in \[0, 0.5\)"):
            residpca.resid_pca(None, 40, P, Q, pimin=bad)
    with pytest.raises(RuntimeError, match="resid_pca: pcs must be >= 1"):
        residpca.resid_pca(None, 40, P, Q, pcs=0)
    with pytest.raises(RuntimeError, match="resid_pca: oversample must be >= 0"):
        residpca.resid_pca(None, 40, P, Q, oversample=-1)
    with pytest.raises(RuntimeError, match="resid_pca: iters must be >= 0"):
        residpca.resid_pca(None, 40, P, Q, iters=-1)
    wide = np.full((40, 17), 0.5, dtype=np.float32)
    for f, arg in ((residpca.resid_pca, ()), (residpca.resid_project, (None, 3)), (residpca.resid_project_t, (None, 3))):
        with pytest.raises(RuntimeError, match="K must be <= 16 for the residual PCA"):
            f(None, 40, wide, None, *arg)
    x = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residpca.resid_pca(x, 40, P, Q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residpca.resid_project(x, 40, P, Q, torch.zeros((40, 16)), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residpca.resid_project_t(x, 40, P, Q, torch.zeros((4, 16)), 3)
    assert abs(residpca.mp_edge(6.0, 3, 12) - 4.5) < 1e-15


def test_sharded_and_cpu_engines_refuse_resid_pca():
    """Engine.resid_pca is single-GPU and needs the resident matrix; the checks come first, so a stand-in without device state shows
    them; its own arguments are refused before either."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(RuntimeError, match=r"resid_pca: pcs \+ oversample must be <= 32"):
        e.resid_pca(pcs=30)
    with pytest.raises(NotImplementedError, match="Engine.resid_pca is single-GPU"):
        e.resid_pca()
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.resid_pca needs the HIP engine with its packed matrix resident"):
        e.resid_pca(pcs=3)


# ================================================================================================ CPU: the command line
def test_cli_residpca_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """The parser has the mode's flags; argument errors and missing or misshapen files end the run with the offender named, before
    the GPU check and before a genotype is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["residpca", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_residpca_args(base[1:] + ["--k", "3"])
    assert (a.pcs, a.oversample, a.iters, a.seed, a.pimin, a.pops_path, a.warn, a.out_name, a.extract, a.keep, a.remove) == \
        (10, 10, 10, 42, 0.01, None, 1.5, None, None, None, None)
    a = cli.parse_residpca_args(base[1:] + ["--min_k", "2", "--max_k", "4", "--pcs", "4", "--oversample", "6", "--iters", "3", "--seed", "7",
                                            "--pimin", "0.05", "--pops_path", "f", "--warn", "2", "--out_name", "o", "--extract", "g"])
    assert (a.min_k, a.max_k, a.pcs, a.oversample, a.iters, a.seed, a.pimin, a.pops_path, a.warn, a.out_name, a.extract) == \
        (2, 4, 4, 6, 3, 7, 0.05, "f", 2.0, "o", "g")
    assert "residpca" in cli._ANALYSIS_MODES

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="Please provide either --k or both --min_k and --max_k"):
        cli.main(base)
    for ks in (["--k", "17"], ["--min_k", "15", "--max_k", "17"]):
        with pytest.raises(SystemExit, match=r"residpca needs every K <= 16.*K = 17 was asked for"):
            cli.main(base + ks)
    with pytest.raises(SystemExit, match=r"pcs \+ oversample must be <= 32"):
        cli.main(base + ["--k", "3", "--pcs", "30"])
    with pytest.raises(SystemExit, match=r"pimin must be in \[0, 0.5\)"):
        cli.main(base + ["--k", "3", "--pimin", "0.5"])
    with pytest.raises(SystemExit, match="pcs must be >= 1"):
        cli.main(base + ["--k", "3", "--pcs", "0"])
    with pytest.raises(SystemExit, match="iters must be >= 0"):
        cli.main(base + ["--k", "3", "--iters", "-2"])
    for value in ("-0.1", "nan"):
        with pytest.raises(SystemExit, match=r"--warn must be >= 0"):
            cli.main(base + ["--k", "3", "--warn", value])
    with pytest.raises(SystemExit, match=r"nopops not found"):
        cli.main(base + ["--k", "3", "--pops_path", str(tmp_path / "nopops")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen"), "--k", "3"])
    with pytest.raises(SystemExit, match=r"residpca needs the .*run\.3\.P not found"):
        cli.main(base + ["--k", "3"])
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    bed.write_bytes(bytes(3 + 2 * 9))                        # N = 5, M = 9
    (tmp_path / "pops").write_text("a\nb\na\nb\n")          # four labels for five samples
    with pytest.raises(SystemExit, match=r"pops lists 4 labels, the data holds 5 samples"):
        cli.main(base + ["--k", "3", "--pops_path", str(tmp_path / "pops")])
    with pytest.raises(SystemExit, match=r"--pcs 6 components were asked of 5 samples"):
        cli.main(base + ["--k", "3", "--pcs", "6"])
    np.savetxt(tmp_path / "run.3.P", np.full((8, 3), 0.5))
    with pytest.raises(SystemExit, match=r"run\.3\.P"):
        cli.main(base + ["--k", "3", "--pcs", "4"])
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    (tmp_path / "pops").write_text("a\nb\na\nb\na\n")
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
        cli.main(base + ["--k", "3", "--pcs", "4", "--pops_path", str(tmp_path / "pops")])
    assert not list(tmp_path.glob("*.eigenval")) and not list(tmp_path.glob("*.eigenvec"))


def test_writer_and_log_lines_on_a_made_up_result(tmp_path, caplog):
    """{name}.{K}.resid.eigenval / .eigenvec in pca.write_result's layout, read back to the same float64; the log names every PC with
    its ratio, and for the one PC above the threshold the warning, the groups at its two ends and its five most extreme samples."""
    from neural_admixture_amd import pca, residpca
    rng = np.random.default_rng(3)
    vec = pca.orient(rng.standard_normal((8, 3)))
    vec[:, 0] = pca.orient(np.asarray([[0.5, 0.4, -0.5, -0.45, 0.01, 0.3, -0.2, 0.02]]).T)[:, 0]
    vals, edge = np.asarray([3.0, 1.0 / 3.0, 1e-9]), 1.25
    res = residpca.ResidPcaResult(3, vals, vec, 1234, 8, 7.5, edge, vals / edge)
    residpca.write_results(str(tmp_path / "out"), "o", [res])
    got = (tmp_path / "out" / "o.3.resid.eigenval").read_text().splitlines()
    assert len(got) == 3 and [float(v) for v in got] == vals.tolist()
    rows = [ln.split() for ln in (tmp_path / "out" / "o.3.resid.eigenvec").read_text().splitlines()]
    assert len(rows) == 8 and all(len(r) == 5 for r in rows) and [r[:2] for r in rows] == [[str(i), str(i)] for i in range(8)]
    assert np.array_equal(np.asarray([[float(x) for x in r[2:]] for r in rows]), vec)
    caplog.set_level(logging.INFO)
    labels = ["a", "a", "b", "b", "c", "a", "b", "c"]
    residpca.log_results([res], [labels], logging.getLogger("residpca"), warn=1.5)
    msgs = [r.getMessage() for r in caplog.records]
    assert any("Residual PCA (K=3): 8 samples x 1234 SNPs" in m and "edge 1.25" in m for m in msgs)
    assert any("PC1: eigenvalue 3, 2.400 x the edge" in m for m in msgs) and sum(bool(re.search(r"PC\d: eigenvalue", m)) for m in msgs) == 3
    warns = [m for m in msgs if "Warning" in m]
    assert len(warns) == 1 and "residual PC1 is 2.40 x the edge" in warns[0] and "Try K = 4" in warns[0] and "'fit' mode" in warns[0]
    n0 = float(np.linalg.norm([0.5, 0.4, -0.5, -0.45, 0.01, 0.3, -0.2, 0.02]))
    assert any(f"groups at the two ends of PC1: a (mean score {0.4 / n0:+.4f}, 3 samples) and b (mean score {-1.15 / 3 / n0:+.4f}, 3 samples)" in m
               for m in msgs)
    assert any("samples with the largest |score| on PC1" in m and re.search(r": 0: \+0\.\d+, 2: -0\.\d+, 3: -0\.\d+, 1: \+0\.\d+, 5: \+0\.\d+$", m)
               for m in msgs)
    caplog.clear()
    residpca.log_results([res], [labels], logging.getLogger("residpca"), warn=2.5)
    assert not any("Warning" in r.getMessage() for r in caplog.records)


# ================================================================================================ GPU: the two products
def _operands(b, M, c, seed):
    """W [M, CP] and Yin [b, CP] float32 on the host: standard normals in the c columns in use, pad columns 0."""
    rng = np.random.default_rng(seed)
    cp = _cp(c)
    out = []
    for rows in (M, b):
        a = np.zeros((rows, cp), dtype=np.float32)
        a[:, :c] = rng.standard_normal((rows, c)).astype(np.float32)
        out.append(a)
    return out


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run_fwd(xp, M, P, Q, rows, W, c):
    from neural_admixture_amd import residpca
    Y, ss, n = residpca.resid_project(xp, M, P, Q, _to(W), c, None if rows is None else _to(rows))
    torch.cuda.synchronize()
    return Y.cpu().numpy(), ss.cpu().numpy(), n.cpu().numpy()


def _run_t(xp, M, P, Q, rows, Yin, c):
    from neural_admixture_amd import residpca
    O, n = residpca.resid_project_t(xp, M, P, Q, _to(Yin), c, None if rows is None else _to(rows))
    torch.cuda.synchronize()
    return O.cpu().numpy(), n.cpu().numpy()


def _check(got, want, mag, c, what):
    """|got - want| <= TOL mag per output, exactly +0.0 where mag is 0, pad columns +0.0 in every bit; prints the largest ratio before
    it asserts."""
    err = np.abs(got[:, :c].astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(mag > 0, err / mag, 0.0)))
    print(f"{what}: max |out - out64| / sum|a||w| = {ratio:.3e} (2^{np.log2(max(ratio, 1e-300)):.1f}); bound 2^{np.log2(TOL):.0f} = {TOL:.3e}")
    assert TOL <= CAP and np.isfinite(got).all()
    assert (err <= TOL * mag).all()
    zero = got[:, :c][mag == 0]
    assert zero.tobytes() == bytes(zero.nbytes) and got[:, c:].tobytes() == bytes(got[:, c:].nbytes)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K, c", CASES)
def test_products_against_float64(b, M, K, c):
    """Both products on a gather list with a duplicate and the all-missing row 4 (b = 1: row 7; b = 4300: drawn with repeats from the
    200 resident rows, so that the transposed product takes more than one slice), dirty padding, pimin = 0.01, against float64 within
    TOL x sum |a||w| (module docstring).  The counts are equal, ss within 1e-5 relative; the all-missing row's Y and the O rows of the
    SNPs nobody observed or pimin masks are +0.0 in every bit."""
    lib, _ = _lib()
    G, P, Q = RO.product_panel(M, K)
    xp = _packed(G, dirty=True).to(_dev())
    rows = case_rows(b, "list", RESIDENT)
    Gr, Qr = G[rows], Q[rows]
    W, Yin = _operands(b, M, c, 1000 * b + M + 10 * K + c)
    assert lib.nadm_resid_project_chunks(b, M) == 1
    if M > 256:
        assert lib.nadm_resid_project_ranges(b, M) > 1
    if b > 4096:
        assert lib.nadm_resid_project_t_slices(b, M) > 1
    Y, ss, n = _run_fwd(xp, M, P, Qr, rows, W, c)
    want, mag, ss64, n64 = RO.project(Gr, P, Qr, W[:, :c])
    _check(Y, want, mag, c, f"resid_project b={b} M={M} K={K} C={c}")
    assert np.array_equal(n, n64) and n.dtype == np.int32
    rel = float(np.max(np.abs(ss - ss64) / np.where(ss64 > 0, ss64, 1.0)))
    print(f"resid_project b={b} M={M} K={K} C={c}: ss within {rel:.3e} relative (allowed 1e-5)")
    assert rel <= 1e-5 and not ss[ss64 == 0].any()
    if b > 1:
        gone = rows == RO.ALL_MISSING_ROW
        assert gone.any() and Y[gone].tobytes() == bytes(Y[gone].nbytes) and not n[gone].any() and not ss[gone].any()
        assert np.array_equal(Y[0], Y[-1]) or b > RESIDENT           # (the list's last entry repeats its first)
    O, ns = _run_t(xp, M, P, Qr, rows, Yin, c)
    wt, magt, ns64 = RO.project_t(Gr, P, Qr, Yin[:, :c])
    _check(O, wt, magt, c, f"resid_project_t b={b} M={M} K={K} C={c}")
    assert np.array_equal(ns, ns64) and ns.dtype == np.int32
    masked = RO.masked_snps(M)
    assert not ns[masked].any() and O[masked].tobytes() == bytes(O[masked].nbytes) and np.abs(O).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 20])
def test_bit_identities(c):
    """b = 65, M = 1027 (a ragged last chunk and a partial last byte), CP = 16 and 32: two calls give the same bits; dirty and clean
    padding give the same bits; other finite values in the W rows of the SNPs nobody observed (3) or pimin masks (21, 1001) leave Y as
    it is bit for bit."""
    b, M, K = 65, 1027, 3
    G, P, Q = RO.product_panel(M, K)
    rows = case_rows(b, "list", RESIDENT)
    Qr = Q[rows]
    W, Yin = _operands(b, M, c, 5)
    dirty, clean = _packed(G, dirty=True).to(_dev()), _packed(G).to(_dev())
    assert not torch.equal(dirty, clean)
    F = _run_fwd(dirty, M, P, Qr, rows, W, c)
    T = _run_t(dirty, M, P, Qr, rows, Yin, c)
    assert np.abs(F[0]).max() > 1 and np.abs(T[0]).max() > 1
    for again in (_run_fwd(dirty, M, P, Qr, rows, W, c), _run_fwd(clean, M, P, Qr, rows, W, c)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, F))
    for again in (_run_t(dirty, M, P, Qr, rows, Yin, c), _run_t(clean, M, P, Qr, rows, Yin, c)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, T))
    V = W.copy()
    for j in RO.masked_snps(M):
        V[j, :c] = 1e6 * (1 + np.arange(c)) * (-1) ** j
    assert not np.array_equal(V, W)
    assert _run_fwd(dirty, M, P, Qr, rows, V, c)[0].tobytes() == F[0].tobytes()


# ------------------------------------------------------------------------------------------------ placement (tests/test_placement.py's two contracts)
PK, PC = 3, 20


@functools.lru_cache(maxsize=None)
def _placement_compact():
    import test_placement as TP
    return TP._pack(np.ascontiguousarray(RO.product_panel(TP.M, PK)[0][:TP.ROWS]))


def _placement_case(name, mode):
    """(operands on the host without the matrix, the genotypes of the case's rows in call order)."""
    import test_placement as TP
    rows = TP._rows("wide", mode)
    G, P, Q = RO.product_panel(TP.M, PK)
    W, Yin = _operands(len(rows), TP.M, PC, 77 + len(rows))
    x = {"P": P, "Q": np.ascontiguousarray(Q[rows])}
    x.update({"W": W} if name == "fwd" else {"Y": Yin})
    if mode == "list":
        x["idx"] = rows.copy()
    return x, G[:TP.ROWS][rows]


def _op_fwd(t):
    import test_placement as TP
    from neural_admixture_amd import residpca
    return residpca.resid_project(t["xp"], TP.M, t["P"], t["Q"], t["W"], PC, t.get("idx"))


def _op_t(t):
    import test_placement as TP
    from neural_admixture_amd import residpca
    return residpca.resid_project_t(t["xp"], TP.M, t["P"], t["Q"], t["Y"], PC, t.get("idx"))


PLACED = {"fwd": _op_fwd, "t": _op_t}


def _placement_check(name, got, Gr, x):
    if name == "fwd":
        want, mag, ss64, n64 = RO.project(Gr, x["P"], x["Q"], x["W"][:, :PC])
        _check(got[0], want, mag, PC, "resid_project (compact)")
        assert np.array_equal(got[2], n64) and np.allclose(got[1], ss64, rtol=1e-5, atol=0)
    else:
        want, mag, n64 = RO.project_t(Gr, x["P"], x["Q"], x["Y"][:, :PC])
        _check(got[0], want, mag, PC, "resid_project_t (compact)")
        assert np.array_equal(got[1], n64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLACED))
def test_stride_rows_past_4_gib(name):
    """tests/test_placement.py part A for the two new entries: 136 rows at ld = 2^25 (rows 64.. start beyond 2^31 bytes, rows 128..
    beyond 2^32, the slack next to the data all set bits) give the bits of the compact rows, with a gather list (130 rows out of
    order, a duplicate) and without one; the compact result is held to float64 first.  Its arena, placements and helpers are used as
    they are."""
    import test_placement as TP
    compact = _placement_compact()
    for mode in ("list", "none"):
        x, Gr = _placement_case(name, mode)
        t = dict(TP._to_dev(x), xp=compact.to(_dev()))
        want = TP._taken(PLACED[name](t))
        torch.cuda.synchronize()
        _placement_check(name, tuple(w.cpu().numpy() for w in want), Gr, x)
        xp = TP._placed("wide", compact)
        assert xp.shape == (TP.ROWS, TP.WIDE_LD)
        got = TP._taken(PLACED[name](dict(TP._to_dev(x), xp=xp)))
        torch.cuda.synchronize()
        TP._assert_same_bits(got, want, f"resid_project {name} wide rows={mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLACED))
def test_side_stream(name):
    """tests/test_placement.py part B for the two new entries: behind a delay on a side stream, with operands that hold decoys until
    copies behind the delay make them true, the call gives the bits of the default stream (its protocol, used as it is)."""
    import test_placement as TP
    x, _ = _placement_case(name, "list")
    true = dict(TP._to_dev(x), xp=_placement_compact().to(_dev()))
    want = TP._taken(PLACED[name](true))
    torch.cuda.synchronize()
    got = TP._on_side_stream(PLACED[name], true, f"resid_project {name}")
    TP._assert_same_bits(got, want, f"resid_project {name} on a side stream")


@pytest.mark.gpu
def test_the_arena_is_released():
    """After the placement tests of this module: the 4.25 GiB buffer goes back to the device (tests/test_placement.py takes its own)."""
    import test_placement as TP
    TP._ARENA.update(kind=None, buf=None)
    torch.cuda.empty_cache()


# ================================================================================================ GPU: end to end
@functools.lru_cache(maxsize=None)
def _gpu(panel):
    from neural_admixture_amd import residpca
    G, P, Q, _ = getattr(RO, panel)(0)
    res = residpca.resid_pca(_packed(G, dirty=True).to(_dev()), G.shape[1], P, Q)
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
def test_resid_pca_against_the_float64_restatement():
    """resid_pca() with its defaults on panel_merged(0, rounds=100) against the float64 restatement with the same Omega: the top
    eigenvalue within 1e-6 relative and 1 - |cos| <= 1e-10 (the fp32-numpy restatement's figures are printed next to the GPU's);
    M_eff and N_eff equal, total and edge within 1e-6; one eigenvalue above 2 x the edge and the second below 1.2 x; eigenvectors
    orthonormal and oriented.  On panel_admixed(0, rounds=100), where the model holds, the top eigenvalue stays below 1.2 x the edge."""
    G, P, Q, pop = RO.merged(0)
    want = RO.rsvd(G, P, Q, near=RO.NEAR_FIT)
    w32 = RO.rsvd(G, P, Q, dtype=np.float32)
    e32, a32 = PO.pc_errors(w32["eigenvalues"], w32["eigenvectors"], want["eigenvalues"], want["eigenvectors"], 1)
    res = _gpu("merged")
    ev, ang = PO.pc_errors(res.eigenvalues, res.eigenvectors, want["eigenvalues"], want["eigenvectors"], 1)
    print(f"fp32 numpy vs float64: eigenvalue {e32[0]:.3e}, 1 - |cos| {a32[0]:.3e};  GPU vs float64: eigenvalue {ev[0]:.3e}, 1 - |cos| {ang[0]:.3e}")
    assert ev[0] <= 1e-6 and ang[0] <= 1e-10
    assert res.K == 3 and res.M_eff == want["M_eff"] and res.N_eff == want["N_eff"] == G.shape[0]
    assert abs(res.total - want["total"]) <= 1e-6 * want["total"] and abs(res.edge - want["edge"]) <= 1e-6 * want["edge"]
    assert res.eigenvalues.shape == (10,) and res.eigenvectors.shape == (G.shape[0], 10) and res.ratio.shape == (10,)
    assert np.allclose(res.ratio, res.eigenvalues / res.edge, rtol=1e-14)
    print(f"panel_merged(0): ratios {res.ratio[0]:.4f}, {res.ratio[1]:.4f}")
    assert res.ratio[0] > 2 and res.ratio[1] < 1.2
    U = res.eigenvectors
    assert np.abs(U.T @ U - np.eye(U.shape[1])).max() <= 1e-5
    assert (U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])] > 0).all()
    assert (np.diff(res.eigenvalues) <= 0).all() and (res.eigenvalues > 0).all()
    means = [float(U[pop == k, 0].mean()) for k in range(4)]
    assert abs(means[0]) < 0.01 and abs(means[1]) < 0.01 and means[2] * means[3] < 0 and min(abs(means[2]), abs(means[3])) > 0.1
    Ga, Pa, Qa, _ = RO.admixed(0)
    wa = RO.rsvd(Ga, Pa, Qa, near=RO.NEAR_FIT)
    ra = _gpu("admixed")
    print(f"panel_admixed(0): ratio {ra.ratio[0]:.4f} (float64 {wa['ratio'][0]:.4f})")
    assert ra.ratio[0] < 1.2 and ra.M_eff == wa["M_eff"] and abs(ra.edge - wa["edge"]) <= 1e-6 * wa["edge"]


@pytest.mark.gpu
def test_a_row_without_a_call_gets_zeros_and_idx_equals_the_subsets_own_matrix():
    """A gather list of 60 rows in ascending order against the run on a matrix that holds only those rows; a sample whose every call
    is missing counts in neither N_eff nor the edge and gets eigenvector entries 0."""
    from neural_admixture_amd import residpca
    G, P, Q, _ = RO.merged(0)
    G = G.copy()
    G[10] = 3
    M = G.shape[1]
    pick = np.sort(np.random.default_rng(2).choice(G.shape[0], size=60, replace=False)).astype(np.int32)
    pick = np.sort(np.union1d(pick[pick != 10][:59], [10])).astype(np.int32)
    kw = dict(pcs=4, oversample=6)
    a = residpca.resid_pca(_packed(G).to(_dev()), M, P, Q[pick], idx=pick, **kw)
    b = residpca.resid_pca(_packed(np.ascontiguousarray(G[pick])).to(_dev()), M, P, Q[pick], **kw)
    assert a.M_eff == b.M_eff and a.N_eff == b.N_eff == len(pick) - 1 and a.eigenvectors.shape == (60, 4)
    assert np.array_equal(a.eigenvalues, b.eigenvalues) and np.array_equal(a.eigenvectors, b.eigenvectors) and a.edge == b.edge
    row = int(np.flatnonzero(pick == 10)[0])
    assert not a.eigenvectors[row].any() and (np.abs(np.delete(a.eigenvectors, row, axis=0)).max(axis=1) > 0).all()
    want = RO.rsvd(G[pick], P, Q[pick], **kw)
    assert a.N_eff == want["N_eff"] and np.allclose(a.eigenvalues[:1], want["eigenvalues"][:1], rtol=1e-5)


@pytest.mark.gpu
def test_engine_and_command_line_give_the_functions_numbers(tmp_path, caplog):
    """Engine.resid_pca on the engine's resident matrix with its own P and final Q, and the `residpca` mode on small BED files
    written here, equal residpca.resid_pca on the same packed rows and matrices; both files are well formed and read back to the
    returned numbers; the warning is logged on panel_merged and not on panel_admixed."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli, residpca
    from neural_admixture_amd.io import read_bed_packed
    from oracle import nadm_oracle as O
    dev = _dev()
    Gm, Pm, Qm, pop = RO.merged(0, 64, 2000)
    N, M = Gm.shape
    kw = dict(pcs=4, oversample=6, iters=5, pimin=0.02, seed=3)
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32)
    p = O.make_params(42, V0, np.ascontiguousarray(Pm.T.astype(np.float32)), 64, [3])
    e = na.Engine(M, 8, 64, [3], dev, N)
    e.load_params(V0, np.ascontiguousarray(Pm.T.astype(np.float32)), np.concatenate([p.g, p.W1.reshape(-1), p.b1, p.Wk[0].reshape(-1), p.bk[0]]))
    e.pack_from_host(torch.from_numpy(np.ascontiguousarray(Gm)))
    got = e.resid_pca(head=0, **kw)
    want = residpca.resid_pca(e.xp, M, *e._fitted(0), **kw)
    assert got.M_eff == want.M_eff and np.array_equal(got.eigenvalues, want.eigenvalues) and np.array_equal(got.eigenvectors, want.eigenvectors)
    assert got.eigenvectors.shape == (N, 4) and got.edge == want.edge

    caplog.set_level(logging.INFO)
    for tag, (G, P, Q) in (("merged", (Gm, Pm, Qm)), ("admixed", RO.admixed(0, 64, 2000)[:3])):
        caplog.clear()
        LO.write_bed(tmp_path / tag, G)
        data = read_bed_packed(str(tmp_path / f"{tag}.bed"), dev, keep_on_device=True)
        np.savetxt(tmp_path / f"{tag}.3.Q", Q.astype(np.float32), delimiter=" ")
        np.savetxt(tmp_path / f"{tag}.3.P", (1.0 - P if data.flipped else P).astype(np.float32), delimiter=" ")
        (tmp_path / "pops").write_text("".join(f"pop{x}\n" for x in (pop if tag == "merged" else np.zeros(N, dtype=int))))
        argv = ["residpca", "--data_path", str(tmp_path / f"{tag}.bed"), "--save_dir", str(tmp_path), "--name", tag, "--k", "3",
                "--out_name", tag + "_out", "--pops_path", str(tmp_path / "pops")]
        assert cli.main(argv) == 0
        Pr, Qr = (np.loadtxt(tmp_path / f"{tag}.3.{x}", ndmin=2) for x in "PQ")
        ref = residpca.resid_pca(data.packed, data.M, Pr, Qr)
        vals = np.loadtxt(tmp_path / f"{tag}_out.3.resid.eigenval", ndmin=1)
        rows = [ln.split() for ln in (tmp_path / f"{tag}_out.3.resid.eigenvec").read_text().splitlines()]
        assert np.array_equal(vals, ref.eigenvalues) and len(rows) == N and all(len(r) == 12 for r in rows)
        assert [r[0] for r in rows] == [str(i) for i in range(N)] == [r[1] for r in rows]
        assert np.array_equal(np.asarray([[float(x) for x in r[2:]] for r in rows]), ref.eigenvectors)
        msgs = [r.getMessage() for r in caplog.records]
        assert sum(bool(re.search(r"PC\d+: eigenvalue .* x the edge", m)) for m in msgs) == 10
        assert any("Residual eigenvalues and eigenvectors saved." in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
        warns = [m for m in msgs if "Warning" in m]
        print(f"{tag}: ratio {ref.ratio[0]:.4f}, {len(warns)} warnings")
        if tag == "merged":
            assert ref.ratio[0] > 2 and len(warns) == 1 and "residual PC1" in warns[0] and "Try K = 4" in warns[0]
            ends = [m for m in msgs if "groups at the two ends of PC1" in m]
            assert len(ends) == 1 and {"pop2", "pop3"} == set(re.findall(r"pop\d", ends[0]))
            assert any("samples with the largest |score| on PC1" in m for m in msgs)
        else:
            assert ref.ratio[0] < 1.2 and not warns
    # without labels the groups are the largest components; --extract and --keep run on the listed SNPs and samples
    (tmp_path / "keep").write_text("".join(f"rs{j}\n" for j in range(0, M, 2)))
    np.savetxt(tmp_path / "half.3.P", np.loadtxt(tmp_path / "merged.3.P", ndmin=2)[0::2], delimiter=" ")
    np.savetxt(tmp_path / "half.3.Q", np.loadtxt(tmp_path / "merged.3.Q", ndmin=2)[:48], delimiter=" ")
    (tmp_path / "samples").write_text("".join(f"f{i} s{i}\n" for i in range(48)))
    caplog.clear()
    assert cli.main(["residpca", "--data_path", str(tmp_path / "merged.bed"), "--save_dir", str(tmp_path), "--name", "half", "--k", "3",
                     "--extract", str(tmp_path / "keep"), "--keep", str(tmp_path / "samples"), "--pcs", "3"]) == 0
    half = np.loadtxt(tmp_path / "half.3.resid.eigenval", ndmin=1)
    assert half.shape == (3,) and len((tmp_path / "half.3.resid.eigenvec").read_text().splitlines()) == 48
    assert any("groups are the samples' largest components" in r.getMessage() for r in caplog.records)
