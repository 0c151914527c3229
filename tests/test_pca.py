"""Standardised PCA of the packed genotypes (nadm_obs_project / nadm_obs_project_t, pca.pca, Engine.pca, the `pca` mode of the command
line).  The float64 numpy restatement and the shared data live in tests/pca_oracle.py.

THE PRODUCTS' TOLERANCE is derived, not measured: |out - out64| <= 2^-15 x (sum of |a||w| over the terms of that output), a = g o or
o.  The genotype operand is exact in one bf16 piece and three round-to-nearest bf16 pieces carry an fp32 value exactly (3 x 8
significand bits), so every product that enters is exact and the whole error is that of the fp32 sums.  One
v_mfma_f32_16x16x32_bf16 adds 32 exact products to its accumulator; taken as a pairwise tree with the accumulator that is
log2(32) + 1 = 6 roundings, each at most 2^-24 of the sum of magnitudes.  The longest chain at the shapes below is ONE 256-SNP chunk
of the forward product (asserted through nadm_obs_project_chunks): 8 steps x 2 matrices x 3 pieces = 48 instructions into one
accumulator, 48 x 6 x 2^-24 = 1.7e-5; the float64 fold of the ranges and the one rounding of the result add 2^-24 = 6e-8.  Together
below 2^-15 = 3.05e-5, the bound tests/test_kinship.py derives for its products and the largest the products may be given.  The
transposed product's chain is shorter (one 64-sample tile in a slice at these shapes: 2 steps x 3 pieces = 6 instructions per
accumulator) and is held to the same bound.
OBSERVED on an MI355X (each case prints its ratios): forward 4.8e-9 .. 9.6e-8, O1 up to 1.5e-7 (2^-22.7), O2 up to 8.9e-8 over CASES;
see DESIGN.md section 4.16.

THE END-TO-END TOLERANCE is not fixed either: the same algorithm with its two products in plain fp32 numpy, against float64, on the
planted panel gives a figure per quantity (largest over the three structured PCs) that is computed here on the CPU and does not
depend on the code under test; the GPU path may differ from float64 by at most 8 x that -- three bits of margin, because the
summation orders differ.  fp32 numpy when this was written: eigenvalue 7.7e-9 relative, 1 - |cos| 1.6e-14, so the bounds were
6.2e-8 and 1.3e-13 (the test recomputes them).
OBSERVED on an MI355X: eigenvalue 2.9e-8, 1 - |cos| 4.7e-14 (with maf = 0.2, pcs 4 + 8: fp32 numpy 1.3e-8 and 5.0e-12, the GPU 6.1e-8
and 4.6e-13); see DESIGN.md section 4.16."""
import ctypes as C
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
from packed_rows import case_rows, dev as _dev, packed as _packed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.0 ** -15
RESIDENT = 200
# (b, M, C): every b, M and C of the issue at least once, not their product; 4300 > 4096 rows drawn with repeats from the 200 resident
CASES = [(1, 257, 1), (63, 1027, 8), (65, 3001, 20), (200, 257, 32), (4300, 1027, 20), (200, 3001, 8), (63, 257, 32), (65, 1027, 1),
         (4300, 3001, 32)]
NEW = ["nadm_obs_project_chunks", "nadm_obs_project_ranges", "nadm_obs_project_scratch_floats", "nadm_obs_project",
       "nadm_obs_project_t_slices", "nadm_obs_project_t_scratch_floats", "nadm_obs_project_t"]


def _lib():
    from neural_admixture_amd._lib import lib, EXPORTS
    return lib, EXPORTS


def _cp(c):
    return 16 if c <= 16 else 32


# ================================================================================================ CPU: the oracle
def test_oracle_by_hand():
    """G (samples x SNPs, 3 = missing):        SNP0: calls 0 1 2      n 3  S 3  f 1/2  c 1    s sqrt2   Z (-sqrt2, 0, sqrt2)
         0 0 2 1                               SNP1: calls 0 . 2      n 2  S 2  f 1/2  c 1    s sqrt2   Z (-sqrt2, 0, sqrt2)
         1 3 2 0                               SNP2: calls 2 2 2      monomorphic             s 0       Z 0
         2 2 2 1                               SNP3: calls 1 0 1      n 3  S 2  f 1/3  c 2/3  s 3/2     Z (1/2, -1, 1/2)
    M_eff = 3.  Z Z^T = [[4.25, -0.5, -3.75], [-0.5, 1, -0.5], [-3.75, -0.5, 4.25]]; (1, 0, -1) is an eigenvector with eigenvalue 8,
    the other two eigenvalues are 1.5 and 0: the top eigenpair of the GRM is 8/3 with (1, 0, -1) / sqrt2."""
    G = np.asarray([[0, 0, 2, 1], [1, 3, 2, 0], [2, 2, 2, 1]], dtype=np.uint8)
    r2 = np.sqrt(2.0)
    f, c, s, m_eff = PO.standardise(G)
    assert np.allclose(f, [0.5, 0.5, 1.0, 1.0 / 3.0], atol=1e-15) and np.allclose(c, 2 * f)
    assert np.allclose(s, [r2, r2, 0.0, 1.5], atol=1e-15) and m_eff == 3
    Zw = np.asarray([[-r2, -r2, 0, 0.5], [0, 0, 0, -1.0], [r2, r2, 0, 0.5]])
    assert np.allclose(PO.Z(G), Zw, atol=1e-15)
    grm = np.asarray([[4.25, -0.5, -3.75], [-0.5, 1.0, -0.5], [-3.75, -0.5, 4.25]]) / 3.0
    assert np.allclose(PO.grm(G), grm, atol=1e-15)
    lam, U = PO.grm_eigh(G)
    assert np.allclose(lam, [8.0 / 3.0, 0.5, 0.0], atol=1e-14)
    assert abs(abs(U[:, 0] @ np.asarray([1.0, 0.0, -1.0]) / r2) - 1.0) < 1e-14 and abs(np.linalg.norm(U[:, 0]) - 1.0) < 1e-15
    # the SNP with f = 1/3 goes at maf 0.4; at 0.5 + nothing is left but the two f = 1/2 SNPs either
    assert PO.standardise(G, maf=0.4)[3] == 2 and PO.standardise(G, maf=0.4)[2][3] == 0.0


def test_standardise_from_counts_equals_the_oracle():
    """pca.standardise works from nadm_snp_counts' three integers per SNP: centre, scale, M_eff and the trace sum_ij Z_ij^2 / M_eff
    against the oracle's Z, with and without a maf cut; nothing left to standardise is refused in words."""
    from neural_admixture_amd import pca
    G = PO.planted_panel()
    o = G != 3
    g = np.where(o, G, 0).astype(np.int64)
    cnt = np.stack([o.sum(axis=0), g.sum(axis=0), (g * g).sum(axis=0)], axis=1)
    for maf in (0.0, 0.2):
        _, c64, s64, m64 = PO.standardise(G, maf)
        c, s, m_eff, total = pca.standardise(cnt, maf)
        use = s64 > 0
        assert m_eff == m64 and np.array_equal(s > 0, use)
        assert np.allclose(s, s64, rtol=1e-14, atol=0) and np.allclose(c[use], c64[use], rtol=1e-14, atol=0)
        assert abs(total - (PO.Z(G, maf) ** 2).sum() / m64) <= 1e-12 * total
    assert PO.standardise(G)[3] == G.shape[1] - 3 and PO.standardise(G, 0.2)[3] < G.shape[1] - 3
    with pytest.raises(RuntimeError, match="no SNP is left to standardise"):
        pca.standardise(np.asarray([[5, 0, 0], [0, 0, 0], [4, 8, 16]]))
    with pytest.raises(RuntimeError, match="no SNP is left to standardise"):
        pca.standardise(np.asarray([[10, 1, 1], [10, 19, 37]]), 0.2)          # f = 0.05 and 0.95: both below the cut


def test_algorithm_against_the_dense_eigh():
    """The float64 randomised restatement (default pcs 10, oversample 10, iters 10, the same Omega as pca.pca) against eigh of the
    dense GRM of the planted panel (4 populations, 200 x 3001, Fst 0.1, 5 % missing, two monomorphic SNPs and one nobody observed),
    for the three structured PCs (eigenvalues 10.0, 9.4, 9.0 above a noise bulk that starts at 1.41).
    BOUNDS, chosen here on the CPU for the restatement alone: eigenvalue within 1e-13 relative, 1 - |cos| <= 1e-16.  ROOM: the
    restatement shows 5.7e-16 and 2.8e-19 -- two orders below both.  The noise-bulk PCs 4.. are NOT compared, neither one by one nor
    as a subspace: their eigenvalues lie 1-3 % apart and 10 rounds do not separate them (the restatement's are 0.5-3 % low)."""
    G = PO.planted_panel()
    lam, U = PO.grm_eigh(G)
    v, u, m_eff, ex = PO.rsvd(G)
    assert lam[2] > 5 * lam[3] and m_eff == G.shape[1] - 3
    ev, ang = PO.pc_errors(v, u, lam, U, PO.STRUCTURED)
    print(f"float64 restatement vs dense eigh: eigenvalue {ev.max():.3e}, 1 - |cos| {ang.max():.3e}")
    assert (ev <= 1e-13).all() and (ang <= 1e-16).all()
    assert np.allclose(ex[:3], lam[:3] / np.trace(PO.grm(G)), rtol=1e-12)
    assert (np.diff(v) <= 0).all() and np.allclose(np.linalg.norm(u, axis=0), 1.0, atol=1e-14)
    assert (u[np.argmax(np.abs(u), axis=0), np.arange(u.shape[1])] > 0).all()


# ================================================================================================ CPU: symbols, refusals, queries
def test_symbols_are_declared_bound_and_exported():
    lib, EXPORTS = _lib()
    header = open(os.path.join(ROOT, "include", "nadm.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in EXPORTS and hasattr(lib, name)
    assert lib.nadm_abi_version() == 14
    assert "#define NADM_OBS_MAX_ROWS (1 << 24)" in header


def _refused(status, pattern):
    lib, _ = _lib()
    msg = lib.nadm_last_error().decode()
    assert status == 1 and re.search(pattern, msg), (status, msg)


def test_every_refusal_of_both_entries_comes_before_a_launch():
    """Every call below is refused (status 1 and the reason through nadm_last_error): none reaches a launch, so none needs a GPU.
    Pointers are made-up aligned addresses; nothing dereferences them."""
    lib, _ = _lib()
    A = 1 << 20                                              # an aligned made-up address

    def fwd(xp=A, ld=272, idx=None, b=8, M=1027, W1=A, W2=A, c=8, cp=16, Y=A, scr=A):
        return lib.nadm_obs_project(xp, ld, idx, b, M, W1, W2, c, cp, Y, scr, None)

    def tr(xp=A, ld=272, idx=None, b=8, M=1027, Yin=A, c=8, cp=16, O1=A, O2=A, scr=A):
        return lib.nadm_obs_project_t(xp, ld, idx, b, M, Yin, c, cp, O1, O2, scr, None)
    for f, ptrs, who in ((fwd, ("xp", "W1", "W2", "Y", "scr"), "nadm_obs_project"), (tr, ("xp", "Yin", "O1", "O2", "scr"), "nadm_obs_project_t")):
        for p in ptrs:
            _refused(f(**{p: None}), who + ": null pointer")
        for kw in (dict(b=0), dict(b=-1), dict(M=0)):
            _refused(f(**kw), who + ": empty block")
        _refused(f(b=(1 << 24) + 1), who + ": b must be <= NADM_OBS_MAX_ROWS")
        _refused(f(ld=256), who + r": ld < ceil\(M/4\)")
        for ld in (264, 1 << 32):
            _refused(f(ld=ld), who + ": ld must be a multiple of 16 and < 2\\^32")
        for cp in (0, 8, 24, 64):
            _refused(f(cp=cp), who + ": CP must be 16 or 32")
        for kw in (dict(c=0), dict(c=17), dict(c=33, cp=32), dict(c=-1)):
            _refused(f(**kw), who + r": C must be in 1\.\.CP")
        _refused(f(xp=A + 8), who + ": xp must be 16-byte and idx 4-byte aligned")
        _refused(f(idx=A + 2), who + ": xp must be 16-byte and idx 4-byte aligned")
        for p in ptrs[1:]:
            _refused(f(**{p: A + 4}), who + ": .* must be 16-byte aligned")


def test_the_split_and_scratch_queries():
    """The split is a rule of the shape alone: an fp32 accumulator of the forward product covers at most 1024 chunks = 2^18 SNPs and
    the ranges cover every chunk; the transposed product's slices are those of nadm_snp_hwe_slices (at most 4096 samples each); the
    scratch sizes grow with b and with M and hold what the kernels write; a shape outside the entries' limits gives 0."""
    lib, _ = _lib()
    bs = [1, 63, 64, 65, 200, 256, 257, 4096, 4097, 4300, 100_000, 1 << 24]
    Ms = [1, 256, 257, 1027, 3001, 65_536, 600_000, 5_000_000, 300_000_000]
    for cp in (16, 32):
        prev_b = None
        for b in bs:
            row = []
            for M in Ms:
                chunks = (M + 255) // 256
                cpr, ranges = lib.nadm_obs_project_chunks(b, M), lib.nadm_obs_project_ranges(b, M)
                assert 1 <= cpr <= 1024 and ranges == (chunks + cpr - 1) // cpr
                fs = lib.nadm_obs_project_scratch_floats(b, M, cp)
                assert fs >= ranges * ((b + 255) // 256) * 256 * cp
                sl = lib.nadm_obs_project_t_slices(b, M)
                tiles = (b + 63) // 64
                assert sl == lib.nadm_snp_hwe_slices(b, M) and 1 <= sl <= tiles and (tiles + sl - 1) // sl <= 64
                ts = lib.nadm_obs_project_t_scratch_floats(b, M, cp)
                assert ts >= sl * chunks * 256 * 2 * cp
                row.append((fs, ts))
            assert all(a[0] <= c[0] and a[1] <= c[1] for a, c in zip(row, row[1:])), "not monotone in M"
            if prev_b is not None:
                assert all(a[0] <= c[0] and a[1] <= c[1] for a, c in zip(prev_b, row)), "not monotone in b"
            prev_b = row
    for b, M, cp in ((0, 10, 16), (10, 0, 16), ((1 << 24) + 1, 10, 16), (10, 10, 8)):
        assert lib.nadm_obs_project_scratch_floats(b, M, cp) == 0 and lib.nadm_obs_project_t_scratch_floats(b, M, cp) == 0
    assert lib.nadm_obs_project_ranges(0, 10) == 0 and lib.nadm_obs_project_chunks(10, 0) == 0 and lib.nadm_obs_project_t_slices(0, 10) == 0
    # the shapes the GPU cases use: ONE chunk per range (the chain the tolerance is derived for), and more than one slice above 4096 rows
    for b, M, _ in CASES:
        assert lib.nadm_obs_project_chunks(b, M) == 1
    assert lib.nadm_obs_project_t_slices(4300, 1027) > 1 and lib.nadm_obs_project_t_slices(4300, 3001) > 1


def test_pca_refuses_bad_arguments_without_a_gpu():
    """L = pcs + oversample > 32, a maf outside [0, 0.5) and non-positive counts are refused before the matrix is looked at (None
    stands in for it); a matrix that is not on a GPU is refused next; M_eff == 0 is standardise's (above)."""
    from neural_admixture_amd import pca
    import neural_admixture_amd as na
    assert na.pca is pca and callable(na.pca.pca) and na.obs_project is pca.obs_project and "pca" in na.__all__
    with pytest.raises(RuntimeError, match=r"pcs \+ oversample must be <= 32.*got 23 \+ 10"):
        pca.pca(None, 100, pcs=23)
    assert pca.check_args(22, 10, 10, 0.0) == 32 and pca.pad_columns(16) == 16 and pca.pad_columns(17) == 32
    for bad in (-0.01, 0.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"maf must be in \[0, 0.5\)"):
            pca.pca(None, 100, maf=bad)
    with pytest.raises(RuntimeError, match="pcs must be >= 1"):
        pca.pca(None, 100, pcs=0)
    with pytest.raises(RuntimeError, match="oversample must be >= 0"):
        pca.pca(None, 100, oversample=-1)
    with pytest.raises(RuntimeError, match="iters must be >= 0"):
        pca.pca(None, 100, iters=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.pca(torch.zeros((4, 16), dtype=torch.uint8), 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.obs_project(torch.zeros((4, 16), dtype=torch.uint8), 40, torch.zeros((40, 16)), torch.zeros((40, 16)), 3)


def test_sharded_and_cpu_engines_refuse_pca():
    """Engine.pca is single-GPU and needs the resident matrix; the checks come first, so a stand-in without device state shows them."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.pca is single-GPU"):
        e.pca()
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.pca needs the HIP engine with its packed matrix resident"):
        e.pca(pcs=3)


# ================================================================================================ CPU: the command line
def test_cli_pca_refuses_before_any_data_is_read(tmp_path, monkeypatch):
    """The parser has the mode's flags; argument errors and missing or misshapen files end the run with the offender named, before
    the GPU check and before a genotype is read (the reader is a stand-in that fails the test); --extract resolves."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    base = ["pca", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_pca_args(base[1:])
    assert (a.pcs, a.oversample, a.iters, a.maf, a.seed, a.out_name, a.extract, a.threads) == (10, 10, 10, 0.0, 42, None, None, 1)
    a = cli.parse_pca_args(base[1:] + ["--pcs", "4", "--oversample", "6", "--iters", "3", "--maf", "0.05", "--seed", "7", "--out_name", "o",
                                      "--extract", "f", "--threads", "4"])
    assert (a.pcs, a.oversample, a.iters, a.maf, a.seed, a.out_name, a.extract, a.threads) == (4, 6, 3, 0.05, 7, "o", "f", 4)
    assert "pca" in cli._ANALYSIS_MODES

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=r"pcs \+ oversample must be <= 32"):
        cli.main(base + ["--pcs", "30"])
    with pytest.raises(SystemExit, match=r"maf must be in \[0, 0.5\)"):
        cli.main(base + ["--maf", "0.5"])
    with pytest.raises(SystemExit, match="pcs must be >= 1"):
        cli.main(base + ["--pcs", "0"])
    with pytest.raises(SystemExit, match="iters must be >= 0"):
        cli.main(base + ["--iters", "-2"])
    with pytest.raises(SystemExit, match=r"x\.fam not found"):
        cli.main(base)
    with pytest.raises(SystemExit, match=r"nothing\.vcf not found"):
        cli.main(base[:-1] + [str(tmp_path / "nothing.vcf")])
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(base[:-1] + [str(tmp_path / "x.pgen")])
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    bed.write_bytes(bytes(3 + 2 * 4 + 1))                    # N = 5: two bytes a SNP; one byte too many
    with pytest.raises(SystemExit, match=r"x\.bed does not hold whole SNPs"):
        cli.main(base)
    bed.write_bytes(bytes(3 + 2 * 4))                        # M = 4
    with pytest.raises(SystemExit, match=r"nolist not found"):
        cli.main(base + ["--extract", str(tmp_path / "nolist")])
    (tmp_path / "x.bim").write_text("".join(f"1\trs{j}\t0\t{j + 1}\tA\tG\n" for j in range(4)))
    (tmp_path / "list").write_text("rs1\nrs9\n")
    with pytest.raises(SystemExit, match="rs9"):
        cli.main(base + ["--extract", str(tmp_path / "list")])
    (tmp_path / "list").write_text("rs1\nrs3\n")
    assert cli._extract_keep(str(bed), str(tmp_path / "list")).tolist() == [False, True, False, True]
    for more in ([], ["--extract", str(tmp_path / "list")]):
        with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):           # everything is in order: the GPU check is what is left
            cli.main(base + more)
    assert not list(tmp_path.glob("*.eigenval")) and not list(tmp_path.glob("*.eigenvec"))


def test_writers_formats_on_a_made_up_result(tmp_path, caplog):
    """{stem}.eigenval: one value per line; {stem}.eigenvec: per sample two identifier columns (the 0-based index, as the kinship
    mode names samples) and PC1 .., plink's layout; both read back to the same float64.  The log names every PC with its share."""
    from neural_admixture_amd import pca
    rng = np.random.default_rng(3)
    vec = pca.orient(rng.standard_normal((7, 3)))
    res = pca.PcaResult(np.asarray([3.0, 1.0 / 3.0, 1e-9]), vec, 1234, np.asarray([0.3, 1.0 / 30.0, 1e-10]), 10.0)
    pca.write_result(str(tmp_path / "o"), res)
    vals = (tmp_path / "o.eigenval").read_text().splitlines()
    assert len(vals) == 3 and [float(v) for v in vals] == res.eigenvalues.tolist()
    rows = [ln.split() for ln in (tmp_path / "o.eigenvec").read_text().splitlines()]
    assert len(rows) == 7 and all(len(r) == 5 for r in rows) and [r[:2] for r in rows] == [[str(i), str(i)] for i in range(7)]
    assert np.array_equal(np.asarray([[float(x) for x in r[2:]] for r in rows]), vec)
    caplog.set_level(logging.INFO)
    pca.log_result(res, logging.getLogger("pca"))
    msgs = [r.getMessage() for r in caplog.records]
    assert any("over 1234 SNPs" in m for m in msgs)
    assert any("PC1: eigenvalue 3, 30.000 % of the variance" in m for m in msgs) and sum("PC" in m and "eigenvalue" in m for m in msgs) == 3


# ================================================================================================ GPU: the two products
def _operands(b, M, c, seed):
    """W1, W2 [M, CP] and Yin [b, CP] float32 on the host: standard normals in the c columns in use, pad columns 0."""
    rng = np.random.default_rng(seed)
    cp = _cp(c)
    out = []
    for rows in (M, M, b):
        a = np.zeros((rows, cp), dtype=np.float32)
        a[:, :c] = rng.standard_normal((rows, c)).astype(np.float32)
        out.append(a)
    return out


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run_fwd(xp, M, rows, W1, W2, c):
    from neural_admixture_amd import pca
    Y = pca.obs_project(xp, M, _to(W1), _to(W2), c, None if rows is None else _to(rows))
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def _run_t(xp, M, rows, Yin, c):
    from neural_admixture_amd import pca
    O1, O2 = pca.obs_project_t(xp, M, _to(Yin), c, None if rows is None else _to(rows))
    torch.cuda.synchronize()
    return O1.cpu().numpy(), O2.cpu().numpy()


def _check(got, want, mag, c, what):
    """|got - want| <= TOL mag per output, exactly 0 where mag is 0, pad columns +0.0; prints the largest ratio before it asserts."""
    err = np.abs(got[:, :c].astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(mag > 0, err / mag, 0.0)))
    print(f"{what}: max |out - out64| / sum|a||w| = {ratio:.3e} (2^{np.log2(max(ratio, 1e-300)):.1f}); bound 2^-15 = {TOL:.3e}")
    assert np.isfinite(got).all()
    assert (err <= TOL * mag).all()
    assert not got[:, :c][mag == 0].any() and got[:, c:].tobytes() == bytes(got[:, c:].nbytes)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, c", CASES)
def test_products_against_float64(b, M, c):
    """Both products on a gather list with a duplicate and the all-missing row 4 (b = 1: row 7; b = 4300: drawn with repeats from the
    200 resident rows, so that the transposed product takes more than one slice), dirty padding, against float64 within
    2^-15 x sum |a||w| (module docstring).  The all-missing row's Y is +0.0 in every bit."""
    lib, _ = _lib()
    G = np.ascontiguousarray(PO.product_panel()[:, :M])      # (contiguous and held here: the packer reads it through a raw pointer)
    xp = _packed(G, dirty=True).to(_dev())
    rows = case_rows(b, "list", RESIDENT)
    Gr = G[rows]
    W1, W2, Yin = _operands(b, M, c, 1000 * b + M + c)
    assert lib.nadm_obs_project_chunks(b, M) == 1
    if b > 4096:
        assert lib.nadm_obs_project_t_slices(b, M) > 1
    Y = _run_fwd(xp, M, rows, W1, W2, c)
    want, mag = PO.project(Gr, W1[:, :c], W2[:, :c])
    _check(Y, want, mag, c, f"obs_project b={b} M={M} C={c}")
    if b > 1:
        assert (rows == 4).any() and Y[rows == 4].tobytes() == bytes(Y[rows == 4].nbytes)
        assert np.array_equal(Y[0], Y[-1]) or b > RESIDENT           # (the list's last entry repeats its first)
    O1, O2 = _run_t(xp, M, rows, Yin, c)
    w1, w2, m1, m2 = PO.project_t(Gr, Yin[:, :c])
    _check(O1, w1, m1, c, f"obs_project_t O1 b={b} M={M} C={c}")
    _check(O2, w2, m2, c, f"obs_project_t O2 b={b} M={M} C={c}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 20])
def test_exact_zeros_and_bit_identities(c):
    """b = 65, M = 1027 (a ragged last chunk and a partial last byte), CP = 16 and 32: two calls give the same bits; dirty and clean
    padding give the same bits; without a list (rows 0..65) the all-missing row 4 gives +0.0; other finite values in the W1 / W2 rows
    of the SNPs 9 and 1025, which nobody observed, leave Y as it is bit for bit."""
    b, M = 65, 1027
    G = np.ascontiguousarray(PO.product_panel()[:, :M])      # (contiguous and held here: the packer reads it through a raw pointer)
    rows = case_rows(b, "list", RESIDENT)
    W1, W2, Yin = _operands(b, M, c, 5)
    dirty, clean = _packed(G, dirty=True).to(_dev()), _packed(G).to(_dev())
    assert not torch.equal(dirty, clean)
    Y = _run_fwd(dirty, M, rows, W1, W2, c)
    T = _run_t(dirty, M, rows, Yin, c)
    assert np.abs(Y).max() > 1 and np.abs(T[0]).max() > 1
    assert _run_fwd(dirty, M, rows, W1, W2, c).tobytes() == Y.tobytes()
    assert _run_fwd(clean, M, rows, W1, W2, c).tobytes() == Y.tobytes()
    for again in (_run_t(dirty, M, rows, Yin, c), _run_t(clean, M, rows, Yin, c)):
        assert again[0].tobytes() == T[0].tobytes() and again[1].tobytes() == T[1].tobytes()
    Yn = _run_fwd(dirty, M, None, W1, W2, c)[:b]
    assert Yn[4].tobytes() == bytes(Yn[4].nbytes) and np.abs(Yn[3]).max() > 0
    assert not (G[:, 9] != 3).any() and not (G[:, 1025] != 3).any()
    V1, V2 = W1.copy(), W2.copy()
    for j in (9, 1025):
        V1[j, :c] = 1e6 * (1 + np.arange(c))
        V2[j, :c] = -3.25e-7
    assert _run_fwd(dirty, M, rows, V1, V2, c).tobytes() == Y.tobytes()
    assert not T[0][[9, 1025]].any() and not T[1][[9, 1025]].any()


# ------------------------------------------------------------------------------------------------ placement (tests/test_placement.py's two contracts)
PM, PC = 1027, 20


@functools.lru_cache(maxsize=None)
def _placement_compact():
    import test_placement as TP
    assert TP.M == PM
    return TP._pack(np.ascontiguousarray(PO.product_panel()[:TP.ROWS, :PM]))


def _placement_case(name, mode):
    """(operands on the host without the matrix, the genotypes of the case's rows in call order)."""
    import test_placement as TP
    rows = TP._rows("wide", mode)
    W1, W2, Yin = _operands(len(rows), PM, PC, 77 + len(rows))
    x = {"W1": W1, "W2": W2} if name == "fwd" else {"Y": Yin}
    if mode == "list":
        x["idx"] = rows.copy()
    return x, PO.product_panel()[:TP.ROWS, :PM][rows]


def _op_fwd(t):
    from neural_admixture_amd import pca
    return (pca.obs_project(t["xp"], PM, t["W1"], t["W2"], PC, t.get("idx")),)


def _op_t(t):
    from neural_admixture_amd import pca
    return pca.obs_project_t(t["xp"], PM, t["Y"], PC, t.get("idx"))


PLACED = {"fwd": _op_fwd, "t": _op_t}


def _placement_check(name, got, Gr, x):
    if name == "fwd":
        want, mag = PO.project(Gr, x["W1"][:, :PC], x["W2"][:, :PC])
        _check(got[0], want, mag, PC, "obs_project (compact)")
    else:
        w1, w2, m1, m2 = PO.project_t(Gr, x["Y"][:, :PC])
        _check(got[0], w1, m1, PC, "obs_project_t O1 (compact)")
        _check(got[1], w2, m2, PC, "obs_project_t O2 (compact)")


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
        TP._assert_same_bits(got, want, f"obs_project {name} wide rows={mode}")


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
    got = TP._on_side_stream(PLACED[name], true, f"obs_project {name}")
    TP._assert_same_bits(got, want, f"obs_project {name} on a side stream")


@pytest.mark.gpu
def test_the_arena_is_released():
    """After the placement tests of this module: the 4.25 GiB buffer goes back to the device (tests/test_placement.py takes its own)."""
    import test_placement as TP
    TP._ARENA.update(kind=None, buf=None)
    torch.cuda.empty_cache()


# ================================================================================================ GPU: end to end
@functools.lru_cache(maxsize=None)
def _fp32_numpy_figures(**kw):
    """(eigenvalue, 1 - |cos|): the largest over the structured PCs of the fp32-numpy restatement against the float64 one, both run
    with the arguments ``kw`` on the planted panel."""
    G = PO.planted_panel()
    v, u, _, _ = PO.rsvd(G, **kw)
    v32, u32, _, _ = PO.rsvd(G, dtype=np.float32, **kw)
    ev, ang = PO.pc_errors(v32, u32, v, u, PO.STRUCTURED)
    return float(ev.max()), float(ang.max())


@functools.lru_cache(maxsize=None)
def _gpu_default():
    from neural_admixture_amd import pca
    G = PO.planted_panel()
    res = pca.pca(_packed(G, dirty=True).to(_dev()), G.shape[1])
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
def test_pca_against_the_float64_restatement():
    """pca() with its defaults on the planted panel against the float64 restatement with the same Omega, per structured PC: the
    eigenvalue's relative error and 1 - |cos| at most 8 x the fp32-numpy restatement's figure (module docstring: three bits of
    margin for the different summation orders; both figures are printed).  M_eff, the share explained and the total are float64
    work on the host and are held tightly."""
    G = PO.planted_panel()
    v, u, m_eff, ex = PO.rsvd(G)
    res = _gpu_default()
    e32, a32 = _fp32_numpy_figures()
    ev, ang = PO.pc_errors(res.eigenvalues, res.eigenvectors, v, u, PO.STRUCTURED)
    print(f"fp32 numpy vs float64: eigenvalue {e32:.3e}, 1 - |cos| {a32:.3e};  GPU vs float64: eigenvalue {ev.max():.3e}, 1 - |cos| {ang.max():.3e}")
    assert e32 > 0 and a32 > 0
    assert res.M_eff == m_eff == G.shape[1] - 3
    assert res.eigenvalues.shape == (10,) and res.eigenvectors.shape == (G.shape[0], 10) and res.explained.shape == (10,)
    assert (ev <= 8 * e32).all(), (ev, e32)
    assert (ang <= 8 * a32).all(), (ang, a32)
    assert abs(res.total - (PO.Z(G) ** 2).sum() / m_eff) <= 1e-12 * res.total
    assert np.allclose(res.explained, res.eigenvalues / res.total, rtol=1e-14)
    assert np.allclose(res.explained[:3], ex[:3], rtol=1e-6)


@pytest.mark.gpu
def test_eigenvectors_are_orthonormal_and_oriented():
    res = _gpu_default()
    U = res.eigenvectors
    assert np.abs(U.T @ U - np.eye(U.shape[1])).max() <= 1e-5
    assert (U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])] > 0).all()
    assert (np.diff(res.eigenvalues) <= 0).all() and (res.eigenvalues > 0).all()


@pytest.mark.gpu
def test_maf_drops_what_it_should():
    """maf = 0.2 leaves the SNPs the oracle leaves, and the result is the restatement's for that cut: the same 8 x fp32 rule, the
    fp32-numpy figure taken for these arguments."""
    from neural_admixture_amd import pca
    G = PO.planted_panel()
    kw = dict(pcs=4, oversample=8, maf=0.2)
    res = pca.pca(_packed(G).to(_dev()), G.shape[1], **kw)
    v, u, m_eff, _ = PO.rsvd(G, **kw)
    assert res.M_eff == m_eff < _gpu_default().M_eff
    e32, a32 = _fp32_numpy_figures(**kw)
    ev, ang = PO.pc_errors(res.eigenvalues, res.eigenvectors, v, u, PO.STRUCTURED)
    print(f"maf 0.2: fp32 numpy vs float64: eigenvalue {e32:.3e}, 1 - |cos| {a32:.3e};  GPU vs float64: eigenvalue {ev.max():.3e}, 1 - |cos| {ang.max():.3e}")
    assert (ev <= 8 * e32).all() and (ang <= 8 * a32).all()


@pytest.mark.gpu
def test_idx_equals_the_subsets_own_matrix():
    """A gather list of 120 rows in ascending order against the run on a matrix that holds only those rows."""
    from neural_admixture_amd import pca
    G = PO.planted_panel()
    pick = np.sort(np.random.default_rng(2).choice(G.shape[0], size=120, replace=False)).astype(np.int32)
    a = pca.pca(_packed(G).to(_dev()), G.shape[1], pcs=4, oversample=6, idx=pick)
    b = pca.pca(_packed(np.ascontiguousarray(G[pick])).to(_dev()), G.shape[1], pcs=4, oversample=6)
    assert a.M_eff == b.M_eff and a.eigenvectors.shape == (120, 4)
    assert np.allclose(a.eigenvalues, b.eigenvalues, rtol=1e-9, atol=0)
    assert np.abs(a.eigenvectors[:, :3] - b.eigenvectors[:, :3]).max() <= 1e-7


@pytest.mark.gpu
def test_engine_and_command_line_give_the_functions_numbers(tmp_path, caplog):
    """Engine.pca on the engine's resident matrix and the `pca` mode on a small BED written here equal pca.pca on the same packed
    rows; the two files are well formed and read back to the returned numbers; --extract runs on the listed SNPs."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli, pca
    from neural_admixture_amd.io import read_bed_packed
    from oracle import nadm_oracle as O
    dev = _dev()
    G = np.ascontiguousarray(PO.planted_panel(N=60, M=1027, seed=9))
    N, M = G.shape
    kw = dict(pcs=4, oversample=6, iters=5, maf=0.05, seed=3)
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(3, M)).astype(np.float32)
    p = O.make_params(42, V0, P0, 64, [3])
    e = na.Engine(M, 8, 64, [3], dev, N)
    e.load_params(V0, P0, np.concatenate([p.g, p.W1.reshape(-1), p.b1, p.Wk[0].reshape(-1), p.bk[0]]))
    e.pack_from_host(torch.from_numpy(G))
    got = e.pca(**kw)
    want = pca.pca(e.xp, M, **kw)
    assert got.M_eff == want.M_eff and np.array_equal(got.eigenvalues, want.eigenvalues) and np.array_equal(got.eigenvectors, want.eigenvectors)
    v, u, m_eff, _ = PO.rsvd(G, **kw)
    assert got.M_eff == m_eff and np.allclose(got.eigenvalues[:3], v[:3], rtol=1e-5)

    LO.write_bed(tmp_path / "panel", G)
    caplog.set_level(logging.INFO)
    argv = ["pca", "--data_path", str(tmp_path / "panel.bed"), "--save_dir", str(tmp_path / "out"), "--name", "run", "--pcs", "4",
            "--oversample", "6", "--iters", "5", "--maf", "0.05", "--seed", "3"]
    assert cli.main(argv) == 0
    data = read_bed_packed(str(tmp_path / "panel.bed"), dev, keep_on_device=True)
    ref = pca.pca(data.packed, data.M, **kw)
    vals = np.loadtxt(tmp_path / "out" / "run.eigenval", ndmin=1)
    rows = [ln.split() for ln in (tmp_path / "out" / "run.eigenvec").read_text().splitlines()]
    assert np.array_equal(vals, ref.eigenvalues) and len(rows) == N and all(len(r) == 6 for r in rows)
    assert [r[0] for r in rows] == [str(i) for i in range(N)] == [r[1] for r in rows]
    assert np.array_equal(np.asarray([[float(x) for x in r[2:]] for r in rows]), ref.eigenvectors)
    assert np.allclose(vals[:3], v[:3], rtol=1e-5)           # (a flipped file has Z -> -Z: the same GRM)
    msgs = [r.getMessage() for r in caplog.records]
    assert sum(bool(re.search(r"PC\d: eigenvalue .* % of the variance", m)) for m in msgs) == 4
    assert any("Eigenvalues and eigenvectors saved." in m for m in msgs) and any("Total elapsed time" in m for m in msgs)
    (tmp_path / "keep").write_text("".join(f"rs{j}\n" for j in range(0, M, 2)))
    assert cli.main(argv + ["--extract", str(tmp_path / "keep"), "--out_name", "half"]) == 0
    half = np.loadtxt(tmp_path / "out" / "half.eigenval", ndmin=1)
    vh, _, mh, _ = PO.rsvd(np.ascontiguousarray(G[:, 0::2]), **kw)
    assert half.shape == (4,) and np.allclose(half[:3], vh[:3], rtol=1e-5)
    assert any(f"over {mh} SNPs" in m for m in [r.getMessage() for r in caplog.records])
