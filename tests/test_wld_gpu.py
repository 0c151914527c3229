"""nadm_wld on the GPU against the numpy restatement of its contract (tests/wld_oracle.py), BY EQUALITY of the int64 arrays: the sums
are integers, so there is no tolerance to choose.  Shapes: the smallest that reach each path of the kernel -- rows either side of the
64-sample step, M that is no multiple of 4 (tail bits and pad bytes garbage), a reach of one "b" tile, of exactly 16, of more than one
blockIdx.y group and of thousands of SNPs, ranges that start and end inside a 64-SNP block, a permuted gather list with a duplicate, a
chromosome gap in the grid, bins that drop pairs, 1, 3 and 32 curves, weights of both signs and zero."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_oracle as LO  # noqa: E402
import wld_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# name: (matrix rows, M, W, m0, m1, C, nbins, gather list?, max cell step)
CASES = {
    "two_rows":    (2, 17, 1, 0, 17, 1, 4, False, 2),
    "rows63_w15":  (63, 64, 15, 3, 61, 3, 9, False, 2),
    "rows64_w16":  (64, 65, 16, 0, 65, 32, 12, False, 2),
    "rows65_w150": (65, 203, 150, 5, 199, 3, 60, True, 2),
    "rows130_c32": (130, 203, 150, 70, 203, 32, 200, True, 2),
    "rows130_w1":  (130, 203, 1, 1, 202, 3, 2, False, 1),
    "w3000":       (64, 3100, 3000, 0, 3100, 1, 64, False, 0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host inputs and the restatement's answer, computed once and left unchanged."""
    n_mat, M, W, m0, m1, Cn, nbins, listed, step = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    f = rng.uniform(0.05, 0.95, size=M)
    G = rng.binomial(2, f, size=(n_mat, M)).astype(np.uint8)
    G[rng.random((n_mat, M)) < (0.12 if n_mat == 2 else 0.08)] = 3       # two rows: many pairs fall below nmin = 2 and are skipped
    ld = (M + 3) // 4 + 15 & ~15
    xp = WO.pack(G, ld + 16, rng)                                        # a spare 16 bytes of pad, garbage like the tail bits
    if listed:                                                           # permuted, one duplicate, one row left out
        rows = rng.permutation(n_mat)[: n_mat - 1]
        rows = np.concatenate([rows, rows[4:5]]).astype(np.int32)         # n_mat entries
    else:
        rows = None
    if step == 0:
        cell = (np.arange(M) // 50).astype(np.int32)                     # every pair within W stays below nbins
    else:
        inc = rng.integers(0, step + 1, size=M)
        inc[0] = 0
        inc[(m0 + m1) // 2] = nbins + 1                                  # a chromosome gap inside the range
        cell = np.cumsum(inc).astype(np.int32)
    wt = rng.uniform(-1.0, 1.0, size=(Cn, M))
    wt[:, rng.random(M) < 0.1] = 0.0
    wt[0, :3] = (1.0, -1.0, 0.0)
    want = WO.wld_restatement(G if rows is None else G[rows], m0, m1, W, cell, wt, nbins, 2)
    assert want[1].sum() > 0 and np.any(want[0] != 0)
    if step:
        total = sum(min(W, m1 - 1 - a) for a in range(m0, m1))
        assert want[1].sum() < total                                     # pairs were dropped (the bins, the gap) or skipped (nmin)
    for a in (G, xp, cell, wt, *want):
        a.setflags(write=False)
    return xp, rows, cell, wt, want


def _run(name, xp_d=None, ld=None):
    """One nadm_wld call through the raw binding: (sum, cnt) as numpy."""
    from neural_admixture_amd._lib import lib, check, ptr
    n_mat, M, W, m0, m1, Cn, nbins, listed, _ = CASES[name]
    xp, rows, cell, wt, _ = _case(name)
    dev = _dev()
    if xp_d is None:
        xp_d, ld = torch.from_numpy(xp.copy()).to(dev), xp.shape[1]
    idx = None if rows is None else torch.from_numpy(rows.copy()).to(dev)
    n = len(rows) if rows is not None else n_mat
    cell_d, wt_d = torch.from_numpy(cell.copy()).to(dev), torch.from_numpy(wt.copy()).to(dev)
    s = torch.empty((Cn, nbins), dtype=torch.int64, device=dev)
    c = torch.empty((nbins,), dtype=torch.int64, device=dev)
    s.view(torch.uint8).random_(0, 256), c.view(torch.uint8).random_(0, 256)          # the entry zeroes both
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.nadm_wld(ptr(xp_d), ld, ptr(idx), n, M, m0, m1, W, ptr(cell_d), ptr(wt_d), Cn, nbins, 2, ptr(s), ptr(c), st), "wld")
    torch.cuda.current_stream().synchronize()
    return s.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_wld_equals_the_restatement(name):
    got = _run(name)
    want = _case(name)[4]
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1]), "cnt"
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), "sum"


def test_two_runs_give_identical_bits_and_a_side_stream_the_same():
    a, b = _run("rows130_c32"), _run("rows130_c32")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run("rows65_w150")
    torch.cuda.current_stream().wait_stream(side)
    want = _case("rows65_w150")[4]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_row_offsets_past_4_gib():
    """ld = 2^25: rows 128 and 129 of the 130 start past 2^32 bytes.  The buffer is address space (torch.empty); only the head of
    every row is written."""
    name = "rows130_c32"
    xp = _case(name)[0]
    ld, n = 1 << 25, xp.shape[0]
    assert n == 130 and 127 * ld < 2 ** 32 <= 128 * ld
    free, _ = torch.cuda.mem_get_info()
    if free < n * ld + (2 << 30):
        pytest.skip(f"the wide matrix needs {n * ld / 2 ** 30:.2f} GiB + 2 GiB of free HBM, {free / 2 ** 30:.2f} GiB are free")
    buf = torch.empty((n, ld), dtype=torch.uint8, device=_dev())
    buf[:, :4096] = 0xFF
    buf[:, : xp.shape[1]] = torch.from_numpy(xp.copy()).to(_dev())
    got = _run(name, buf, ld)
    del buf
    torch.cuda.empty_cache()
    want = _case(name)[4]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the Python layer on a simulated panel ----------------------------------------------------------------------------------------
PANEL = dict(N=60, chroms=2, snps=400, spacing=0.05, n_gen=20.0)
FIT = dict(binsize=0.05, dmin=0.5, maxdist=10.0)


@functools.lru_cache(maxsize=None)
def _panel():
    from neural_admixture_amd import admixdate as ad
    G, cm, chrom, pa, pb = WO.simulate(11, PANEL["N"], PANEL["chroms"], PANEL["snps"], PANEL["spacing"], PANEL["n_gen"])
    M = G.shape[1]
    nbins = ad.check_args(FIT["binsize"], FIT["dmin"], FIT["maxdist"])
    cell, ranges = ad.grid_cells(cm, chrom, FIT["binsize"], nbins)
    rng = np.random.default_rng(5)
    P = np.stack([pa, pb, rng.uniform(0.05, 0.95, size=M)], axis=1).astype(np.float32)
    Q = np.tile(np.asarray([[0.5, 0.44, 0.06]]), (PANEL["N"], 1))
    pairs = ad.choose_pairs(Q)
    assert pairs == [(0, 1), (0, 2), (1, 2)]
    wt = ad.component_weights(P, pairs)
    want = WO.wld_restatement_ranges(G, ranges, ad.reach(cell, nbins, ranges), cell, wt, nbins)
    xp = WO.pack(G, ((M + 3) // 4 + 127) // 128 * 128)
    return G, xp, cm, chrom, P, Q, cell, ranges, nbins, wt, want


def test_wld_curves_and_admix_date_on_a_simulated_panel():
    from neural_admixture_amd import admixdate as ad
    G, xp, cm, chrom, P, Q, cell, ranges, nbins, wt, want = _panel()
    xp_d = torch.from_numpy(xp.copy()).to(_dev())
    M = G.shape[1]
    s, n = ad.wld_curves(xp_d, M, cell, wt, nbins, chrom_ranges=ranges)
    assert s.shape == (2, 3, nbins) and n.shape == (2, nbins) and s.dtype == n.dtype == np.int64
    assert np.array_equal(n, want[1]) and np.array_equal(s, want[0])
    # more than 32 curves: groups of 32, the same integers curve by curve
    wt35 = np.concatenate([wt] * 11 + [wt[:2]])
    s35, n35 = ad.wld_curves(xp_d, M, cell, wt35, nbins, chrom_ranges=ranges)
    assert s35.shape == (2, 35, nbins) and np.array_equal(n35, n)
    assert all(np.array_equal(s35[:, c], s[:, c % 3]) for c in range(35))
    # the fit is the same host code on equal integers
    got = ad.admix_date(xp_d, M, P, Q, cm, chrom, **FIT)
    ref = ad.date_from_curves(want[0], want[1], FIT["binsize"], FIT["dmin"], FIT["maxdist"], [(0, 1), (0, 2), (1, 2)])
    assert np.array_equal(got.sum, want[0]) and np.array_equal(got.cnt, want[1])
    for g, r in zip(got.results, ref.results):
        assert (g.a, g.b) == (r.a, r.b)
        np.testing.assert_allclose([g.generations, g.se, g.A, g.c], [r.generations, r.se, r.A, r.c], rtol=1e-12, atol=0.0, equal_nan=True)
    assert np.isfinite(got.results[0].generations) and np.isfinite(got.results[0].se)
    with pytest.raises(RuntimeError, match=r"every weight must be in \[-1, 1\]"):
        ad.wld_curves(xp_d, M, cell, wt * 1.5, nbins, chrom_ranges=ranges)
    with pytest.raises(RuntimeError, match=r"more than 65536: use a larger bin or a smaller --maxdist"):
        ad.wld_curves(torch.zeros((2, 17504), dtype=torch.uint8, device=_dev()), 70000, np.zeros(70000, dtype=np.int32),
                      np.zeros((1, 70000)), 4)


def test_date_command_writes_both_files(tmp_path):
    """The `date` mode in a child process on a tiny BED: {name}.{K}.wld and .date with the stated columns."""
    G, xp, cm, chrom, P, Q, cell, ranges, nbins, wt, want = _panel()
    M = G.shape[1]
    LO.write_bed(str(tmp_path / "tiny"), G, chroms=[str(c) for c in chrom])
    with open(tmp_path / "tiny.bim", "w") as fb:
        for j in range(M):
            fb.write(f"{chrom[j]}\trs{j}\t{float(cm[j])!r}\t{j + 1}\tA\tG\n")      # (repr: the same float64 back)
    np.savetxt(tmp_path / "run.3.P", P)
    np.savetxt(tmp_path / "run.3.Q", Q)
    r = subprocess.run([sys.executable, "-m", "neural_admixture_amd", "date", "--name", "run", "--save_dir", str(tmp_path), "--data_path",
                        str(tmp_path / "tiny.bed"), "--k", "3", "--maxdist", "10", "--out_name", "out"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Admixture date (K=3, components 1-2):" in r.stdout
    wld = (tmp_path / "out.3.wld").read_text().splitlines()
    assert wld[0].split() == ["d_cM", "pairs", "1-2", "1-3", "2-3"] and len(wld) == 1 + nbins
    row = wld[11].split()
    assert len(row) == 5 and float(row[0]) == pytest.approx(0.5) and int(row[1]) == int(want[1][:, 10].sum())
    date = (tmp_path / "out.3.date").read_text().splitlines()
    assert date[0].split() == ["a", "b", "generations", "se", "A", "se_A", "c", "z"] and len(date) == 4
    assert [ln.split()[:2] for ln in date[1:]] == [["1", "2"], ["1", "3"], ["2", "3"]] and all(len(ln.split()) == 8 for ln in date[1:])
