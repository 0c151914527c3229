"""nadm_local_anc on the GPU, through the raw binding, against the float64 restatement of its contract (tests/localanc_oracle.py).

TOLERANCE.  Per case the fp32 restatement's own error against float64 is computed on the CPU (``e32``); the GPU's error against
float64 must be at most ``8 e32 + 1e-6`` for dosage and post: the hardware's reciprocal (1 ulp) and its fused multiply-adds round
differently from numpy's, and 1e-6 is four fp32 ulps of a dosage of 2.  The same rule, relative, for ll, where the relative error of a
value is taken against max(|ll|, 1): an all-missing sample has ll = 0 up to the rounding of its q.
``call`` is compared where float64's two largest pair masses differ by more than 1e-4 (closer than that, fp32 may order them either
way); at most 1 % of the points may be left out so, which every case checks on the CPU's result alone.

The shapes are the smallest that reach each path: rows either side of a wave and of the 256-row tile, M no multiple of 4 or 256
with garbage in the tail bits and pad bytes, segments that start inside a byte and inside a chunk and one of a single SNP, output
points on a segment's first and last SNP and a segment without any, a permuted gather list with a duplicate, q_stride > kp, an
all-missing row, a Q row with exact zeros, rho holding 0 and 1, and one chain of 20000 SNPs."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localanc_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-6
SEG = [0, 5, 258, 259, 1030]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(seed, rows, M, K, seg, zero_q=True):
    """A panel with the edge cases planted: codes [rows, M], P, Q, rho, seg, out_snp, oseg."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.02, 0.98, size=(M, K)).astype(np.float32)
    Q = rng.dirichlet(np.full(K, 0.7), size=rows).astype(np.float32)
    if zero_q and K >= 2 and rows >= 3:
        Q[2] = 0.0                                          # exact zeros in Q
        Q[2, : max(1, K // 2)] = np.float32(1.0 / max(1, K // 2))
    z = rng.integers(0, K, size=(rows, M))
    for j in range(1, M):                                   # ancestry that persists along the row: the data carry linkage
        keep = rng.random(rows) < 0.97
        z[keep, j] = z[keep, j - 1]
    pj = P[np.arange(M)[None, :], z]
    codes = (rng.random((rows, M)) < pj).astype(np.uint8) + (rng.random((rows, M)) < pj).astype(np.uint8)
    codes[rng.random((rows, M)) < 0.05] = 3
    if rows >= 2:
        codes[1] = 3                                        # an all-missing row: its posterior is the prior
    rho = rng.uniform(0.0, 0.2, size=M).astype(np.float32)
    rho[rng.random(M) < 0.03] = 0.0                         # rho holding 0 and 1
    rho[rng.random(M) < 0.03] = 1.0
    out, oseg = [], [0]
    for s in range(len(seg) - 1):
        s0, s1 = seg[s], seg[s + 1]
        if s == 1 and len(seg) > 3:                         # a segment without output points
            pts = []
        else:
            inner = rng.choice(np.arange(s0, s1), size=min(s1 - s0, 6), replace=False).tolist()
            pts = sorted(set(inner + [s0, s1 - 1]))         # on the segment's first and last SNP
        out += pts
        oseg.append(len(out))
    return dict(codes=codes, P=P, Q=Q, rho=rho, seg=np.asarray(seg, np.int32), out_snp=np.asarray(out, np.int32),
                oseg=np.asarray(oseg, np.int32), K=K, M=M)


def _oracles(c, rows=None):
    """(float64, float32) restatements of the listed rows (default all, in order)."""
    sel = np.arange(c["codes"].shape[0]) if rows is None else np.asarray(rows)
    return tuple(LO.local_anc(c["codes"][sel], c["P"], c["Q"][sel], EPS, c["rho"], c["seg"], c["out_snp"], c["oseg"], dtype=dt)
                 for dt in (np.float64, np.float32))


def _device_matrix(codes, ld=None, seed=99):
    """The packed rows on the device, garbage in the tail bits and pad bytes."""
    M = codes.shape[1]
    ld = ld or ((M + 3) // 4 + 15) // 16 * 16
    return torch.from_numpy(LO.pack(codes, ld, np.random.default_rng(seed))).to(_dev())


def _call(xp, c, rows=None, q_stride=None, seg=None, out_snp=None, oseg=None, full=True, ld=None):
    """nadm_local_anc through the raw binding: rows = the gather list (None: rows 0..b of xp, Q rows in that order; else Q row s is
    that of matrix row rows[s]).  Returns (dosage [b, n_out, K], call, post, ll) as numpy, or ll alone when not ``full``."""
    from neural_admixture_amd._lib import lib, check, ptr
    dev = xp.device
    K, M = c["K"], c["M"]
    kp = int(lib.nadm_pad_k(K))
    qs = q_stride or kp
    sel = np.arange(xp.shape[0]) if rows is None else np.asarray(rows)
    b = len(sel)
    Pp = torch.zeros((M, kp), dtype=torch.float32, device=dev)
    Pp[:, :K] = torch.from_numpy(c["P"]).to(dev)
    Qp = torch.full((b, qs), 7.0, dtype=torch.float32, device=dev)          # what lies behind kp is never read
    Qp[:, :kp] = 0.0
    Qp[:, :K] = torch.from_numpy(c["Q"][sel]).to(dev)
    idx = None if rows is None else torch.from_numpy(sel.astype(np.int32)).to(dev)
    seg = c["seg"] if seg is None else np.asarray(seg, np.int32)
    out_snp = c["out_snp"] if out_snp is None else np.asarray(out_snp, np.int32)
    oseg = c["oseg"] if oseg is None else np.asarray(oseg, np.int32)
    n_seg, n_out = len(seg) - 1, len(out_snp)
    rho_d, seg_d = torch.from_numpy(c["rho"]).to(dev), torch.from_numpy(seg).to(dev)
    ll = torch.full((b, n_seg), float("nan"), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ldv = int(ld or xp.stride(0))
    if not full:
        check(lib.nadm_local_anc(ptr(xp), ldv, ptr(idx), b, M, ptr(Pp), K, kp, ptr(Qp), qs, EPS, ptr(rho_d), ptr(seg_d), n_seg, None, None,
                                 0, None, None, None, ptr(ll), None, st), "local_anc")
        torch.cuda.current_stream().synchronize()
        return ll.cpu().numpy()
    out_d, oseg_d = torch.from_numpy(out_snp).to(dev), torch.from_numpy(oseg).to(dev)
    nf = int(lib.nadm_local_anc_scratch_floats(b, n_out, kp))
    assert nf >= n_out * kp * (kp + 1) // 2 * ((b + 255) // 256 * 256) > 0
    scratch = torch.empty(nf, dtype=torch.float32, device=dev)
    dosage = torch.full((b, n_out, kp), -5.0, dtype=torch.float32, device=dev)
    call = torch.full((b, n_out), 77, dtype=torch.uint8, device=dev)
    post = torch.full((b, n_out), -5.0, dtype=torch.float32, device=dev)
    check(lib.nadm_local_anc(ptr(xp), ldv, ptr(idx), b, M, ptr(Pp), K, kp, ptr(Qp), qs, EPS, ptr(rho_d), ptr(seg_d), n_seg, ptr(out_d),
                             ptr(oseg_d), n_out, ptr(dosage), ptr(call), ptr(post), ptr(ll), ptr(scratch), st), "local_anc")
    torch.cuda.current_stream().synchronize()
    d = dosage.cpu().numpy()
    assert (d[:, :, K:] == 0).all() and not np.signbit(d[:, :, K:]).any()   # pad columns +0.0
    return d[:, :, :K], call.cpu().numpy(), post.cpu().numpy(), ll.cpu().numpy()


def _rel(x, ref):
    return np.abs(x - ref) / np.maximum(np.abs(ref), 1.0)


def _hold(got, o64, o32, what):
    """The tolerance rule of the module docstring; prints each figure before it asserts."""
    d, cl, p, ll = got
    assert not np.isnan(o64["dosage"]).any() and not np.isnan(o32["dosage"]).any(), what
    e_d = float(np.abs(o32["dosage"].astype(np.float64) - o64["dosage"]).max())
    e_p = float(np.abs(o32["post"].astype(np.float64) - o64["post"]).max())
    e_l = float(_rel(o32["ll"], o64["ll"]).max())
    g_d = float(np.abs(d.astype(np.float64) - o64["dosage"]).max())
    g_p = float(np.abs(p.astype(np.float64) - o64["post"]).max())
    g_l = float(_rel(ll, o64["ll"]).max())
    clear = o64["gap"] > 1e-4
    left_out = 1.0 - float(clear.mean())
    print(f"{what}: dosage gpu {g_d:.3e} fp32 {e_d:.3e}; post gpu {g_p:.3e} fp32 {e_p:.3e}; ll(rel) gpu {g_l:.3e} fp32 {e_l:.3e}; "
          f"calls left out {left_out:.4f}")
    assert left_out <= 0.01, what                            # (of the oracle alone: the seed's choice)
    assert not np.isnan(d).any() and not np.isnan(p).any() and d.min() >= 0.0 and d.max() <= 2.0, what
    assert g_d <= 8.0 * e_d + 1e-6, what
    assert g_p <= 8.0 * e_p + 1e-6, what
    assert g_l <= 8.0 * e_l + 1e-6, what
    assert (cl[clear] == o64["call"][clear]).all(), what
    assert cl.max() < c_pairs(o64["dosage"].shape[2]), what


def c_pairs(K):
    return K * (K + 1) // 2


# ---- against the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 12, 16])
def test_every_width_against_float64(K):
    """65 rows x 1030 SNPs in the four segments, through a permuted gather list with a duplicate and q_stride > kp."""
    c = _case(100 + K, 65, 1030, K, SEG)
    rng = np.random.default_rng(K)
    rows = rng.permutation(65)
    rows = np.concatenate([rows, rows[:1]])                 # a duplicate: a sample of its own
    xp = _device_matrix(c["codes"])
    o64, o32 = _oracles(c, rows)
    got = _call(xp, c, rows=rows, q_stride=int(np.ceil(K / 4) * 4) + 8)
    _hold(got, o64, o32, f"K={K}")
    # the all-missing row: the posterior is the prior q_x q_y -- in float64, which _hold has just held the GPU to.  The fp32 row of Q
    # sums to 1 within u = K 2^-24, which moves a dosage by at most 4 u and a step's ln S by at most 2 u
    s = int(np.nonzero(rows == 1)[0][0])
    q, u = c["Q"][1].astype(np.float64), 16 * 2.0 ** -24
    assert np.abs(o64["dosage"][s] - 2.0 * q[None, :]).max() <= 4 * u and np.abs(o64["ll"][s]).max() <= 2 * u * 1030


@pytest.mark.parametrize("rows,M,K", [(1, 17, 3), (63, 259, 4), (257, 259, 3), (300, 1030, 2), (65, 17, 8)])
def test_rows_and_lengths_against_float64(rows, M, K):
    seg = [s for s in SEG if s < M] + [M]
    c = _case(7 * rows + M, rows, M, K, seg)
    o64, o32 = _oracles(c)
    _hold(_call(_device_matrix(c["codes"]), c), o64, o32, f"rows={rows} M={M} K={K}")


def test_long_chain_against_float64():
    """One segment of 20000 SNPs at 65 rows, with a Q row of exact zeros whose calls disagree with it: no NaN, and the error has not
    grown with the chain."""
    c = _case(5, 65, 20000, 2, [0, 20000])
    c["codes"][2] = np.where(c["P"][:, 1] > 0.5, 2, 0)      # Q[2] = (1, 0): calls drawn from the OTHER component
    c["out_snp"] = np.asarray([0, 1, 4999, 10000, 15000, 19998, 19999], np.int32)
    c["oseg"] = np.asarray([0, 7], np.int32)
    o64, o32 = _oracles(c)
    _hold(_call(_device_matrix(c["codes"]), c), o64, o32, "long chain")


# ---- exact properties -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    c = _case(11, 300, 1030, 5, SEG)
    xp = _device_matrix(c["codes"])
    return c, xp, _call(xp, c)


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, i)


def test_two_runs_give_the_same_bits():
    c, xp, first = _batch()
    _same(_call(xp, c), first, "second run")


def test_a_sample_alone_gives_the_bits_of_its_place_in_the_batch():
    c, xp, whole = _batch()
    for r in (0, 63, 64, 255, 256, 299):
        alone = _call(xp, c, rows=[r])
        _same(alone, tuple(o[r:r + 1] for o in whole), f"row {r}")
    sub = [299, 5, 256, 5]                                  # and through a list, at other positions, next to other rows
    _same(_call(xp, c, rows=sub), tuple(o[sub] for o in whole), "a list")


def test_segments_in_one_call_give_the_bits_of_one_call_per_segment():
    c, xp, whole = _batch()
    for s in range(len(SEG) - 1):
        a, b = int(c["oseg"][s]), int(c["oseg"][s + 1])
        if b == a:                                          # no output points: the forward pass is all there is
            ll = _call(xp, c, seg=SEG[s:s + 2], full=False)
            assert ll.tobytes() == whole[3][:, s:s + 1].tobytes()
            continue
        d, cl, p, ll = _call(xp, c, seg=SEG[s:s + 2], out_snp=c["out_snp"][a:b], oseg=[0, b - a])
        _same((d, cl, p, ll), (whole[0][:, a:b], whole[1][:, a:b], whole[2][:, a:b], whole[3][:, s:s + 1]), f"segment {s}")


def test_forward_only_ll_equals_the_full_call():
    c, xp, whole = _batch()
    assert _call(xp, c, full=False).tobytes() == whole[3].tobytes()


def test_row_offsets_past_4_gib_and_a_side_stream():
    """136 rows at ld = 2^25: rows 64.. start beyond 2^31 bytes, rows 128.. beyond 2^32 (address space, barely touched); the call runs
    on a side stream.  The compact rows' bits, which test_every_width_against_float64's shapes hold to the oracle."""
    rows, ld = 136, 1 << 25
    free, _ = torch.cuda.mem_get_info()
    assert free > rows * ld + (2 << 30), "4.25 GiB + 2 GiB of free HBM are needed"
    c = _case(21, rows, 1030, 8, SEG)
    o64, o32 = _oracles(c)
    compact = _device_matrix(c["codes"])
    want = _call(compact, c)
    _hold(want, o64, o32, "compact rows")
    big = torch.empty((rows, ld), dtype=torch.uint8, device=_dev())
    big[:, :4096] = 0xFF
    big[:, : compact.shape[1]] = compact
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _call(big, c)
        sel = [135, 0, 64, 128, 127]
        part = _call(big, c, rows=sel)
    _same(got, want, "wide rows")
    _same(part, tuple(o[sel] for o in want), "wide rows through a list")


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _panel():
    G, cm, chrom, P, Q, anc = LO.simulate(3, 24, 2, 3000, 0.02, 20.0, K=3)
    M = G.shape[1]
    ld = ((M + 3) // 4 + 15) // 16 * 16
    return G, cm, chrom, P.astype(np.float32), Q.astype(np.float32), anc, torch.from_numpy(LO.pack(G, ld)).to(_dev())


def test_row_blocks_give_the_unblocked_bits_and_the_posterior_finds_the_truth():
    from neural_admixture_amd import localanc
    G, cm, chrom, P, Q, anc, xp = _panel()
    M = G.shape[1]
    # 600 rows through a list: three blocks of 256 rows once the budget is one block's worth
    idx = torch.from_numpy(np.resize(np.arange(24), 600).astype(np.int32)).to(_dev())
    Qi = Q[np.resize(np.arange(24), 600)]
    whole = localanc.local_ancestry(xp, M, P, Qi, cm, chrom, 20.0, idx=idx, dosage=True)
    assert localanc.block_rows(len(whole.out_snp), 3) >= 600
    blocked = localanc.local_ancestry(xp, M, P, Qi, cm, chrom, 20.0, idx=idx, dosage=True, budget=1)
    assert localanc.block_rows(len(whole.out_snp), 3, 1) == 256
    for name in ("call", "post", "ll", "dosage", "share"):
        assert getattr(whole, name).tobytes() == getattr(blocked, name).tobytes(), name
    assert np.allclose(whole.point_share, blocked.point_share, rtol=0, atol=1e-12) and whole.nan_points == 0
    assert whole.dosage[24:48].tobytes() == whole.dosage[:24].tobytes()
    # the posterior dosage against the simulated truth, beside the prior 2 q: a relation, not a threshold
    truth = anc[:, whole.out_snp, :].astype(np.float64)
    mse = float(((whole.dosage[:24] - truth) ** 2).mean())
    prior = float(((2.0 * Q[:, None, :] - truth) ** 2).mean())
    print(f"dosage mse: posterior {mse:.4f}, prior {prior:.4f}")
    assert mse < prior
    # loglik is the forward pass of the same call
    assert localanc.loglik(xp, M, P, Q, cm, chrom, 20.0).tobytes() == whole.ll[:24].tobytes()


def test_scan_generations_lands_between_the_grid_neighbours_of_the_truth():
    """Truth 20 generations; the nine-value grid of the design study has 14 and 28 either side of it."""
    from neural_admixture_amd import localanc
    G, cm, chrom, P, Q, anc, xp = _panel()
    n, grid, lls = localanc.scan_generations(xp, G.shape[1], P, Q, cm, chrom)
    print(f"scan: {n:.2f} generations; grid maximum at {grid[int(np.argmax(lls))]:.2f}")
    assert 14.0 < n < 28.0
    coarse = [2, 5, 10, 14, 20, 28, 40, 80, 200]
    tot = [float(localanc.loglik(xp, G.shape[1], P, Q, cm, chrom, g).sum()) for g in coarse]
    assert coarse[int(np.argmax(tot))] == 20, tot


def test_local_command_writes_its_files(tmp_path):
    """The `local` mode in a child process on a small BED, once with a given number of generations and --target, once with auto."""
    import subprocess
    import ld_oracle as LDO
    from neural_admixture_amd import localanc
    G, cm, chrom, P, Q, anc, xp = _panel()
    N, M = G.shape
    LDO.write_bed(str(tmp_path / "tiny"), G, chroms=[str(c) for c in chrom])
    with open(tmp_path / "tiny.bim", "w") as fb:
        for j in range(M):
            fb.write(f"{chrom[j]}\trs{j}\t{float(cm[j])!r}\t{j + 1}\tA\tG\n")      # (repr: the same float64 back)
    np.savetxt(tmp_path / "run.3.P", P)
    np.savetxt(tmp_path / "run.3.Q", Q)
    (tmp_path / "pops").write_text("".join("A\n" if i % 2 == 0 else "B\n" for i in range(N)))
    base = [sys.executable, "-m", "neural_admixture_amd", "local", "--name", "run", "--save_dir", str(tmp_path), "--data_path",
            str(tmp_path / "tiny.bed"), "--k", "3"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(base + ["--generations", "20", "--out_name", "out", "--dosage", "--pops_path", str(tmp_path / "pops"), "--target", "A"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    pts = localanc.output_points(cm, chrom)[0]
    assert "Local ancestry (K=3, 20 generations): 12 samples at" in r.stdout and "0 of" in r.stdout
    rows = (tmp_path / "out.3.lanc").read_text().splitlines()
    assert len(rows) == len(pts) and rows[0].split()[:4] == ["1", "rs0", "1", "0"] and len(rows[0].split()) == 4 + 12
    assert set(v for ln in rows for v in ln.split()[4:]) <= {"1/1", "1/2", "1/3", "2/2", "2/3", "3/3"}
    sample = (tmp_path / "out.3.lanc.sample").read_text().splitlines()
    assert len(sample) == 13 and len(sample[1].split()) == 1 + 6 + 2
    got = np.asarray([[float(v) for v in ln.split()[1:7]] for ln in sample[1:]])
    assert np.abs(got[:, 0::2].sum(axis=1) - 1.0).max() < 1e-4 and np.abs(got[:, 1::2] - Q[0::2]).max() < 1e-5
    assert len((tmp_path / "out.3.lanc.mean").read_text().splitlines()) == 1 + len(pts)
    assert np.load(tmp_path / "out.3.lanc.dosage.npy").shape == (12, len(pts), 3)
    r = subprocess.run(base, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "--generations auto chose" in r.stdout and "generations: log-likelihood" in r.stdout
    assert len((tmp_path / "run.3.lanc").read_text().splitlines()) == len(pts)
