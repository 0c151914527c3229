"""Two contracts every entry point of the library shares (include/nadm.h, conventions), held for each of them:

A. STRIDE.  The address of row r of a packed matrix is r * ld in 64 bits, for any ld < 2^32.  Every entry point runs on the same rows
   in three placements and every output must be BIT-IDENTICAL to the compact one's:
     compact  [R, row_stride(M)], as every other test has it
     wide     R = 136 rows, ld = 2^25: rows 64.. start beyond 2^31 bytes, rows 128.. beyond 2^32 (4.25 GiB of address space, of which
              the first 4096 bytes of a row are touched: 0xFF, then the compact row over it, so the slack next to the data holds set
              pad bits)
     huge     3 rows, ld = 2^31 (6 GiB): ld itself in [2^31, 2^32), rows at 0, 2^31 and 2^32
   with a gather list (130 rows out of order, rows 0, 63, 64, 127, 128 and 135 and a duplicate among them; huge: rows 2, 0, 1, 2) and
   without one (all 136 rows: rows 128..135 are a ragged third 64-sample tile that lies beyond 2^32; huge: 3 rows).  M = 1027: five
   256-SNP chunks, the last ragged, a partial last byte.  Bit equality would also hold if both calls did nothing, so the compact
   result is held to the float64 oracle of its operation with the bound of that operation's own module (imported, not restated;
   where the bound lives inside a test function its rule is repeated here and says where it is from).  One exception, said where it
   is made: the held-out deviance of the huge matrix's 3 rows, sums of one or two terms, for which test_cv's bound is not made; its
   count is held exactly.  And every output is overwritten with random bytes once it is copied (_taken): the allocator hands its memory
   to the next call's output, where a call that wrote nothing would otherwise find the right answer.
   Writers with a wide OUTPUT (nadm_cv_mask, nadm_pack2bit, nadm_bed_to_packed_dev, nadm_synth_packed): the first row_stride(M) bytes
   of every row equal the compact output, and what the compact form promises about the slack holds up to ld (checked on the device).

B. STREAM.  All device work of a call is issued on the stream it is given.  On a side stream (torch's streams do not block against the
   null stream) a delay kernel runs first; behind it, copies make "live" operands true that until then hold decoys (matrix all 0xFF,
   Q uniform, P 0.5, idx zeros); behind them the entry point is called.  When the call returns on the host the delay must still be
   running (`not marker.query()`: the PREMISE, asserted -- a test whose premise fails, fails), so every launch was enqueued while the
   operands held decoys.  A launch, memset or copy issued on another stream runs during the delay, reads decoys or another call's
   partial sums (a warm-up call with other inputs ran on the side stream before) and changes the bits: every output must be
   bit-identical to the default-stream result.
   The delay is torch.cuda._sleep, calibrated once per session to DELAY_MS = 150 ms with two events.  MEASURED on an MI355X:
   torch.cuda._sleep(359514565) delivers 149.9 ms between two events (printed by the first stream test of a run); the host side of the
   longest protocol, two production steps + infer_q, returns well inside it.  The premise assertion, not the number, is the guard.
   Left out because they synchronise with the host by design: nadm_gmm_fit_means_dev (an EM loop that reads its convergence figure
   back every iteration) and nadm_plan_kernel_ms / nadm_plan_bucket_ms (they wait for the timing events they read).  Wrappers that
   synchronise (report.loglikelihood_hip, ld.select_snps) are replaced by the C call below them.

Every test is marked `gpu`.  A test skips only when torch.cuda.mem_get_info() reports less free memory than its allocations plus
2 GiB; the wide and the huge matrix are never alive at the same time (one arena).  76 tests, 8 s on an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_oracle as BO  # noqa: E402
import cv_oracle as CO  # noqa: E402
import fitcheck_oracle as FO  # noqa: E402
import hwe_oracle as HO  # noqa: E402
import kinship_oracle as KO  # noqa: E402
import ld_oracle as LO  # noqa: E402
import project_oracle as R  # noqa: E402
import project_p_oracle as PO  # noqa: E402
import pse_oracle as PSO  # noqa: E402
from oracle import nadm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

M, K = 1027, 8
ROWS = 136
RS = ((M + 3) // 4 + 127) // 128 * 128                     # ModelLayout.row_stride(M) (asserted in _arena)
WIDE_LD, HUGE_LD, HEAD = 1 << 25, 1 << 31, 4096
SHAPE = {"wide": (ROWS, WIDE_LD), "huge": (3, HUGE_LD)}
MUST = [0, 1, 2, 4, 5, 63, 64, 127, 128, 135]              # the rows either side of 2^31 and 2^32, the last row, the oracles' planted rows
CV = dict(seed=42, folds=5, fold=2, row0=0)
LD_WINDOW = 65
DELAY_MS = 150.0


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from neural_admixture_amd._lib import lib, check, ptr
    return lib, check, ptr


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ data (host, computed once, left unchanged)
@functools.lru_cache(maxsize=None)
def _data(name):
    """(G uint8 [136, M], P float32 [M, K], Q float32 [136, K]) from the builders of the operations' own modules."""
    if name == "edge":
        G, P, Q, _ = HO.make_edge_case(ROWS, M, K)
    elif name == "proj":
        G, P, Q, _ = PO.make_edge_case(ROWS, M, K)
    else:
        G, P, Q = FO.make_panel(ROWS, M, K)
    return np.ascontiguousarray(G), np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)


def _pack(G):
    """Compact rows [N, RS] on the host (pad bits and pad bytes 0)."""
    lib, check, ptr = _lib()
    out = torch.empty((G.shape[0], RS), dtype=torch.uint8)
    check(lib.nadm_pack2bit_host(ptr(torch.from_numpy(np.ascontiguousarray(G))), ptr(out), G.shape[0], G.shape[1], RS), "pack2bit_host")
    return out


@functools.lru_cache(maxsize=None)
def _compact(name):
    return _pack(_data(name)[0])


@functools.lru_cache(maxsize=None)
def _rows(placement, mode):
    """The matrix rows of a case in call order.  list: the gather list; none: rows 0..n."""
    if placement == "huge":
        return np.asarray([2, 0, 1, 2] if mode == "list" else [0, 1, 2], dtype=np.int32)
    if mode == "none":
        return np.arange(ROWS, dtype=np.int32)
    rng = np.random.default_rng(130)
    rest = [int(r) for r in rng.permutation(ROWS) if r not in MUST][:129 - len(MUST)]
    rows = np.asarray(MUST + rest)[rng.permutation(129)]
    rows = np.concatenate([rows, rows[:1]]).astype(np.int32)
    assert len(rows) == 130 and len(set(rows.tolist())) == 129 and set(MUST) <= set(rows.tolist()) and (np.diff(rows) < 0).any()
    return rows


# ------------------------------------------------------------------------------------------------ placements
_ARENA = {"kind": None, "buf": None}


def _room(n_bytes, what):
    free, _ = torch.cuda.mem_get_info()
    if free < n_bytes + (2 << 30):
        pytest.skip(f"{what} needs {n_bytes / 2 ** 30:.2f} GiB + 2 GiB of free HBM, {free / 2 ** 30:.2f} GiB are free")


def _arena(kind):
    """THE big buffer, [136, 2^25] or [3, 2^31] (torch.empty: address space, not touched): one at a time."""
    from neural_admixture_amd.layout import ModelLayout
    assert RS == ModelLayout.row_stride(M) and RS <= HEAD
    if _ARENA["kind"] != kind:
        _ARENA.update(kind=None, buf=None)
        torch.cuda.empty_cache()
        rows, ld = SHAPE[kind]
        _room(rows * ld, f"the {kind} matrix")
        _ARENA.update(kind=kind, buf=torch.empty((rows, ld), dtype=torch.uint8, device=_dev()))
    buf = _ARENA["buf"]
    ld = buf.shape[1]
    assert buf.is_contiguous() and buf.stride(0) == ld and ld % 16 == 0 and ld < 1 << 32
    if kind == "wide":
        assert 63 * ld < 2 ** 31 <= 64 * ld and 127 * ld < 2 ** 32 <= 128 * ld and buf.shape[0] == ROWS
    else:
        assert 2 ** 31 <= ld < 2 ** 32 and [r * ld for r in range(3)] == [0, 2 ** 31, 2 ** 32]
    return buf


def _placed(kind, compact_host):
    """The rows of ``compact_host`` (its first 3 for huge) in the placement ``kind``, on the device."""
    if kind == "compact":
        return compact_host.to(_dev())
    buf = _arena(kind)
    src = compact_host[: buf.shape[0]].to(_dev())
    buf[:, :HEAD] = 0xFF
    buf[:, : src.shape[1]] = src
    return buf


def _compact_of(kind, compact_host):
    return compact_host if kind != "huge" else compact_host[:3].contiguous()


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _taken(out):
    """Copies of a call's outputs; the outputs themselves are then overwritten with random bytes.  The allocator hands their memory to
    the NEXT call's outputs: a call that wrote nothing would otherwise return the previous call's (right) answer."""
    res = tuple(o.clone() for o in out)
    for o in out:
        o.view(torch.uint8).random_(0, 256)
    return res


def _assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i)
        if _bits(g) != _bits(w):
            a, b = g.detach().cpu().numpy().reshape(-1), w.detach().cpu().numpy().reshape(-1)
            bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0]
            raise AssertionError(f"{what}: output {i} differs in {len(set(bad.tolist()))} of {len(a)} entries, the first at flat index {int(bad[0])}: "
                                 f"{a[bad[0]]!r} != {b[bad[0]]!r}")


# ------------------------------------------------------------------------------------------------ the entry points (t: dict of device operands)
def _n(t):
    return int(t["idx"].numel()) if t.get("idx") is not None else int(t["xp"].shape[0])


def _padded(t):
    from neural_admixture_amd._packed import pad_P, pad_Q
    dev = t["xp"].device
    Pp = pad_P(t["P"], dev)
    return Pp, pad_Q(t["Q"], _n(t), K, int(Pp.shape[1]), dev)


def _op_project_q(t):
    from neural_admixture_amd import project
    lib, _, _ = _lib()
    n, dev = _n(t), t["xp"].device
    Pp, qin = _padded(t)
    qout = torch.empty_like(qin)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    no = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(lib.nadm_project_scratch_floats(n, M, Pp.shape[1])), 4), dtype=torch.float32, device=dev)
    project.em_step(t["xp"], M, t.get("idx"), n, Pp, K, qin, qout, scratch, R.EPS, R.QMIN, ll, no, weights=t.get("w"))
    return qout, ll, no


def _op_project_p(t):
    from neural_admixture_amd import project
    lib, _, _ = _lib()
    n, dev = _n(t), t["xp"].device
    pin, Qp = _padded(t)
    pout = torch.empty_like(pin)
    no = torch.empty(M, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(lib.nadm_project_p_scratch_floats(n, M, pin.shape[1])), 4), dtype=torch.float32, device=dev)
    project.p_step(t["xp"], M, t.get("idx"), n, Qp, K, pin, pout, scratch, PO.EPS, PO.PMIN, no)
    return pout, no


def _op_kinship(t):
    from neural_admixture_amd import relate
    Pp, Qp = _padded(t)
    return relate.kinship_block(t["xp"], M, Pp, K, t.get("idx"), Qp, t.get("idx"), Qp)


def _op_snp_hwe(t):
    from neural_admixture_amd import hwe
    return hwe.snp_hwe_sums(t["xp"], M, t["P"], t["Q"], t.get("idx"))


def _op_snp_info(t):
    from neural_admixture_amd import pse
    return pse.p_info(t["xp"], M, t["P"], t["Q"], t.get("idx"))


def _op_em_sums(t):
    from neural_admixture_amd import fitcheck
    return fitcheck.em_sums(t["xp"], M, t["P"], t["Q"], t.get("idx"))


def _op_resid_cor(t):
    from neural_admixture_amd import fitcheck
    Pp, Qp = _padded(t)
    return fitcheck.resid_cor_block(t["xp"], M, Pp, K, t.get("idx"), Qp, t.get("idx"), Qp, t["B"], t["C"])


def _op_snp_counts(t):
    from neural_admixture_amd import ld
    return (ld.snp_counts(t["xp"], M, t.get("idx")),)


def _op_ld_band(t):
    from neural_admixture_amd import ld
    return ld.ld_band(t["xp"], M, LD_WINDOW, 0, None, t.get("idx"), with_moments=True)


def _op_cv_deviance(t):
    from neural_admixture_amd import cv
    return cv.heldout_deviance(t["xp"], M, t["P"], t["Q"], CV["fold"], CV["folds"], CV["seed"], row0=CV["row0"])


def _op_loglik(t):
    lib, check, ptr = _lib()
    xp = t["xp"]
    part = torch.empty(int(lib.nadm_loglik_blocks(M)), dtype=torch.float64, device=xp.device)
    check(lib.nadm_loglik(ptr(xp), xp.shape[1], xp.shape[0], M, ptr(t["P"]), ptr(t["Q"]), K, K, 1e-6, ptr(part), _st()), "loglik")
    return (part,)


def _class_start(n):
    return np.asarray([0, n // 3, n - n // 4, n], dtype=np.int64)          # three classes of different sizes


def _op_class_sums(t):
    lib, check, ptr = _lib()
    xp, n = t["xp"], _n(t)
    sums = torch.zeros((3, M), dtype=torch.int32, device=xp.device)
    start = _class_start(n)
    check(lib.nadm_class_sums(ptr(xp), xp.shape[1], xp.shape[0], M, ptr(t["idx"]), start.ctypes.data_as(C.POINTER(C.c_int64)), 3, ptr(sums),
                              _st()), "class_sums")
    return (sums,)


def _op_unpack2bit(t):
    lib, check, ptr = _lib()
    xp = t["xp"]
    out = torch.empty((xp.shape[0], M), dtype=torch.uint8, device=xp.device)
    check(lib.nadm_unpack2bit(ptr(xp), ptr(out), xp.shape[0], M, xp.shape[1], _st()), "unpack2bit")
    return (out,)


@functools.lru_cache(maxsize=None)
def _keep():
    mask = np.random.default_rng(11).random(M) < 0.6
    mask[[0, 1025]] = True                                   # the first SNP and one of the ragged last chunk
    if mask.sum() % 4 == 0:
        mask[7] = not mask[7]                                # a partial last byte in the output too
    keep = np.nonzero(mask)[0].astype(np.int64)
    assert keep[-1] >= 1024 and len(keep) % 4 != 0 and 256 < len(keep) < M
    return keep


def _op_select_snps(t):
    lib, check, ptr = _lib()
    xp, m_out = t["xp"], int(t["keep"].numel())
    ld_out = ((m_out + 3) // 4 + 127) // 128 * 128
    out = torch.empty((xp.shape[0], ld_out), dtype=torch.uint8, device=xp.device)
    check(lib.nadm_select_snps(ptr(xp), xp.shape[1], xp.shape[0], ptr(t["keep"]), m_out, 1, ptr(out), ld_out, _st()), "select_snps")
    return (out,)


def _op_encode_fwd(t, pca=False):
    lib, check, ptr = _lib()
    xp, n = t["xp"], _n(t)
    chunks = int(lib.nadm_encode_chunks(M))
    zpart = torch.empty(chunks * n * 8, dtype=torch.float32, device=xp.device)
    fold = torch.empty(n * 8, dtype=torch.float32, device=xp.device)
    fn = lib.nadm_pca_project if pca else lib.nadm_encode_fwd
    check(fn(ptr(xp), xp.shape[1], ptr(t["idx"]), n, M, ptr(t["V"]), 8, ptr(zpart), _st()), "encode_fwd")
    check(lib.nadm_sum_rows(ptr(zpart), chunks, n * 8, ptr(fold), _st()), "sum_rows")
    return zpart, fold


def _op_pca_project(t):
    return _op_encode_fwd(t, pca=True)


def _op_pca_project_t(t):
    lib, check, ptr = _lib()
    xp, n = t["xp"], _n(t)
    yimg = torch.empty(int(lib.nadm_dz_image_bytes(n)), dtype=torch.uint8, device=xp.device)
    out = torch.empty((M, 8), dtype=torch.float32, device=xp.device)
    check(lib.nadm_dz_image(ptr(t["Y"]), n, 8, ptr(yimg), _st()), "dz_image")
    check(lib.nadm_pca_project_t(ptr(xp), xp.shape[1], ptr(t["idx"]), n, M, ptr(t["Y"]), ptr(yimg), 8, ptr(out), _st()), "pca_project_t")
    return (out,)


# ------------------------------------------------------------------------------------------------ the oracles (float64; the bounds are the modules' own)
def _ratio_print(what, **figs):
    print(what + ": " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))


def _chk_project_q(got, G, P, Q, x, what):
    import test_project_q as TQ
    q, ll, n = got[0][:, :K], got[1], got[2]
    assert not got[0][:, K:].any()
    if "w" in x:
        q64, ll64, n64 = BO.em_step_w(G, P, Q, x["w"])
        _, ll32, _ = BO.em_step_w(G, P, Q, x["w"], dtype=np.float32)
        nz = ll64 != 0.0
        e32 = float((np.abs(ll32 - ll64)[nz] / np.abs(ll64[nz])).max()) if nz.any() else 0.0
        tol = max(8.0 * e32, 1e-6)                           # test_bootstrap.test_one_weighted_step_against_float64's rule
    else:
        q64, ll64, n64 = R.em_step(G, P, Q)
        tol, _ = TQ._ll_tol(G, P, Q, ll64)
    dq = float(np.abs(q - q64).max())
    _ratio_print(what, dq=dq, ll_tol=tol)
    assert np.array_equal(n, n64) and dq <= 1e-6             # test_project_q.test_one_step_against_float64's bounds
    assert (np.abs(ll - ll64) <= tol * np.abs(ll64)).all()
    assert (ll[n64 == 0] == 0.0).all() and np.array_equal(q[n64 == 0], Q[n64 == 0]) and (n64 > 0).any()


def _chk_project_p(got, G, P, Q, x, what):
    p, n = got[0][:, :K], got[1]
    p64, n64 = PO.p_step(G, P, Q)
    dp = float(np.abs(p - p64).max())
    _ratio_print(what, dp=dp)
    assert np.array_equal(n, n64) and dp <= 1e-6 and not got[0][:, K:].any()      # test_project_p.test_one_step_against_float64's bounds
    assert p[n64 == 0].tobytes() == P[n64 == 0].tobytes() and (n64 > 0).any()


def _chk_kinship(got, G, P, Q, x, what):
    import test_kinship as TK
    t = KO.terms(G, P, Q, 0.0)
    want = KO.from_terms(t, t)
    TK._check_block(got, want, what)
    assert want[2].any()


def _chk_snp_hwe(got, G, P, Q, x, what):
    import test_hwe as TH
    want = HO.sums(G, P, Q)
    TH._check_sums(got, want, TH.TOL_U, TH.TOL_H, what)
    assert want[2].any()


def _chk_snp_info(got, G, P, Q, x, what):
    import test_p_se as TP
    want = PSO.info(G, P, Q)
    TP._check_info(got, want, TP.TOL, what)
    assert want[1].any()


def _chk_em_sums(got, G, P, Q, x, what):
    import test_fitcheck as TF
    Bd, Cd = got
    B64, C64 = FO.em_sums(G, P, Q)
    assert not Bd[:, K:].any() and not Cd[:, K:].any() and (B64 > 0).any()
    for name, g, w in (("B", Bd[:, :K], B64), ("C", Cd[:, :K], C64)):      # test_fitcheck.test_em_sums_against_float64's bound
        assert (np.abs(g - w) <= TF.TOL_SUMS * w).all(), name
        assert (g[w == 0] == 0).all()


def _chk_resid_cor(got, G, P, Q, x, what):
    import test_fitcheck as TF
    want = FO.resid_cor_block(G, G, P, Q, Q, x["B"][:, :K], x["C"][:, :K])
    TF._check_block(got, want, what)
    assert want["n"].any()


def _chk_snp_counts(got, G, P, Q, x, what):
    assert np.array_equal(got[0], LO.counts(G)) and got[0].any()


def _chk_ld_band(got, G, P, Q, x, what):
    r2w, momw = LO.band(G, LD_WINDOW - 1)
    assert np.array_equal(got[1], momw) and got[0].tobytes() == r2w.tobytes()     # test_ld.test_band_bit_for_bit: the bits
    assert momw.any()


def _chk_cv_deviance(got, G, P, Q, x, what):
    import test_cv as TC
    F = CO.folds_of(CV["seed"], CV["row0"] + np.arange(G.shape[0]), M, CV["folds"])
    want = CO.deviance(G, P, Q, F, CV["fold"])
    assert want[1].any() and np.array_equal(got[1], want[1])
    if G.shape[0] <= 4:
        # the huge matrix's 3 rows: a SNP's sum has one term or two.  test_cv's bound is relative to sum |d|, and a single heterozygous
        # call at pi near 1/2 has d = -2 ln(4 r u) ~ 8 (pi - 1/2)^2 next to nothing while the kernel's error stays an ulp of log2: the
        # ratio reached 0.30 here (test_cv keeps its own bound for b = 1 for that reason, and it does not fit either).  The count is
        # exact, the deviance is held on the 136 rows of the wide case; here it must be finite, and exactly 0 where nothing is held out.
        assert np.isfinite(got[0]).all() and (got[0][want[1] == 0] == 0).all() and got[0].any()
        return
    TC._check_dev(got, want, TC.TOL, what)


def _chk_loglik(got, G, P, Q, x, what):
    ref = O.loglikelihood(G, P, Q)
    val = float(got[0].sum())
    assert ref != 0.0 and abs(val - ref) <= 1e-11 * abs(ref)  # test_gpu_parity.test_loglikelihood_kernel_matches_float64_oracle's bound


def _chk_class_sums(got, G, P, Q, x, what):
    start = _class_start(G.shape[0])
    want = np.stack([G[start[c]:start[c + 1]].astype(np.int64).sum(axis=0) for c in range(3)])
    assert np.array_equal(got[0].astype(np.int64), want) and want.any()


def _chk_unpack2bit(got, G, P, Q, x, what):
    assert np.array_equal(got[0], G)


def _chk_select_snps(got, G, P, Q, x, what):
    sel = G[:, _keep()]
    sel = np.where(sel == 0, 2, np.where(sel == 2, 0, sel)).astype(np.uint8)      # flip = 1: 0 <-> 2, 1 and 3 stay
    ref = O.pack2bit(sel)
    assert np.array_equal(got[0][:, :ref.shape[1]], ref) and not got[0][:, ref.shape[1]:].any()


def _mx(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def _chk_encode_fwd(got, G, P, Q, x, what):
    Z = got[1].reshape(G.shape[0], 8)
    want = O.decode_x(G).astype(np.float64) @ x["V"].astype(np.float64)
    _ratio_print(what, dZ=_mx(Z, want))
    assert np.abs(want).max() > 0.1 and _mx(Z, want) < 1e-5   # test_gpu_parity.test_step_against_oracle_random_shapes' bound on Z


def _chk_pca_project(got, G, P, Q, x, what):
    Z = got[1].reshape(G.shape[0], 8)
    ref = (G.astype(np.float64) / 2) @ x["V"].astype(np.float64)
    assert _mx(Z, ref) < 2e-6 * max(1.0, float(np.abs(ref).max()))      # test_gpu_parity.test_pca_projection_on_gpu_...'s bound


def _chk_pca_project_t(got, G, P, Q, x, what):
    ref = (G.astype(np.float64) / 2).T @ x["Y"].astype(np.float64)
    assert _mx(got[0], ref) < 2e-6 * float(np.abs(ref).max())           # test_gpu_parity.test_rsvd_through_hip_kernels_...'s bound (both sides halved)


# name -> (data set, the C entry points it reaches, fn, oracle check, needs a list, has a no-list-only ABI, extra operands)
OPS = {
    "project_q":     ("proj", _op_project_q, _chk_project_q, False, False, ()),
    "project_q_w":   ("proj", _op_project_q, _chk_project_q, False, False, ("w",)),
    "project_p":     ("proj", _op_project_p, _chk_project_p, False, False, ()),
    "kinship":       ("edge", _op_kinship, _chk_kinship, False, False, ()),
    "snp_counts":    ("edge", _op_snp_counts, _chk_snp_counts, False, False, ()),
    "ld_band":       ("edge", _op_ld_band, _chk_ld_band, False, False, ()),
    "select_snps":   ("edge", _op_select_snps, _chk_select_snps, False, True, ("keep",)),
    "snp_hwe":       ("edge", _op_snp_hwe, _chk_snp_hwe, False, False, ()),
    "cv_deviance":   ("edge", _op_cv_deviance, _chk_cv_deviance, False, True, ()),
    "snp_info":      ("edge", _op_snp_info, _chk_snp_info, False, False, ()),
    "em_sums":       ("fit", _op_em_sums, _chk_em_sums, False, False, ()),
    "resid_cor":     ("fit", _op_resid_cor, _chk_resid_cor, False, False, ("B", "C")),
    "loglik":        ("edge", _op_loglik, _chk_loglik, False, True, ()),
    "class_sums":    ("edge", _op_class_sums, _chk_class_sums, True, False, ()),
    "unpack2bit":    ("edge", _op_unpack2bit, _chk_unpack2bit, False, True, ()),
    "encode_fwd":    ("edge", _op_encode_fwd, _chk_encode_fwd, True, False, ("V",)),
    "pca_project":   ("edge", _op_pca_project, _chk_pca_project, True, False, ("V",)),
    "pca_project_t": ("edge", _op_pca_project_t, _chk_pca_project_t, True, False, ("Y",)),
}


@functools.lru_cache(maxsize=None)
def _fit_sums():
    """B, C [M, kp] of the "fit" panel over ALL its 136 rows (numpy, from the library on the compact matrix): operands of resid_cor."""
    from neural_admixture_amd import fitcheck
    G, P, Q = _data("fit")
    B, Cc = fitcheck.em_sums(_compact("fit").to(_dev()), M, P, Q)
    torch.cuda.synchronize()
    return B.cpu().numpy(), Cc.cpu().numpy()


def _host_operands(name, placement, mode):
    """(host operands of the case without the matrix, the genotypes / Q of its rows in call order).  A no-list call of an entry point
    that demands a list gets the list 0..n."""
    data, _, _, needs_list, no_list_abi, extra = OPS[name]
    G, P, Q = _data(data)
    rows = _rows(placement, mode)
    if name == "class_sums" and placement == "huge":
        rows = rows[:3]                                      # (the call takes no more listed rows than the matrix has: 2, 0, 1 without the duplicate)
    x = {"P": P, "Q": np.ascontiguousarray(Q[rows])}
    if mode == "list" or needs_list:
        x["idx"] = rows.copy()
    rng = np.random.default_rng(len(name) + len(rows))
    for e in extra:
        if e == "w":
            import test_bootstrap as TB
            x["w"] = TB._weights(M)
        elif e == "keep":
            x["keep"] = _keep()
        elif e == "V":
            Vm = np.zeros((M, 8), dtype=np.float32)
            Vm[:, :] = rng.standard_normal((M, 8)) / np.sqrt(M)
            x["V"] = Vm
        elif e == "Y":
            x["Y"] = rng.standard_normal((len(rows), 8)).astype(np.float32)
        elif e in ("B", "C"):
            x["B"], x["C"] = _fit_sums()
    return x, np.ascontiguousarray(G[rows])


def _to_dev(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(_dev()) for k, v in x.items()}


def _modes(name):
    return ("none",) if OPS[name][4] else ("list", "none")


def _run_np(name, xp, x):
    t = dict(_to_dev(x), xp=xp)
    res = _taken(OPS[name][1](t))
    torch.cuda.synchronize()
    return res


# ================================================================================================ part A: stride
@pytest.mark.parametrize("name", list(OPS))
@pytest.mark.parametrize("placement", ["wide", "huge"])
def test_stride(name, placement):
    """The entry point on the compact rows against its float64 oracle, then on the same rows in the wide / huge placement: every
    output bit-identical, with a gather list and without one."""
    data, fn, chk, _, _, _ = OPS[name]
    ch = _compact_of(placement, _compact(data))
    for mode in _modes(name):
        x, G = _host_operands(name, placement, mode)
        want = _run_np(name, ch.to(_dev()), x)
        what = f"{name} compact({placement}) rows={mode} n={len(G)}"
        chk(tuple(w.cpu().numpy() for w in want), G, x["P"], x["Q"], x, what)
        xp = _placed(placement, _compact(data))
        assert xp.shape[1] == SHAPE[placement][1] and xp.shape[0] == ch.shape[0]
        got = _run_np(name, xp, x)
        _assert_same_bits(got, want, f"{name} {placement} rows={mode}")


# ------------------------------------------------------------------------------------------------ writers with a wide output
def _slack_is_zero(out):
    return int(out[:, RS:].max()) == 0


def _bed_of(G):
    """PLINK .bed bytes [M, ceil(N/4)] whose conversion gives G (codes 0, 1, 2, 3 <- PLINK 3, 2, 0, 1), and the host converter's result."""
    lib, check, ptr = _lib()
    N = G.shape[0]
    nb = (N + 3) // 4
    codes = np.zeros((M, nb * 4), dtype=np.uint8)
    codes[:, :N] = np.asarray([3, 2, 0, 1], dtype=np.uint8)[G.T]
    bed = np.ascontiguousarray(codes[:, 0::4] | (codes[:, 1::4] << 2) | (codes[:, 2::4] << 4) | (codes[:, 3::4] << 6)).astype(np.uint8)
    ref = torch.full((N, RS), 255, dtype=torch.uint8)
    c4, fl = (C.c_int64 * 4)(), C.c_int32(0)
    check(lib.nadm_bed_to_packed(C.c_void_p(bed.ctypes.data), N, M, ptr(ref), RS, c4, 1, C.byref(fl)), "bed_to_packed")
    return bed, ref.numpy(), [int(c4[i]) for i in range(4)], int(fl.value)


def _w_pack2bit(t, out):
    lib, check, ptr = _lib()
    check(lib.nadm_pack2bit(ptr(t["G"]), ptr(out), out.shape[0], M, out.shape[1], _st()), "pack2bit")
    return ()


def _w_bed(t, out):
    lib, check, ptr = _lib()
    cnt = torch.empty(4, dtype=torch.int64, device=out.device)
    flp = torch.empty(1, dtype=torch.int32, device=out.device)
    check(lib.nadm_bed_to_packed_dev(ptr(t["bed"]), out.shape[0], M, ptr(out), out.shape[1], ptr(cnt), 1, ptr(flp), _st()), "bed_to_packed_dev")
    return cnt, flp


def _w_synth(t, out):
    lib, check, ptr = _lib()
    check(lib.nadm_synth_packed(ptr(out), out.shape[0], 7, M, out.shape[1], ptr(t["Qt"]), ptr(t["Fq"]), K, 0.05, 77, _st()), "synth_packed")
    return ()


def _w_cv_mask(t, out):
    from neural_admixture_amd import cv
    cv.mask_fold(t["xp"], M, CV["fold"], CV["folds"], CV["seed"], out=out, row0=CV["row0"])
    return ()


def _writer_operands(name):
    G, P, Q = _data("edge")
    if name == "pack2bit":
        return {"G": G}
    if name == "bed":
        return {"bed": _bed_of(G)[0]}
    if name == "synth":
        return {"Qt": Q, "Fq": np.ascontiguousarray(P.T)}
    return {}


WRITERS = {"pack2bit": _w_pack2bit, "bed": _w_bed, "synth": _w_synth, "cv_mask": _w_cv_mask}


def _chk_writer(name, out, extra):
    """The compact output against the host form of the operation (bytes: equal)."""
    G, P, Q = _data("edge")
    if name == "pack2bit":
        assert np.array_equal(out, _compact("edge").numpy())
    elif name == "bed":
        _, ref, c4, fl = _bed_of(G)
        assert np.array_equal(out, ref) and [int(v) for v in extra[0]] == c4 and int(extra[1][0]) == fl and fl == 1
    elif name == "cv_mask":
        want = CO.mask_packed(_compact("edge").numpy(), M, CV["seed"], CV["folds"], CV["fold"], CV["row0"])
        assert np.array_equal(out, want) and not np.array_equal(out, _compact("edge").numpy())
    else:                                                    # synth: a generator, no oracle: calls of all four codes, the pad bits and bytes 0
        codes = np.stack([(out >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(out.shape[0], -1)
        assert all((codes[:, :M] == c).any() for c in range(4)) and not codes[:, M:].any()
        assert len({codes[r, :M].tobytes() for r in range(out.shape[0])}) == out.shape[0]


@pytest.mark.parametrize("name", list(WRITERS))
def test_stride_of_a_wide_output(name):
    """nadm_pack2bit, nadm_bed_to_packed_dev, nadm_synth_packed and nadm_cv_mask (input wide too) writing rows 2^25 bytes apart: the
    first row_stride(M) bytes of every row equal the compact output; pack2bit, bed_to_packed_dev and synth_packed write zeros up to
    ld, cv_mask copies every other bit of its input."""
    dev = _dev()
    t = _to_dev(_writer_operands(name))
    if name == "cv_mask":
        t["xp"] = _compact("edge").to(dev)
    small = torch.full((ROWS, RS), 0xAA, dtype=torch.uint8, device=dev)
    extra = _taken(WRITERS[name](t, small))
    torch.cuda.synchronize()
    _chk_writer(name, small.cpu().numpy(), tuple(e.cpu().numpy() for e in extra))
    if name == "cv_mask":
        t["xp"] = _placed("wide", _compact("edge"))
        _room(ROWS * WIDE_LD, "the wide output of cv_mask")
        out = torch.empty((ROWS, WIDE_LD), dtype=torch.uint8, device=dev)
    else:
        out = _arena("wide")
    out[:, :HEAD] = 0xAA
    extra_w = WRITERS[name](t, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :RS], small)
    _assert_same_bits(extra_w, extra, f"{name}: by-products")
    if name == "cv_mask":                                    # every bit that holds no call of the fold is copied: the slack too, in pieces of 4 MiB a row
        step = 1 << 22
        assert all(torch.equal(out[:, max(c, RS): c + step], t["xp"][:, max(c, RS): c + step]) for c in range(0, WIDE_LD, step))
    else:
        assert _slack_is_zero(out)
    del out


# ------------------------------------------------------------------------------------------------ the step: Engine(ld=...)
CFG = {"mfma": dict(ks=[8], C=8, Hd=64), "wide_model": dict(ks=[20], C=12, Hd=64)}


@functools.lru_cache(maxsize=None)
def _step_G():
    return O.synth_genotypes(ROWS, M, 6, seed=417, missing=0.05)


def _step_params(cfg):
    c = CFG[cfg]
    rng = np.random.default_rng(5 + len(cfg))
    V0 = (rng.standard_normal((M, c["C"])) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.02, 0.98, size=(sum(c["ks"]), M)).astype(np.float32)
    return O.make_params(31, V0, P0, c["Hd"], c["ks"])


def _engine(cfg, xp):
    import neural_admixture_amd as na
    from test_gpu_parity import small_vec
    c, p = CFG[cfg], _step_params(cfg)
    e = na.Engine(M, c["C"], c["Hd"], c["ks"], _dev(), ROWS, ld=int(xp.shape[1]))
    assert e.ld == xp.shape[1]
    e._load = lambda: e.load_params(p.V, np.concatenate([Pm.T for Pm in p.P], axis=0), small_vec(p))
    e._load()
    e.set_packed(xp)
    return e


def _phases(e, idx, b):
    """forward + backward (nadm_encode_fwd, nadm_mlp_fwd*, nadm_decode_bce_images or nadm_decode_bce, nadm_mlp_bwd*, nadm_encode_bwd),
    then pass 3 once more, which now reads the resident matrix and not the batch copy pass 2 left, then the backward once more without
    Q's operand images."""
    L = e.lay
    e.forward(idx, b)
    e.backward(idx, b, True)
    first = e.gflat.clone()
    e.encode_backward(idx, b)
    out = (e.zpart[: L.enc_chunks * b * L.CP].clone(), e.Z.clone(), e._Q.clone(), e.dqpart.clone(), e._dZ.clone(), first, e.gflat.clone(),
           e.loss_acc.clone())
    e.invalidate_q()                                         # Q's operand images dropped: pass 2 of C <= 8 is now nadm_decode_bce_gather, and the loss clamps
    e.backward(idx, b, True)
    return (*out, e.dqpart.clone(), e._dZ.clone(), e.gflat.clone(), e.loss_acc.clone())


def _steps(e, idx, b):
    """Two production steps (nadm_step) and the encoder-only pass (nadm_plan_infer)."""
    for _ in range(2):
        e.train_step(idx, b, 2e-3, True)
    qs = e.infer_q(idx, b)
    small = e.small                                          # (settles what the last step left to the next one)
    return (e.pflat.clone(), small.clone(), e.mflat.clone(), e.vflat.clone(), e.loss_acc.clone(), *qs)


def _chk_phases(cfg, e_out, rows):
    """test_gpu_parity.test_step_against_oracle_random_shapes' bounds: the loss within 5e-6 of float64, Z within 1e-5, every gradient as
    close to float64 as max(2e-5, 8 x the fp32 oracle's own error)."""
    from neural_admixture_amd.layout import ModelLayout
    from test_gpu_parity import split_small
    c, p = CFG[cfg], _step_params(cfg)
    G = _step_G()[rows]
    b = len(rows)
    loss, grads, aux = O.step_grads(p, G)
    with O.precision64():
        p64 = O.Params(*[a.astype(np.float64) if isinstance(a, np.ndarray) else [v.astype(np.float64) for v in a]
                         for a in (p.V, p.g, p.W1, p.b1, p.Wk, p.bk, p.P)], ks=list(p.ks))
        loss64, grads64, aux64 = O.step_grads(p64, G)
    L = ModelLayout(M, c["C"], c["Hd"], c["ks"])
    zpart, Z, Q, dqpart, dZ, gflat, gflat2, loss_acc = (t.cpu().numpy() for t in e_out[:8])
    assert abs(loss_acc[1] - loss64) / abs(loss64) < 5e-6
    assert _mx(Z[: b * L.CP].reshape(b, L.CP)[:, :L.C], aux64["Z"]) < 1e-5
    g = split_small(L, gflat[: L.n_small])
    big = gflat[L.off_v:]
    g["V"] = big[: M * L.CP].reshape(M, L.CP)[:, :L.C]
    for h, k in enumerate(L.ks):
        g[f"P{h}"] = big[L.p_off[h]: L.p_off[h] + M * L.kp[h]].reshape(M, L.kp[h])[:, :k]
    g["dZ"] = dZ[: b * L.CP].reshape(b, L.CP)[:, :L.C]
    for name, want64 in dict(grads64, dZ=aux64["dZ"]).items():
        want32 = aux["dZ"] if name == "dZ" else grads[name]
        scale = float(np.abs(want64).max()) + 1e-30
        err_gpu, err_o32 = _mx(g[name], want64) / scale, _mx(want32, want64) / scale
        assert err_gpu < max(2e-5, 8 * err_o32), (name, err_gpu, err_o32)


def _chk_steps(cfg, e_out, rows):
    """__graft_entry__.smoke's bounds after two steps against the oracle's step_grads + Adam: the loss to 1e-5 relative, P and V to 1e-5."""
    from neural_admixture_amd.layout import ModelLayout
    c, p = CFG[cfg], _step_params(cfg)
    G = _step_G()[rows]
    opt = O.Adam(p, 2e-3)
    for _ in range(2):
        loss, grads, _ = O.step_grads(p, G)
        opt.step(p, grads)
    L = ModelLayout(M, c["C"], c["Hd"], c["ks"])
    pflat, loss_acc = e_out[0].cpu().numpy(), e_out[4].cpu().numpy()
    big = pflat[L.off_v:]
    assert abs(loss_acc[1] - loss) / loss < 1e-5
    assert np.abs(big[: M * L.CP].reshape(M, L.CP)[:, :L.C] - p.V).max() < 1e-5
    for h, k in enumerate(L.ks):
        assert np.abs(big[L.p_off[h]: L.p_off[h] + M * L.kp[h]].reshape(M, L.kp[h])[:, :k] - p.P[h]).max() < 1e-5
    for q in e_out[5:]:
        assert abs(float(q.sum()) - len(rows)) < 1e-3


ENGINE_RUNS = {"phases": (_phases, _chk_phases), "steps": (_steps, _chk_steps)}


@pytest.mark.parametrize("what", list(ENGINE_RUNS))
@pytest.mark.parametrize("cfg", list(CFG))
@pytest.mark.parametrize("placement", ["wide", "huge"])
def test_stride_of_the_step(cfg, what, placement):
    """Engine(ld=...) on the wide / huge matrix against an engine on the compact rows: the plain phases and two production steps +
    infer_q, bit for bit, with a gather list and with the list 0..n; the compact engine against the float64 oracle.  ks = [8], C = 8
    runs the matrix-pipe kernels; ks = [20], C = 12 encode_fwd_kernel<12>, decode_bce_kernel<24>, gather_rows_kernel and
    encode_bwd_kernel<12>."""
    run, chk = ENGINE_RUNS[what]
    full = _pack(_step_G())
    ch = _compact_of(placement, full)
    for mode in ("list", "none"):
        rows = _rows(placement, mode)
        idx = torch.from_numpy(rows).to(_dev())
        e = _engine(cfg, ch.to(_dev()))
        assert e.ld == RS
        want = run(e, idx, len(rows))
        torch.cuda.synchronize()
        chk(cfg, want, rows)
        e = _engine(cfg, _placed(placement, full))
        got = run(e, idx, len(rows))
        torch.cuda.synchronize()
        _assert_same_bits(got, want, f"{cfg} {what} {placement} rows={mode}")
        del e


def test_engine_with_a_stride_of_its_own_takes_set_packed_and_refuses_pack_from_host():
    import neural_admixture_amd as na
    dev = _dev()
    e = na.Engine(M, 8, 64, [3], dev, 8, ld=RS + 16)
    assert e.ld == RS + 16
    with pytest.raises(RuntimeError, match=f"uint8 \\[rows, {RS + 16}\\]"):
        e.set_packed(torch.zeros((8, RS), dtype=torch.uint8, device=dev))
    e.set_packed(torch.zeros((8, RS + 16), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="set_packed"):
        e.pack_from_host(torch.zeros((8, M), dtype=torch.uint8))
    for bad in (8, RS - 16, 2 ** 32):
        with pytest.raises(ValueError, match="ld must be"):
            na.Engine(M, 8, 64, [3], dev, 8, ld=bad)
    assert na.Engine(M, 8, 64, [3], dev, 8).ld == RS


# ================================================================================================ part B: stream
_DELAY = {}


def _delay_cycles():
    """torch.cuda._sleep cycles worth DELAY_MS, calibrated once with two events; prints what a delay then delivers."""
    if not _DELAY:
        def ms_of(cycles):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)
        ms_of(1_000_000)
        probe = 20_000_000
        cycles = int(probe * DELAY_MS / ms_of(probe))
        _DELAY.update(cycles=cycles, ms=ms_of(cycles))
        print(f"delay: torch.cuda._sleep({cycles}) delivers {_DELAY['ms']:.1f} ms between two events (target {DELAY_MS:.0f} ms)")
        assert _DELAY["ms"] > 0.5 * DELAY_MS
    return _DELAY["cycles"]


def _decoy(key, t):
    if key == "xp":
        return torch.full_like(t, 0xFF)
    if key == "Q" or key == "Qt":
        return torch.full_like(t, 1.0 / t.shape[1])
    if key in ("P", "Fq"):
        return torch.full_like(t, 0.5)
    if key in ("w", "B", "C"):
        return torch.ones_like(t)
    if key == "G":
        return torch.full_like(t, 3)
    if key == "bed":
        return torch.full_like(t, 0x55)                      # PLINK 01 four times: every call missing
    return torch.zeros_like(t)                               # idx, keep: row / SNP 0; V, Y: zeros


def _other(key, t):
    """Inputs of the warm-up call: valid, and neither the true ones nor the decoys."""
    if key in ("xp", "G", "bed"):
        return t.flip(0).contiguous()
    if key in ("idx", "keep"):
        return t.flip(0).contiguous()
    if t.dtype.is_floating_point:
        return t.roll(1, dims=-1).contiguous() if t.dim() > 1 else t.flip(0).contiguous()
    return t.flip(0).contiguous()


def _on_side_stream(call, true, what):
    """The protocol of part B for ``call(operands) -> outputs``; ``true``: dict of device operands.  Returns the outputs."""
    cycles = _delay_cycles()
    live = {k: _decoy(k, v) for k, v in true.items()}
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _taken(call({k: _other(k, v) for k, v in true.items()}))      # warm-up: scratch the allocator hands out again now holds another call's sums
    torch.cuda.synchronize()
    marker = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        marker.record(side)
        for k in true:
            live[k].copy_(true[k], non_blocking=True)
        out = call(live)
        premise = not marker.query()
        out = tuple(o.clone() for o in out)
    assert premise, f"{what}: the delay ended before the call returned on the host: nothing is shown"
    side.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(OPS))
def test_stream(name):
    data, fn, chk, _, _, _ = OPS[name]
    mode = _modes(name)[0]
    x, G = _host_operands(name, "wide", mode)
    true = dict(_to_dev(x), xp=_compact(data).to(_dev()))
    want = _taken(fn(true))
    torch.cuda.synchronize()
    got = _on_side_stream(fn, true, name)
    _assert_same_bits(got, want, f"{name} on a side stream")


@pytest.mark.parametrize("name", list(WRITERS))
def test_stream_of_a_writer(name):
    dev = _dev()
    true = _to_dev(_writer_operands(name))
    if name == "cv_mask":
        true["xp"] = _compact("edge").to(dev)

    def call(t):
        out = torch.full((ROWS, RS), 0xAA, dtype=torch.uint8, device=dev)
        return (out, *WRITERS[name](t, out))
    want = _taken(call(true))
    torch.cuda.synchronize()
    got = _on_side_stream(call, true, name)
    _assert_same_bits(got, want, f"{name} on a side stream")


@pytest.mark.parametrize("what", list(ENGINE_RUNS))
@pytest.mark.parametrize("cfg", list(CFG))
def test_stream_of_the_step(cfg, what):
    """The plain phases and nadm_step / nadm_plan_infer under torch.cuda.stream(side): the engine's matrix and the gather list are the
    live operands; the parameters are loaded before.  The warm-up call moves the engine's state, so the parameters are loaded again
    behind it (on both engines: the same history)."""
    run, _ = ENGINE_RUNS[what]
    dev = _dev()
    rows = _rows("wide", "list")
    b = len(rows)
    true = {"xp": _pack(_step_G()).to(dev), "idx": torch.from_numpy(rows).to(dev)}

    def fresh(xp):
        e = _engine(cfg, xp)
        run(e, torch.from_numpy(rows[::-1].copy()).to(dev), b)      # the warm-up's history, here on the default stream
        torch.cuda.synchronize()
        e._load()
        e.loss_acc.zero_()
        torch.cuda.synchronize()
        return e
    want = run(fresh(true["xp"]), true["idx"], b)
    torch.cuda.synchronize()

    cycles = _delay_cycles()
    live = {k: _decoy(k, v) for k, v in true.items()}
    e = _engine(cfg, live["xp"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        live["xp"].copy_(true["xp"])
        run(e, torch.from_numpy(rows[::-1].copy()).to(dev), b)
    torch.cuda.synchronize()
    live["xp"].fill_(0xFF)
    e._load()
    e.loss_acc.zero_()
    torch.cuda.synchronize()
    marker = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        marker.record(side)
        for k in true:
            live[k].copy_(true[k], non_blocking=True)
        got = run(e, live["idx"], b)
        premise = not marker.query()
    assert premise, f"{cfg} {what}: the delay ended before the calls returned on the host: nothing is shown"
    side.synchronize()
    torch.cuda.synchronize()
    _assert_same_bits(got, want, f"{cfg} {what} on a side stream")


def test_the_arena_is_released():
    """Last in the module: the 4.25 / 6 GiB buffer goes back to the device."""
    _ARENA.update(kind=None, buf=None)
    torch.cuda.empty_cache()
