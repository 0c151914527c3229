"""Precision "medium"  held to float64 at ragged and sliced shapes.

The medium step runs instantiations of its own of pass 1 (encode_fwd_mfma_kernel<CP, MED>) and pass 2 (decode_bce_bf16_kernel<KP, ..., MED>,
whole and in sample slices, KP 4 / 8 / 12 / 16) which the plain phases -- and with them tests/test_gpu_parity.py -- never launch.  Here one
``train_step`` of a medium engine is compared entry by entry with the float64 oracle, under the a-priori bound of tests/medium_bounds.py, at
shapes with several sample tiles, ragged last tiles, pad columns, sliced launches and more than four SNP chunks, in three engine forms:
"dp" without a communicator (gradients stored), the single-GPU engine and the SNP-sharded engine on a 1-rank RCCL communicator (Adam in
the epilogues of passes 2 and 3: the gradient is recovered from the first step's moment).

CPU tests (no GPU): the bound holds for the numpy restatement of the medium roundings at every shape, would not hold with dR's unit
halved, and rejects every planted defect.  GPU tests: the bound, per element, on the kernels; a shorter batch behind a longer one;
sliced against whole (test build); the two loss forms on planted P rows; infer_q over long and short batches."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import nadm_oracle as O      # noqa: E402
import medium_bounds as MB               # noqa: E402
import test_precision_medium as TM       # noqa: E402  (its engine helpers)

gpu = pytest.mark.gpu
HD, CW = 64, 8
SHAPE_IDS = [MB.shape_id(s) for s in MB.SHAPES]


def _to64(p):
    return O.Params(*[a.astype(np.float64) if isinstance(a, np.ndarray) else [x.astype(np.float64) for x in a]
                      for a in (p.V, p.g, p.W1, p.b1, p.Wk, p.bk, p.P)], ks=list(p.ks))


@functools.lru_cache(maxsize=None)
def _case(b, M, ks):
    """One shape's inputs and its float64 step, computed once and shared (read-only) by every test of the shape."""
    Gm, perm, p = MB.make_case(O, b, M, list(ks), HD, CW)
    Gb = Gm[perm[:b]]
    with O.precision64():
        loss64, grads64, aux64 = O.step_grads(_to64(p), Gb)
    for a in list(grads64.values()) + [aux64["Z"]] + aux64["Qs"]:
        a.setflags(write=False)
    return {"G": Gm, "perm": perm, "p": p, "X": MB.decode_x64(Gb), "loss": loss64, "grads": grads64, "Z": aux64["Z"], "Qs": aux64["Qs"]}


# ------------------------------------------------------------------------------------------------ the bound itself (no GPU)
def test_hi_plus_mid_leaves_two_to_the_minus_16():
    """The split the bound's u16 is about (csrc/nadm_common.h, split3: every piece a round-to-nearest-even conversion): hi + mid is off
    by at most 2^-16 |v|, half of u16, and is exact in fp32."""
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.uniform(0.0, 1.0, 200_000), rng.standard_normal(200_000) * 1e-3, [0.0, 1.0, 0.02, 0.98, 1e-12]]).astype(np.float32)
    t = MB.hi_mid(v)
    err = np.abs(t.astype(np.float64) - v.astype(np.float64))
    assert (err <= 2.0 ** -16 * np.abs(v.astype(np.float64))).all() and 2.0 ** -16 < MB.U16
    tt = MB.hi_mid(v, MB.bf16_trunc)                         # pass 1's truncating split of V: just inside u16, and never above |v|
    assert (np.abs(tt.astype(np.float64) - v.astype(np.float64)) < MB.U16 * np.abs(v.astype(np.float64)) + (v == 0)).all() and (np.abs(tt) <= np.abs(v)).all()
    assert np.array_equal(MB.bf16_rne(t) + MB.bf16_rne(t - MB.bf16_rne(t)), t)          # two pieces hold it exactly
    # ties go to even: 1 + 2^-8 lies half-way between the bf16 neighbours 1 and 1 + 2^-7
    assert MB.bf16_rne(np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]))[0] == 1.0
    assert MB.bf16_rne(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == np.float32(1.0 + 2.0 ** -6)


@pytest.mark.parametrize("shape", MB.SHAPES, ids=SHAPE_IDS)
def test_bound_holds_for_the_restated_roundings(shape):
    """The reference alone stays inside the bound: hi + mid operands, fp32 products, dR as one bf16 piece, fp32 accumulation."""
    b, M, ks = shape
    c = _case(b, M, tuple(ks))
    for h, k in enumerate(ks):
        P, Q = c["p"].P[h], c["Qs"][h].astype(np.float32)
        B, dP64 = MB.dp_bound(c["X"], P, Q)
        for cut in (MB.bf16_rne, MB.bf16_trunc):            # the operands as split3 leaves them, and at the whole u16 (truncated pieces)
            ok, ratio, at, _ = MB.check_dp(MB.restate_dp(c["X"], P, Q, cut), k, dP64, B)
            print(f"{MB.shape_id(shape)} K={k}: restated dP ({cut.__name__}) err / B_dP {ratio:.3f} at SNP {at[0]} k {at[1]}")
            assert ok and ratio <= 1.0
    Bz, Z64 = MB.z_bound(c["X"], c["p"].V)
    rz, _ = MB.worst(MB.restate_z(c["X"], c["p"].V) - Z64, Bz)
    print(f"{MB.shape_id(shape)}: restated Z err / B_Z {rz:.3f}")
    assert rz <= 1.0


def test_bound_is_not_slack_in_drs_unit():
    """u8 = 2^-8 is dR's one bf16 piece and nothing smaller will do: with 2^-9 the restated roundings break the bound where no second
    sample averages the rounding out (b = 1: 1.28 of the halved bound; at b = 23 the sum is already at 0.73 of it)."""
    shape = MB.SHAPES[0]
    b, M, ks = shape
    assert b == 1
    c = _case(b, M, tuple(ks))
    P, Q = c["p"].P[0], c["Qs"][0].astype(np.float32)
    B, dP64 = MB.dp_bound(c["X"], P, Q, u8=2.0 ** -9)
    ratio, _ = MB.worst(MB.restate_dp(c["X"], P, Q) - dP64, B)
    print(f"{MB.shape_id(shape)}: err / B_dP(u8 = 2^-9) {ratio:.3f}")
    assert ratio > 1.0


@pytest.mark.parametrize("shape", MB.SHAPES, ids=SHAPE_IDS)
def test_bound_rejects_every_planted_defect(shape):
    """It is sharp: a dropped last sample of a ragged tile, a dropped last SNP, a tile counted twice, two k columns swapped across the
    k slots and a non-zero pad column, planted in the float64 dP, are each rejected (medium_bounds.required_defects says which ones a
    shape must catch); the unspoilt dP passes."""
    b, M, ks = shape
    c = _case(b, M, tuple(ks))
    for h, k in enumerate(ks):
        kp = (k + 3) // 4 * 4
        P, Q = c["p"].P[h], c["Qs"][h].astype(np.float32)
        B, dP64 = MB.dp_bound(c["X"], P, Q)
        clean = np.zeros((M, kp))
        clean[:, :k] = dP64
        assert MB.check_dp(clean, k, dP64, B)[0]
        planted = MB.planted_defects(c["X"], P, Q, kp)
        assert {"last_snp_dropped", "first_tile_twice"} <= set(planted)
        assert ("last_sample_of_ragged_tile_dropped" in planted) == (b % 64 != 0)
        assert ("columns_8_and_last_swapped" in planted) == (k > 9) and ("pad_column_nonzero" in planted) == (kp > k)
        for name, bad in planted.items():
            ok, ratio, at, share = MB.check_dp(bad, k, dP64, B)
            print(f"{MB.shape_id(shape)} K={k} {name}: err / B_dP {ratio:.3g}, {100 * share:.1f} % of the entries flagged")
            if name in MB.required_defects(b):
                assert not ok, (name, ratio)
            if name == "last_snp_dropped" and name in MB.required_defects(b):
                assert (np.abs(bad[M - 1, :k] - dP64[M - 1]) > B[M - 1]).all()           # its whole row


# ------------------------------------------------------------------------------------------------ GPU
def _p_sm(p):
    return np.concatenate([P.T for P in p.P], axis=0)


def _engine(Gm, p, bmax, **kw):
    return TM._engine(Gm, p, bmax, precision="medium", **kw)


# adam_element (csrc/nadm_common.h): m1 = m0 + (g - m0) * omb1 with omb1 = (float)(1.0 - 0.9) and m0 = 0, i.e. ONE fp32 multiplication:
# g = m1 / omb1 (in float64, with the fp32 constant) recovers the gradient to 2^-24 relative, 2^-16 of dR's own unit
OMB1 = float(np.float32(1.0 - 0.9))


def _split(L, flat):
    """A flat parameter-shaped buffer (gradients, a moment) -> {name: array}, P and V with their pad columns."""
    h = L.heads
    out = {"g": flat[h.g_off:h.g_off + L.C], "W1": flat[h.w1_off:h.w1_off + L.Hd * L.C], "b1": flat[h.b1_off:h.b1_off + L.Hd]}
    big = flat[L.off_v:]
    out["Vp"] = big[: L.M * L.CP].reshape(L.M, L.CP)
    out["V"] = out["Vp"][:, : L.C]
    for i, k in enumerate(L.ks):
        out[f"Wk{i}"] = flat[h.wk_off[i]:h.wk_off[i] + k * L.Hd]
        out[f"bk{i}"] = flat[h.bk_off[i]:h.bk_off[i] + k]
        out[f"Pp{i}"] = big[L.p_off[i]: L.p_off[i] + L.M * L.kp[i]].reshape(L.M, L.kp[i])
    return out


def _make(form, c, b, M, ks):
    """(engine, communicator or None) of one of the three engine forms, loaded with the case's parameters and genotypes."""
    p = c["p"]
    if form == "dp":
        return _engine(c["G"], p, b, mode="dp"), None
    if form == "single":
        return _engine(c["G"], p, b), None
    from neural_admixture_amd.comm import rccl_comm
    from neural_admixture_amd.snp_parallel import SnpShardedEngine
    comm = rccl_comm(0, 1)
    e = SnpShardedEngine(M, CW, HD, ks, TM._dev(), b, comm=comm, precision="medium")
    e.load_params(p.V, _p_sm(p), TM._small_vec(p))
    e.pack_from_host(torch.from_numpy(np.ascontiguousarray(c["G"])))
    return e, comm


SNP_SHAPES = [(150, 2301, [8]), (520, 2301, [4, 8, 12]), (65, 2049, [5])]
STEP_CASES = [(s, f) for s in MB.SHAPES for f in ("dp", "single")] + [(s, "snp") for s in SNP_SHAPES]


@gpu
@pytest.mark.parametrize("shape,form", STEP_CASES, ids=[f"{MB.shape_id(s)}-{f}" for s, f in STEP_CASES])
def test_medium_step_within_the_bound_of_float64(shape, form):
    """One medium train_step against the float64 oracle: every entry of every head's dP within B_dP (from the engine's own Q and the
    host's P0), Z within B_Z, Q 1e-4, loss 1e-4, the other gradients within 2^-8 of their maximum; pad columns exactly zero, everything
    finite, an all-missing sample's Z row exactly 0."""
    b, M, ks = shape
    c = _case(b, M, tuple(ks))
    p = c["p"]
    from neural_admixture_amd._lib import lib
    e, comm = _make(form, c, b, M, ks)
    try:
        L = e.lay
        slices = [int(lib.nadm_decode_slices(b, M, kp)) for kp in L.kp]
        if b in (520, 900):
            assert min(slices) > 1                           # pass 2 in sample slices by the library's own rule
        idx = torch.from_numpy(c["perm"][:b].copy()).to(e.device)
        e.train_step(idx, b, 2e-3, with_loss=True)
        e.sync()
        torch.cuda.synchronize()
        _, loss = e.read_loss()
        Q = e.Q.cpu().numpy()[: b * L.SP].reshape(b, L.SP)
        Z = e.Z.cpu().numpy()[: b * L.CP].reshape(b, L.CP)
        mom, vel = e.mflat.cpu().numpy(), e.vflat.cpu().numpy()
        if form == "dp":                                     # the gradients as stored
            flat = e.gflat.cpu().numpy().astype(np.float64)
        else:                                                # Adam ran in the epilogues: the first step's moment is the gradient times omb1
            flat = mom.astype(np.float64) / OMB1
    finally:
        del e
        if comm is not None:
            comm.close()
    g = _split(L, flat)
    assert all(np.isfinite(a).all() for a in (flat, mom, vel, Q, Z)) and np.isfinite(loss)
    # pad columns: gradients (or what stands for them) and both moments
    for buf in (g, _split(L, mom), _split(L, vel)):
        assert not buf["Vp"][:, L.C:].any()
        for h, k in enumerate(ks):
            assert not buf[f"Pp{h}"][:, k:].any()
    assert not Z[:, L.C:].any()
    report, fails = [], []
    # pass 1
    Bz, Z64 = MB.z_bound(c["X"], p.V)
    rz, at = MB.worst(Z[:, : L.C] - Z64, Bz)
    report.append(f"Z {rz:.3f}")
    if rz > 1.0:
        fails.append(f"Z: err / B_Z {rz:.3f} at sample {at[0]} column {at[1]}")
    if shape == MB.MISSING_HEAVY:
        assert not Z[5].any()                                # the sample without a single call projects to exactly 0
    # pass 2, head by head, judged on the Q it was given
    for h, k in enumerate(ks):
        Qh = Q[:, L.qoff[h]: L.qoff[h] + k]
        qe = float(np.abs(Qh - c["Qs"][h]).max())
        report.append(f"Q{h} {qe:.1e}")
        if qe >= 1e-4:
            fails.append(f"Q{h}: {qe:.2e}")
        B, dP64 = MB.dp_bound(c["X"], p.P[h], Qh)
        ok, ratio, (snp, kk), share = MB.check_dp(g[f"Pp{h}"], k, dP64, B)
        report.append(f"dP{h}[K={k} KP={L.kp[h]} S={slices[h]}] {ratio:.3f}")
        if not ok:
            fails.append(f"dP{h}: err / B_dP {ratio:.3f} at SNP {snp} k {kk} (SNP chunk {snp // 512}; {slices[h]} slices over "
                         f"{(b + 63) // 64} tiles), {100 * share:.2f} % of the entries over")
    le = abs(loss - c["loss"]) / abs(c["loss"])
    report.append(f"loss {le:.1e}")
    if le >= 1e-4:
        fails.append(f"loss: {le:.2e}")
    # the project's own medium bound on every other gradient
    names = ["V", "g", "W1", "b1"] + [f"{w}{h}" for h in range(len(ks)) for w in ("Wk", "bk")]
    for n_ in names:
        want = np.asarray(c["grads"][n_], dtype=np.float64)
        r = float(np.abs(g[n_].reshape(want.shape) - want).max() / (np.abs(want).max() + 1e-30))
        report.append(f"{n_} {r:.1e}")
        if r >= 2.0 ** -8:
            fails.append(f"{n_}: {r:.2e} of its maximum")
    print(f"medium {MB.shape_id(shape)} {form}: worst err / B and errors: " + " ".join(report))
    assert not fails, fails


@gpu
@pytest.mark.parametrize("b,M,ks,b2", [(150, 2301, [3, 8, 13], 87), (520, 2301, [4, 8, 12], 470)], ids=["150_then_87", "520_then_470"])
def test_medium_shorter_batch_after_a_longer_one_leaves_no_stale_rows(b, M, ks, b2):
    """Pass 2 reads Q from tile images that outlive the step: after a batch of b rows, a step on b2 < b rows (a ragged tile whose
    remaining rows held the longer batch's Q, and whole tiles behind it that did) must give the dP of the b2 rows alone, within B_dP --
    the three k forms at once, whole (150 -> 87) and in slices (520 -> 470)."""
    c = _case(b, M, tuple(ks))
    p = c["p"]
    from neural_admixture_amd._lib import lib
    e = _engine(c["G"], p, b, mode="dp")
    L = e.lay
    idx = torch.from_numpy(c["perm"][:b].copy()).to(e.device)
    e.train_step(idx, b, 2e-3, with_loss=True)
    e.load_params(p.V, _p_sm(p), TM._small_vec(p))          # the parameters of the first step again, moments and step count zeroed
    e.train_step(idx[:b2], b2, 2e-3, with_loss=True)
    e.sync()
    torch.cuda.synchronize()
    Q = e.Q.cpu().numpy()[: b2 * L.SP].reshape(b2, L.SP)
    g = _split(L, e.gflat.cpu().numpy().astype(np.float64))
    X = c["X"][:b2]
    with O.precision64():
        Q64 = O.encoder_forward(_to64(p), X)[4]
    for h, k in enumerate(ks):
        Qh = Q[:, L.qoff[h]: L.qoff[h] + k]
        assert np.abs(Qh - Q64[h]).max() < 1e-4
        B, dP64 = MB.dp_bound(X, p.P[h], Qh)
        ok, ratio, (snp, kk), share = MB.check_dp(g[f"Pp{h}"], k, dP64, B)
        print(f"medium {b} -> {b2} rows x {M} K={k} S={int(lib.nadm_decode_slices(b2, M, L.kp[h]))}: dP err / B_dP {ratio:.3f}")
        assert ok, f"dP{h}: err / B_dP {ratio:.3f} at SNP {snp} k {kk}, {100 * share:.2f} % of the entries over"


@gpu
@pytest.mark.parametrize("b,M,ks", [(520, 2301, [8]), (400, 2301, [3, 12])], ids=["520x2301-k8", "400x2301-k3_12"])
def test_medium_pass2_in_sample_slices_gives_the_unsliced_gradients(request, b, M, ks):
    """The sliced medium pass 2 against the S = 1 medium kernel on the same inputs, S = 2, 3, 4 and the library's own choice: gradients
    within 2e-6 of their scale, the loss within 1e-6 (the bounds of the "highest" test: here too only the order of the fp32 dP sum
    differs), the same bits on a second call, counters back at zero.  (Forcing S needs the test build: conftest.in_hook_build.)"""
    from conftest import in_hook_build
    if not in_hook_build(request):
        return
    from neural_admixture_amd._lib import lib
    c = _case(b, M, tuple(ks))
    p = c["p"]
    idx = torch.from_numpy(c["perm"][:b].copy()).to(TM._dev())

    def run(force):
        lib.nadm_test_force_slices(force)
        try:
            e = _engine(c["G"], p, b, mode="dp")
            want = [int(lib.nadm_decode_slices(b, M, kp)) for kp in e.lay.kp]
            outs = []
            for _ in range(2):
                e.load_params(p.V, _p_sm(p), TM._small_vec(p))              # (zeroes the moments and the step count as well)
                e.train_step(idx, b, 2e-3, with_loss=True)
                e.sync()
                torch.cuda.synchronize()
                outs.append((e.gflat.clone(), e.read_loss()[1]))
                assert e._p2_cnt is None or int(e._p2_cnt.abs().sum().item()) == 0
            assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], "not reproducible"
            return _split(e.lay, outs[0][0].cpu().numpy()), outs[0][1], want
        finally:
            lib.nadm_test_force_slices(0)

    g1, loss1, want1 = run(1)
    assert want1 == [1] * len(ks)
    for force in (2, 3, 4, 0):
        g, loss, want = run(force)
        if force:
            assert all(w == min(force, (b + 63) // 64) or w <= force for w in want) and max(want) > 1
        for k_ in g1:
            scale = np.abs(g1[k_]).max() + 1e-30
            d = float(np.abs(g[k_] - g1[k_]).max() / scale)
            assert d <= 2e-6, (force, k_, d)
        assert abs(loss - loss1) <= 1e-6 * abs(loss1)
        print(f"medium sliced {b}x{M} {ks}: forced {force} -> {want} slices, loss {abs(loss - loss1) / abs(loss1):.1e}")


@gpu
@pytest.mark.parametrize("ks", [[5], [13]])
def test_medium_pair_product_loss_and_its_exact_fallback(ks):
    """The planted P rows of test_gpu_parity.test_pair_product_loss_and_its_exact_fallback (0 under non-zero genotypes, 1e-12, 1) over two
    sample tiles under "medium": the one-logarithm-per-pair loss and the exact form (p_unit False) agree within 2e-6, the gradients do not
    depend on the loss form at all, and with the rows of 0 and 1e-12 the loss is within 1e-4 of the oracle's."""
    rng = np.random.default_rng(21)
    N, M = 70, 3000
    Gm = O.synth_genotypes(N, M, 4, seed=9, missing=0.03)
    Gm[:, 100:140] = rng.integers(0, 3, size=(N, 40))
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.02, 0.98, size=(sum(ks), M)).astype(np.float32)
    P0[:, 100:140] = 0.0
    P0[:, 300:320] = 1e-12
    P1 = P0.copy()
    P1[:, 200:230] = 1.0
    G2 = Gm.copy()
    G2[:, 200:230] = 1                                       # ... and called heterozygous in every sample
    loss_o = O.step_grads(O.make_params(3, V0, P0, HD, ks), Gm)[0]
    for what, Pm, Gx, ref in (("rows of 0 and 1e-12", P0, Gm, loss_o), ("and rows of 1", P1, Gm, None), ("rows of 1 under heterozygotes", P1, G2, None)):
        p = O.make_params(3, V0, Pm, HD, ks)
        res = {}
        for form in ("fast", "exact"):
            e = _engine(Gx, p, N, mode="dp")
            idx = torch.arange(N, dtype=torch.int32, device=e.device)
            assert e.p_unit
            e.p_unit = form == "fast"
            e.train_step(idx, N, 2e-3, with_loss=True)
            e.sync()
            torch.cuda.synchronize()
            res[form] = (e.read_loss()[1], e.gflat.clone())
            del e
        lf, le = res["fast"][0], res["exact"][0]
        print(f"medium loss forms K={ks[0]} {what}: fast / exact {abs(lf - le) / abs(le):.1e}" + ("" if ref is None else f", oracle {abs(lf - ref) / abs(ref):.1e}"))
        assert np.isfinite(lf) and abs(lf - le) <= 2e-6 * abs(le)
        assert torch.equal(res["fast"][1], res["exact"][1]) and bool(torch.isfinite(res["fast"][1]).all())
        if ref is not None:
            assert abs(lf - ref) <= 1e-4 * abs(ref)


@gpu
def test_medium_infer_q_against_float64_over_long_and_short_batches():
    """infer_q under "medium" in batches of 1024 / 1024 / 52 (the first two beyond pass 1's 832-row block, the last one short) against
    the float64 oracle, in row order."""
    from neural_admixture_amd.engine import final_q, row_ranges
    N, M, ks = 2100, 1531, [3, 9]
    assert [bb for _, bb in row_ranges(N, 1024)] == [1024, 1024, 52]
    Gm = O.synth_genotypes(N, M, 5, seed=77, missing=0.05)
    rng = np.random.default_rng(12)
    p = O.make_params(7, (rng.standard_normal((M, CW)) / np.sqrt(M)).astype(np.float32), rng.uniform(0.02, 0.98, (sum(ks), M)).astype(np.float32), HD, ks)
    with O.precision64():
        want = O.infer_q(Gm, _to64(p), 1024)
    e = _engine(Gm, p, 1024)
    got = [q.cpu().numpy() for q in final_q(e, N, 1024)]
    for h, k in enumerate(ks):
        assert got[h].shape == (N, k) and np.isfinite(got[h]).all()
        d = np.abs(got[h] - want[h]).max(axis=1)
        print(f"medium infer_q K={k}: max |dQ| {d.max():.2e} (row {int(d.argmax())})")
        assert d.max() < 1e-4
