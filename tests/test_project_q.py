"""Projection (nadm_project_q, project.project_q, Engine.project_q, `infer --refine`): Q refined against a fixed P with masked EM
steps.  The float64 / float32 numpy restatement lives in tests/project_oracle.py."""
import ctypes as C
import functools
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_oracle as R  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
PROJ_CHUNK = 256             # SNPs per chunk of the accumulate kernel (csrc/nadm_project.hip: PROJ_CHUNK); 64-sample tiles
SHAPES = [(70, 3001, 3), (130, 2050, 8), (70, 1027, 16)]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_raises_the_likelihood_keeps_row_sums_and_leaves_an_empty_row(shape):
    N, M, K = shape
    Gm, P, Q = R.make_case(N, M, K)
    assert (Gm[4] == 3).all() and (Gm[5] != 3).sum() == 7 and (P == 0).all(axis=1).any() and (P == 1).all(axis=1).any()
    assert abs(float((Gm == 3).mean()) - 0.05) < 0.03 and Q[2].max() == 1.0
    Qn, lls = R.iterate(Gm, P, Q, 13)                       # lls[t] = ll at the input of step t: 12 steps apart
    assert (np.diff(lls, axis=0) >= 0.0).all()
    assert np.abs(Qn.sum(axis=1) - 1.0).max() <= 1.5e-8
    assert np.array_equal(Qn[4], Q[4].astype(np.float64)) and (lls[:, 4] == 0.0).all()
    q32, _, n32 = R.em_step(Gm, P, Q, dtype=np.float32)
    q64, _, n64 = R.em_step(Gm, P, Q)
    assert np.array_equal(n32, n64) and np.abs(q32 - q64).max() < 2.5e-7


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    P = torch.full((50, 4), 0.25)
    Q = torch.full((4, 4), 0.25)
    out = torch.empty((4, 4))
    scratch = torch.empty(64)
    keep = (xp, P, Q, out, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, P=P.data_ptr(), k=3, kp=4, Qin=Q.data_ptr(), Qout=out.data_ptr(), q_stride=4,
             eps=1e-6, qmin=1e-6, loglik=None, nobs=None, scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(P=None), "null pointer"), (dict(Qin=None), "null pointer"), (dict(Qout=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(ld=12), "ld < ceil(M/4)"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(b=0), "empty batch"), (dict(b=-3), "empty batch"),
])
def test_project_q_refuses_before_any_launch(change, message):
    """Every refusal of nadm_project_q is decided on the host: it is reported with its message on a machine without a GPU."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    a.update(change)
    status = lib.nadm_project_q(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_project_q"):
        check(status, "project_q")
    del keep


def test_project_scratch_floats_grows_with_the_batch_and_the_snps():
    from neural_admixture_amd._lib import lib
    f = lib.nadm_project_scratch_floats
    for kp in (4, 8, 12, 16, 24, 64):
        last = 0
        for b in (1, 2, 64, 65, 800):
            v = [int(f(b, M, kp)) for M in (1, 255, 256, 257, 3001, 500000)]
            assert v[0] > 0 and all(y >= x for x, y in zip(v, v[1:])) and v[0] >= last
            assert int(f(b, 500000, kp)) >= int(f(max(1, b - 1), 500000, kp))
            last = v[0]
    assert int(f(800, 500000, 8)) >= (500000 // PROJ_CHUNK) * 800 * 8


def test_header_declares_both_symbols_and_the_binding_has_them():
    from neural_admixture_amd._lib import EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_project_q", "nadm_project_scratch_floats"):
        assert name + "(" in header and name in EXPORTS
    assert "#define NADM_ABI_VERSION 14" in header


def test_cli_refine_flags_and_a_missing_P_file(tmp_path, monkeypatch):
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    base = ["--out_name", "o", "--save_dir", str(tmp_path), "--data_path", "x.bed", "--name", "run"]
    a = cli.parse_infer_args(base)
    assert a.refine == 0 and a.refine_tol == 1e-4
    a = cli.parse_infer_args(base + ["--refine", "5", "--refine_tol", "1e-3"])
    assert a.refine == 5 and a.refine_tol == 1e-3
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    # the config's num_features is the width of the encoder's input (2 here); the model's number of SNPs is the rows of V (10)
    (tmp_path / "run_config.json").write_text(json.dumps({"ks": [3, 4], "num_features": 2, "hidden_size": 16, "activation": "relu"}))
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.25, dtype=np.float32))
    with pytest.raises(SystemExit, match=r"run\.4\.P not found"):                  # before the checkpoint is even looked for
        cli.main(["infer"] + base + ["--refine", "5"])
    torch.save({"V": torch.zeros(10, 2)}, tmp_path / "run.pt")
    np.savetxt(tmp_path / "run.4.P", np.full((9, 4), 0.25, dtype=np.float32))
    with pytest.raises(SystemExit, match=r"run\.4\.P holds a 9 x 4 matrix, the model needs 10 x 4"):
        cli.main(["infer"] + base + ["--refine", "5"])
    np.savetxt(tmp_path / "run.3.P", np.full((2, 3), 0.25, dtype=np.float32))     # num_features rows is NOT what is asked for
    np.savetxt(tmp_path / "run.4.P", np.full((10, 4), 0.25, dtype=np.float32))
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 2 x 3 matrix, the model needs 10 x 3"):
        cli.main(["infer"] + base + ["--refine", "5"])


def test_sharded_engines_refuse_projection():
    """Engine.project_q is single-GPU; the check comes first, so a stand-in without any device state shows it."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan = "dp", 2, None
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.project_q(None, 1)
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.project_q(None, 1)


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(M, K, edge=True):
    Gm, P, Q = R.make_case(130, M, K, edge=edge)
    return Gm, P, Q, _packed(Gm)


def _batch(b):
    """Rows of the batch: a permutation of the 130 resident rows with the all-missing row 4 and the 7-call row 5 in it, cut to b, the
    last entry a duplicate of the first; b = 1 is the 7-call row."""
    if b == 1:
        return np.asarray([5], dtype=np.int32)
    perm = np.random.default_rng(b).permutation(130)
    perm = np.concatenate([[4, 5], perm[(perm != 4) & (perm != 5)]])[:b]
    perm = perm[np.random.default_rng(b + 1).permutation(b)]
    perm[-1] = perm[0]
    return perm.astype(np.int32)


def _gpu_step(xp, M, idx, P, Q, loglik=True, inplace=False, eps=R.EPS, qmin=R.QMIN):
    """One nadm_project_q call -> (Q_out [b, K] numpy, ll [b] or None, nobs [b])."""
    from neural_admixture_amd import project
    from neural_admixture_amd._lib import lib
    dev = xp.device
    b, K = Q.shape
    Pp = project.pad_P(P, dev)
    qin = project.pad_Q(Q, b, K, Pp.shape[1], dev)
    qout = qin if inplace else torch.full_like(qin, 7.0)
    ll = torch.full((b,), 7.0, dtype=torch.float64, device=dev) if loglik else None
    no = torch.full((b,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.nadm_project_scratch_floats(b, M, Pp.shape[1])), dtype=torch.float32, device=dev)
    project.em_step(xp, M, None if idx is None else torch.from_numpy(idx).to(dev), b, Pp, K, qin, qout, scratch, eps, qmin, ll, no)
    torch.cuda.synchronize()
    assert not qout[:, K:].any()                             # padded columns stay 0
    return qout[:, :K].cpu().numpy(), None if ll is None else ll.cpu().numpy(), no.cpu().numpy()


def _ll_tol(Gb, P, Q, ll64):
    """Relative tolerance of the kernel's ll: 8 x the float32 restatement's own relative error to float64, at least 1e-6."""
    _, ll32, _ = R.em_step(Gb, P, Q, dtype=np.float32)
    nz = ll64 != 0.0
    e32 = float((np.abs(ll32 - ll64)[nz] / np.abs(ll64[nz])).max()) if nz.any() else 0.0
    return max(8.0 * e32, 1e-6), e32


ONE_STEP = [(b, M, K) for b in (1, 70, 130) for M in (1027, 3001, PROJ_CHUNK + 1, 2 * PROJ_CHUNK + 1) for K in (2, 3, 8, 9, 16)] + [(70, 1027, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K", ONE_STEP)
def test_one_step_against_float64(b, M, K):
    """max |Q_gpu - Q_f64| <= 1e-6 (the float32 restatement lands 5e-8 .. 1.2e-7 from float64; the bound leaves ~8x for another summation
    order and hardware reciprocals), nobs exact, ll within max(8 e32, 1e-6) relative, e32 = the float32 restatement's own relative
    error.  Every case prints its figures before it asserts.  OBSERVED on an MI355X over the whole ONE_STEP grid (61 cases):
    max |Q_gpu - Q_f64| 3.4e-9 .. 2.5e-7 (b = 1: <= 2.4e-8; the largest at b = 70, M = 257, K = 3); ll relative error 5.4e-9 .. 2.7e-7
    (b = 1: <= 8.1e-8; the largest at b = 70, M = 257, K = 8).  e32 is 3.3e-10 .. 5.5e-8 for the single 7-call row of b = 1 (tol = the
    1e-6 floor; M = 513, K = 3: 8.1e-4) and 1.8e-4 .. 8.1e-4 for b = 70 and 130 (tol 1.5e-3 .. 6.5e-3): there the worst row meets rows of
    P that are exactly 0 or 1, r sits at the clip, and the float32 restatement's fl(1 - eps) is 1.3 % off in 1 - r."""
    dev = _dev()
    Gm, P, Q, xph = _case(M, K)
    idx = _batch(b)
    Gb, Qb = Gm[idx], Q[:b].copy()
    if b > 2:
        assert Qb[2].max() == 1.0 and (Gb == 3).all(axis=1).sum() >= 1 and ((Gb != 3).sum(axis=1) == 7).sum() >= 1
    q64, ll64, n64 = R.em_step(Gb, P, Qb)
    tol, e32 = _ll_tol(Gb, P, Qb, ll64)
    q, ll, n = _gpu_step(xph.to(dev), M, idx, P, Qb)
    dq = float(np.abs(q - q64).max())
    rel = np.abs(ll - ll64) / np.maximum(np.abs(ll64), 1e-300)
    print(f"b={b} M={M} K={K}: max|Q_gpu - Q_f64| = {dq:.3e}, ll rel err = {float(rel[ll64 != 0].max()) if (ll64 != 0).any() else 0.0:.3e}, "
          f"e32 = {e32:.3e}, tol = {tol:.3e}")
    assert np.array_equal(n, n64)
    assert dq <= 1e-6
    assert np.abs(q.sum(axis=1) - 1.0).max() < 1e-6
    assert (np.abs(ll - ll64) <= tol * np.abs(ll64)).all()
    assert (ll[n64 == 0] == 0.0).all() and np.array_equal(q[n64 == 0], Qb[n64 == 0])
    if b == 70 and M == 1027:                                # rows 0..b without a gather list
        q0, _, n0 = _gpu_step(xph.to(dev), M, None, P, Qb, loglik=False)
        assert np.abs(q0 - R.em_step(Gm[:b], P, Qb)[0]).max() <= 1e-6 and np.array_equal(n0, (Gm[:b] != 3).sum(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 16, 20])
def test_a_missing_call_and_the_pad_bits_contribute_exactly_nothing(K):
    """P changed at the SNPs where a sample's call is missing, every bit of the packed row that holds no SNP set: that sample's row
    of Q, its ll and its count come out bit-identical."""
    dev = _dev()
    M, b = 1027, 70
    Gm, P, Q, xph = _case(M, K)
    want = _gpu_step(xph.to(dev), M, None, P, Q[:b])
    dirty = _packed(Gm, dirty=True).to(dev)
    for i in (0, 5, 69):
        miss = Gm[i] == 3
        assert miss.any()
        P2 = P.copy()
        P2[miss] = 1.0 - 0.5 * P[miss][:, ::-1]
        got = _gpu_step(dirty, M, None, P2, Q[:b])
        for w, g in zip(want, got):
            assert w[i].tobytes() == g[i].tobytes()
        assert not np.array_equal(want[0][1], got[0][1])     # (a row that observes those SNPs does move)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 20])
def test_two_launches_agree_bit_for_bit_and_in_place_equals_out_of_place(K):
    dev = _dev()
    M, b = 3001, 130
    Gm, P, Q, xph = _case(M, K)
    xp, idx = xph.to(dev), _batch(b)
    one = _gpu_step(xp, M, idx, P, Q)
    two = _gpu_step(xp, M, idx, P, Q)
    inp = _gpu_step(xp, M, idx, P, Q, inplace=True)
    nol = _gpu_step(xp, M, idx, P, Q, loglik=False)
    for x, y, z in zip(one, two, inp):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert nol[0].tobytes() == one[0].tobytes() and nol[1] is None and np.array_equal(nol[2], one[2])   # the loglik-free variant: the same Q


@pytest.mark.gpu
def test_twelve_steps_raise_the_likelihood_and_follow_the_float64_trajectory():
    """(130, 2050, 8), P in [0.02, 0.98]: the kernel's per-sample ll never drops by more than its tolerance of the one-step test, the
    summed ll rises, the final Q stays within 1e-6 of the float64 trajectory (the float32 restatement: 1.2e-7).  OBSERVED on an MI355X:
    the largest relative "drop" of a sample's ll over the 12 steps is -1.6e-4 (every sample's ll rose at every step; tol = the 1e-6
    floor, e32 = 4.8e-8), the summed ll goes -285330.655 -> -276922.696, max |Q_gpu - Q_f64| after 12 steps 1.6e-7."""
    from neural_admixture_amd import project
    dev = _dev()
    b, M, K = 130, 2050, 8
    Gm, P, Q, xph = _case(M, K, edge=False)
    assert P.min() >= 0.02 and P.max() <= 0.98
    xp = xph.to(dev)
    q64, lls64 = R.iterate(Gm, P, Q, 13)
    tol, e32 = _ll_tol(Gm, P, Q, lls64[0])
    q, lls = Q, []
    for _ in range(12):
        q, ll, _ = _gpu_step(xp, M, None, P, q)
        lls.append(ll)
    _, ll, _ = _gpu_step(xp, M, None, P, q)
    lls = np.asarray(lls + [ll])
    drop = (lls[:-1] - lls[1:]) / np.abs(lls[:-1])
    q12 = R.iterate(Gm, P, Q, 12)[0]
    print(f"largest relative drop of a sample's ll {float(drop.max()):.3e} (tol {tol:.3e}, e32 {e32:.3e}); summed ll {lls.sum(axis=1)[0]:.3f} -> "
          f"{lls.sum(axis=1)[-1]:.3f}; max|Q_gpu - Q_f64| after 12 steps {float(np.abs(q - q12).max()):.3e}")
    assert (drop <= tol).all()
    assert (np.diff(lls.sum(axis=1)) > 0).all()
    assert np.abs(q - q12).max() <= 1e-6
    assert (np.abs(lls - lls64) <= tol * np.abs(lls64)).all()
    # the library-free form runs the same steps: the same bits, and ll at the returned Q
    Qp, llp, nobs = project.project_q(xp, M, P, q0=Q, iters=12, tol=0.0, with_loglik=True)
    assert Qp.cpu().numpy().tobytes() == q.tobytes() and llp.cpu().numpy().tobytes() == ll.tobytes()
    assert np.array_equal(nobs.cpu().numpy(), (Gm != 3).sum(axis=1))
    Qu = project.project_q(xp, M, P, iters=3, tol=0.0)      # q0 = None: the uniform start
    want = R.iterate(Gm, P, np.full((b, K), 1.0 / K, dtype=np.float32), 3)[0]
    assert np.abs(Qu.cpu().numpy() - want).max() <= 1e-6


@pytest.mark.gpu
def test_engine_projects_every_head_like_the_library_free_form():
    import neural_admixture_amd as na
    from neural_admixture_amd import project
    from oracle import nadm_oracle as O
    dev = _dev()
    N, M, ks, Hd, C_ = 96, 3001, [3, 5], 32, 8
    Gm = O.synth_genotypes(N, M, 5, seed=3, missing=0.05)
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, C_)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(sum(ks), M)).astype(np.float32)
    p = O.make_params(42, V0, P0, Hd, ks)
    small = np.concatenate([p.g, p.W1.reshape(-1), p.b1] + [x for h in range(len(ks)) for x in (p.Wk[h].reshape(-1), p.bk[h])])
    e = na.Engine(M, C_, Hd, ks, dev, N)
    e.load_params(V0, P0, small)
    e.pack_from_host(torch.from_numpy(Gm))
    b = 70
    idx = torch.from_numpy(np.random.default_rng(1).permutation(N)[:b].astype(np.int32)).to(dev)
    q0 = e.infer_q(idx, b)
    same = e.project_q(idx, b, iters=0)
    assert all(torch.equal(a, c) for a, c in zip(q0, same))                       # iters = 0: the start, which defaults to infer_q's
    Qs, lls, nobs = e.project_q(idx, b, iters=6, tol=0.0, with_loglik=True)
    assert e.project_iters == 6
    o = 0
    for h, k in enumerate(ks):
        Ph = np.ascontiguousarray(P0[o:o + k].T)
        o += k
        assert np.array_equal(e.P(h).cpu().numpy(), Ph)
        Qh, llh, nh = project.project_q(e.xp, M, Ph, q0=q0[h], iters=6, tol=0.0, idx=idx, b=b, with_loglik=True)
        assert Qs[h].shape == (b, k) and torch.equal(Qs[h], Qh) and torch.equal(lls[h], llh) and torch.equal(nobs[h], nh)
        q64 = R.iterate(Gm[idx.cpu().numpy()], Ph, q0[h].cpu().numpy(), 6)[0]
        assert np.abs(Qh.cpu().numpy() - q64).max() <= 1e-6
    loose = e.project_q(idx, b, iters=6, tol=0.5)                                  # no entry moves by 0.5: one step, then the stop
    assert e.project_iters == 1
    one = e.project_q(idx, b, iters=1, tol=0.0)
    assert all(torch.equal(a, c) for a, c in zip(loose, one))
    # load_P: the decoder of a head replaced from a host matrix [M, k]
    newP = np.ascontiguousarray(1.0 - P0[:3].T)
    e.load_P(0, newP)
    assert np.array_equal(e.P(0).cpu().numpy(), newP) and np.array_equal(e.P(1).cpu().numpy(), P0[3:].T)
    with pytest.raises(RuntimeError, match="load_P"):
        e.load_P(1, newP)


def _set_missing(bed_bytes, N, sample, snps):
    """PLINK .bed bytes (SNP-major, 4 samples per byte, after the 3 magic bytes) with `sample`'s calls at `snps` set to missing (0b01)."""
    a = np.array(bed_bytes, dtype=np.uint8, copy=True)
    body = a[3:].reshape(-1, (N + 3) // 4)
    sh = 2 * (sample % 4)
    col = body[snps, sample // 4]
    body[snps, sample // 4] = (col & ~np.uint8(3 << sh)) | np.uint8(1 << sh)
    return a


@pytest.mark.gpu
def test_infer_refine_end_to_end_on_the_demo(tmp_path, caplog):
    """Train the demo for a few epochs, take 30 % of one sample's calls away in a copy of the data: `infer` without --refine writes the
    encoder's Q byte for byte as before; with --refine 20 the file differs, its rows sum to 1 and the logged log-likelihood rises."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli
    from neural_admixture_amd.io import read_bed_packed, write_outputs
    dev = _dev()
    d = np.load(f"{G}/demo_k3.npz")
    N, M = int(d["N"]), int(d["M"])
    d["bed_bytes"].tofile(tmp_path / "demo.bed")
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    out = tmp_path / "out"
    assert cli.main(["train", "--epochs", "5", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128"]) == 0
    snps = np.sort(np.random.default_rng(0).choice(M, size=int(0.3 * M), replace=False))
    _set_missing(d["bed_bytes"], N, 7, snps).tofile(tmp_path / "query.bed")
    (tmp_path / "query.fam").write_text("\n".join(["s"] * N) + "\n")
    data = read_bed_packed(str(tmp_path / "query.bed"), dev, True)
    assert data.flipped == read_bed_packed(str(tmp_path / "demo.bed")).flipped      # the query file's allele coding is the training data's
    assert (data.unpack_rows(7, 8)[0][snps] == 3).all()
    base = ["infer", "--name", "demo", "--save_dir", str(out), "--data_path", str(tmp_path / "query.bed")]
    assert cli.main(base + ["--out_name", "plain"]) == 0
    # what infer wrote before this option existed: engine.infer_q through write_outputs
    sd = torch.load(out / "demo.pt", map_location="cpu", weights_only=True)
    cfg = json.loads((out / "demo_config.json").read_text())
    model = na.Q_P(int(cfg["hidden_size"]), int(cfg["num_features"]), ks_list=cfg["ks"], is_train=False)
    model.load_state_dict(sd, device=dev, max_batch=1024)
    model.engine.pack_from_host(data)
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    write_outputs([q.cpu().numpy() for q in model.engine.infer_q(idx, N)], "want", 3, 3, 3, out)
    assert (out / "plain.3.Q").read_bytes() == (out / "want.3.Q").read_bytes()
    caplog.set_level(logging.INFO)
    caplog.clear()
    assert cli.main(base + ["--out_name", "refined", "--refine", "20"]) == 0
    assert (out / "refined.3.Q").read_bytes() != (out / "plain.3.Q").read_bytes()
    Qr = np.loadtxt(out / "refined.3.Q", dtype=np.float32)
    assert Qr.shape == (N, 3) and np.abs(Qr.sum(axis=1) - 1.0).max() < 1e-5 and Qr.min() > 0.0
    ll = [float(r.getMessage().split(":")[1]) for r in caplog.records if "Log-likelihood of the observed calls" in r.getMessage()]
    print("summed log-likelihood before / after refinement:", ll)
    assert len(ll) == 2 and ll[1] > ll[0]
