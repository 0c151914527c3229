"""The P half of the block EM over observed calls (nadm_project_p, project.p_step / project_p / polish, Engine.polish,
`train --polish`): P refitted against a fixed Q with masked EM steps, and the two halves alternated.  The float64 / float32 numpy
restatement lives in tests/project_p_oracle.py (the Q half: tests/project_oracle.py).

The 1e-6 bound on P is the margin tests/test_project_q.py uses for Q: the float32 restatement (fp32 sums over 64-sample slices, the
partials added in float64) lands 8e-8 .. 1.4e-7 from float64 in P, which leaves ~8x for another summation order and the hardware's
reciprocals."""
import builtins
import functools
import inspect
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_oracle as R  # noqa: E402
import project_p_oracle as PO  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
PP_CHUNK = 256               # SNPs per chunk of the accumulate kernel (csrc/nadm_snp_sweep.h: SWEEP_CHUNK); 64-sample tiles
ROWS = 200                   # resident rows of the GPU cases
GRID = [(b, M, K) for b in (1, 70, 130, 200) for M in (257, 513, 1027, 3001) for K in (2, 3, 8, 9, 16, 20)]
BIG = (4200, 257, 8)         # crosses the 4096 samples one fp32 running sum may cover


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("shape", [(130, 1027, 3), (130, 257, 8), (70, 513, 16)])
def test_restatement_never_lowers_the_likelihood_and_leaves_an_unobserved_snp(shape):
    N, M, K = shape
    Gm, P, Q, dead = PO.make_edge_case(N, M, K)
    assert (Gm[4] == 3).all() and (Gm[:, dead] == 3).all() and (P == 0).all(axis=1).any() and (P == 1).all(axis=1).any()
    assert Q[2].max() == 1.0 and P[dead].min() > 0.0
    Pn, Qn, lls = PO.alternate(Gm, P, Q, 6)
    assert len(lls) == 13 and (np.diff(lls) >= 0.0).all()
    assert Pn[dead].astype(np.float32).tobytes() == P[dead].tobytes()
    p64, n64 = PO.p_step(Gm, P, Q)
    p32, n32 = PO.p_step(Gm, P, Q, dtype=np.float32)
    assert np.array_equal(n32, n64) and n64[dead] == 0 and np.array_equal(n64, (Gm != 3).sum(axis=0))
    assert p32[dead].tobytes() == P[dead].tobytes() and p64[dead].astype(np.float32).tobytes() == P[dead].tobytes()
    assert np.abs(p32 - p64).max() < 2.5e-7


def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    Q = torch.full((4, 4), 0.25)
    P = torch.full((50, 4), 0.25)
    out = torch.empty((50, 4))
    scratch = torch.empty(4096)
    keep = (xp, P, Q, out, scratch)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, Q=Q.data_ptr(), q_stride=4, k=3, kp=4, Pin=P.data_ptr(), Pout=out.data_ptr(),
             eps=1e-6, pmin=1e-6, nobs_snp=None, scratch=scratch.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(xp=None), "null pointer"), (dict(Q=None), "null pointer"), (dict(Pin=None), "null pointer"), (dict(Pout=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(b=0), "empty batch"), (dict(b=-3), "empty batch"), (dict(M=0), "empty batch"),
    (dict(ld=12), "ld < ceil(M/4)"), (dict(ld=24), "ld must be a multiple of 16 and < 2^32"), (dict(ld=1 << 32), "ld must be a multiple of 16 and < 2^32"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"), (dict(q_stride=6), "q_stride must be a multiple of 4"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(pmin=-1e-3), "pmin must be in [0, 0.5)"), (dict(pmin=0.5), "pmin must be in [0, 0.5)"), (dict(pmin=float("nan")), "pmin must be in [0, 0.5)"),
    (dict(unaligned="Q"), "must be 16-byte aligned"), (dict(unaligned="Pout"), "must be 16-byte aligned"),
])
def test_project_p_refuses_before_any_launch(change, message):
    """Every refusal of nadm_project_p is decided on the host: it is reported with its message on a machine without a GPU."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    else:
        a.update(change)
    status = lib.nadm_project_p(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode()
    with pytest.raises(RuntimeError, match="nadm_project_p"):
        check(status, "project_p")
    del keep


def test_slices_are_a_rule_of_the_shape_and_the_scratch_grows_with_it():
    from neural_admixture_amd._lib import lib
    sl, f = lib.nadm_project_p_slices, lib.nadm_project_p_scratch_floats
    Ms = (1, 255, 256, 257, 513, 1027, 3001, 70000, 500000)
    bs = (1, 2, 63, 64, 65, 128, 129, 130, 200, 800, 4096, 4097, 4200, 100000)
    for M in Ms:
        assert all(int(sl(b, M)) == 1 for b in (1, 2, 63, 64))
        for b in bs:
            tiles = (b + 63) // 64
            s = int(sl(b, M))
            assert 1 <= s <= tiles and -(-tiles // s) <= 64                   # whole tiles; at most 4096 samples in a slice
    assert int(sl(130, 257)) >= 2
    assert int(sl(4200, 257)) >= 2 and int(sl(800, 500000)) == 1 and int(sl(100000, 500000)) >= 25
    for kp in (4, 8, 12, 16, 24, 64):
        for b in bs:
            v = [int(f(b, M, kp)) for M in Ms]
            assert v[0] > 0 and all(y >= x for x, y in zip(v, v[1:]))
            assert all(int(f(b, M, kp)) >= int(sl(b, M)) * ((M + PP_CHUNK - 1) // PP_CHUNK) * PP_CHUNK * (2 * kp + 1) for M in Ms)
        for M in Ms:
            v = [int(f(b, M, kp)) for b in range(1, 1400)] + [int(f(b, M, kp)) for b in bs[10:]]
            assert all(y >= x for x, y in zip(v, v[1:]))
    for M in range(1, 6000, 7):                                                # the wobble of ceil(1024 / chunks) * chunks is not in the size
        assert int(f(130, M + 7, 8)) >= int(f(130, M, 8)) and int(f(5000, M + 7, 8)) >= int(f(5000, M, 8))
    assert int(f(0, 100, 8)) == 0 and int(f(10, 0, 8)) == 0 and int(sl(0, 100)) == 0


def test_header_declares_the_three_symbols_and_the_binding_has_them():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for name in ("nadm_project_p", "nadm_project_p_slices", "nadm_project_p_scratch_floats"):
        assert name + "(" in header and name in EXPORTS
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14


def test_train_keeps_its_positional_signature_and_takes_polish_by_keyword():
    from neural_admixture_amd.train import train
    ps = inspect.signature(train).parameters
    positional = [n for n, p in ps.items() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["epochs", "batch_size", "learning_rate", "K", "seed", "data", "device", "num_gpus", "hidden_size", "master", "V",
                          "pops", "min_k", "max_k", "n_components"]
    assert [ps[n].default for n in ("min_k", "max_k", "n_components")] == [None, None, None]
    for name, default in (("polish", 0), ("polish_tol", 1e-5)):
        assert ps[name].kind == inspect.Parameter.KEYWORD_ONLY and ps[name].default == default
    # the refusals of the boundary function come before it touches its data
    with pytest.raises(ValueError, match="polish"):
        train(1, 8, 1e-3, 2, 0, None, torch.device("cpu"), 1, 8, True, None, ["a", "b"], polish=2)
    with pytest.raises(ValueError, match="polish"):
        train(1, 8, 1e-3, 2, 0, None, torch.device("cpu"), 2, 8, True, None, None, polish=2)


def test_cli_polish_flags_and_its_two_refusals(tmp_path, monkeypatch):
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    base = ["--k", "3", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "absent.bed")]
    a = cli.parse_train_args(base)
    assert a.polish == 0 and a.polish_tol == 1e-5
    a = cli.parse_train_args(base + ["--polish", "7", "--polish_tol", "1e-4"])
    assert a.polish == 7 and a.polish_tol == 1e-4
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)

    def no_open(*args, **kw):
        raise AssertionError(f"a file was opened before the refusal: {args[0]}")
    monkeypatch.setattr(builtins, "open", no_open)
    with pytest.raises(SystemExit, match=r"--polish is single-GPU"):
        cli.main(["train"] + base + ["--polish", "5", "--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--polish ignores labels"):
        cli.main(["train"] + base + ["--polish", "5", "--pops_path", str(tmp_path / "absent.pop")])


def test_sharded_engines_refuse_polish():
    """Engine.polish is single-GPU; the check comes first, so a stand-in without any device state shows it."""
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan = "dp", 2, None
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.polish(3)
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="single-GPU"):
        e.polish(3, 1e-5)


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(M, K):
    """ROWS resident rows with the edge cases of project_oracle.make_case and a SNP nobody observes; the tests leave them as they are."""
    Gm, P, Q, dead = PO.make_edge_case(ROWS, M, K)
    return Gm, P, Q, dead, _packed(Gm)


def _batch(b, rows=ROWS):
    """Rows of the batch: a permutation of the resident rows with the one-hot row 2, the all-missing row 4 and the 7-call row 5 in it,
    cut to b, the last entry a duplicate of the first; b = 1 is row 7."""
    if b == 1:
        return np.asarray([7], dtype=np.int32)
    perm = np.random.default_rng(b).permutation(rows)
    perm = np.concatenate([[2, 4, 5], perm[(perm != 2) & (perm != 4) & (perm != 5)]])[:b]
    perm = perm[np.random.default_rng(b + 1).permutation(b)]
    perm[-1] = perm[0]
    return perm.astype(np.int32)


def _gpu_pstep(xp, M, idx, P, Q, nobs=True, inplace=False, guard=0, eps=PO.EPS, pmin=PO.PMIN):
    """One nadm_project_p call -> (P_out [M, K] numpy, n [M] or None).  ``guard`` rows behind Pout hold a sentinel that must survive."""
    from neural_admixture_amd import project
    from neural_admixture_amd._lib import lib
    dev = xp.device
    b, K = Q.shape
    pin = project.pad_P(P, dev)
    kp = pin.shape[1]
    Qp = project.pad_Q(Q, b, K, kp, dev)
    buf = torch.full((M + guard, kp), 7.0, dtype=torch.float32, device=dev)
    pout = pin if inplace else buf[:M]
    no = torch.full((M,), -7, dtype=torch.int32, device=dev) if nobs else None
    scratch = torch.empty(int(lib.nadm_project_p_scratch_floats(b, M, kp)), dtype=torch.float32, device=dev)
    project.p_step(xp, M, None if idx is None else torch.from_numpy(idx).to(dev), b, Qp, K, pin, pout, scratch, eps, pmin, no)
    torch.cuda.synchronize()
    assert not pout[:, K:].any()                             # pad columns are written 0
    assert (buf[M:] == 7.0).all()                            # rows at or beyond M are never written
    return pout[:, :K].cpu().numpy(), None if no is None else no.cpu().numpy()


def _slice_counts(shapes):
    from neural_admixture_amd._lib import lib
    return {int(lib.nadm_project_p_slices(b, M)) for b, M, _ in shapes}


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K", GRID)
def test_one_step_against_float64(b, M, K):
    """max |P_gpu - P_f64| <= 1e-6, n_j exact, pad columns 0, the unobserved SNP's row bit-identical to the input.  Every case prints
    its figure before it asserts.  OBSERVED on an MI355X over the grid (96 cases): max |P_gpu - P_f64| 5.4e-8 .. 1.5e-7 (b = 1:
    <= 1.1e-7; the largest at b = 70, M = 3001, K = 20), the case without a gather list 1.1e-7 .. 1.3e-7; 1, 2, 3 and 4 sample slices."""
    dev = _dev()
    Gm, P, Q, dead, xph = _case(M, K)
    idx = _batch(b)
    Gb, Qb = Gm[idx], Q[idx]
    if b > 2:
        assert Qb.max(axis=1).max() == 1.0 and (Gb == 3).all(axis=1).sum() >= 1 and ((Gb != 3).sum(axis=1) == 7).sum() >= 1
        assert idx[-1] == idx[0] and len(set(idx[:-1].tolist())) == b - 1
    p64, n64 = PO.p_step(Gb, P, Qb)
    p, n = _gpu_pstep(xph.to(dev), M, idx, P, Qb, guard=3)
    dp = float(np.abs(p - p64).max())
    print(f"b={b} M={M} K={K}: max|P_gpu - P_f64| = {dp:.3e}, slices = {_slice_counts([(b, M, K)])}")
    assert np.array_equal(n, n64) and n[dead] == 0
    assert dp <= 1e-6
    assert p[dead].tobytes() == P[dead].tobytes()
    assert p[n64 == 0].tobytes() == P[n64 == 0].tobytes()
    if b == 70 and M == 1027:                                # rows 0..b without a gather list
        p0, n0 = _gpu_pstep(xph.to(dev), M, None, P, Q[:b])
        w0, wn = PO.p_step(Gm[:b], P, Q[:b])
        d0 = float(np.abs(p0 - w0).max())
        print(f"   without a gather list: max|P_gpu - P_f64| = {d0:.3e}")
        assert d0 <= 1e-6 and np.array_equal(n0, wn) and p0[dead].tobytes() == P[dead].tobytes()


@pytest.mark.gpu
def test_a_batch_beyond_4096_samples_and_the_guard_rows():
    """b = 4200 gathered with duplicates from 130 rows: more samples than one fp32 running sum may cover, so the float64 combination
    of the slices' partials is on the path.  Pout has guard rows beyond M whose sentinel must survive.  OBSERVED on an MI355X:
    max |P_gpu - P_f64| 5.4e-8 with 66 slices."""
    dev = _dev()
    b, M, K = BIG
    Gm, P, Q, dead, xph = _case(M, K)
    idx = np.random.default_rng(9).integers(0, 130, size=b).astype(np.int32)
    assert len(set(idx.tolist())) == 130
    p64, n64 = PO.p_step(Gm[idx], P, Q[idx])
    p, n = _gpu_pstep(xph.to(dev), M, idx, P, Q[idx], guard=5)
    dp = float(np.abs(p - p64).max())
    seen = _slice_counts(GRID + [BIG])
    print(f"b={b} M={M} K={K}: max|P_gpu - P_f64| = {dp:.3e}; slice counts over the grid and this case: {sorted(seen)}")
    assert np.array_equal(n, n64) and dp <= 1e-6 and p[dead].tobytes() == P[dead].tobytes()
    assert 1 in seen and max(seen) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 16, 20])
def test_a_missing_call_and_the_pad_bits_contribute_exactly_nothing(K):
    """For a SNP j, the Q rows of exactly the samples whose call at j is missing are changed and every bit of the packed rows that
    holds no SNP is set: row j of Pout and n_j come out bit-identical; a SNP those samples do observe moves."""
    dev = _dev()
    M, b = 1027, 130
    Gm, P, Q, dead, xph = _case(M, K)
    want_p, want_n = _gpu_pstep(xph.to(dev), M, None, P, Q[:b])
    dirty = _packed(Gm, dirty=True).to(dev)
    for j in (0, 255, 256, 600, dead, M - 1):
        miss = Gm[:b, j] == 3
        assert miss.any()
        Q2 = Q[:b].copy()
        Q2[miss] = np.roll(Q2[miss], 1, axis=1) * 0.5 + 0.5 / K
        got_p, got_n = _gpu_pstep(dirty, M, None, P, Q2)
        assert want_p[j].tobytes() == got_p[j].tobytes() and want_n[j] == got_n[j]
        seen = ((Gm[:b] != 3) & miss[:, None]).any(axis=0) & (P.min(axis=1) > 0) & (P.max(axis=1) < 1)
        assert seen.any() and not np.array_equal(want_p[seen], got_p[seen])      # (SNPs those samples observe do move)
        assert np.array_equal(want_n, got_n)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 20])
def test_two_launches_agree_bit_for_bit_and_in_place_equals_out_of_place(K):
    dev = _dev()
    M, b = 3001, 200
    Gm, P, Q, dead, xph = _case(M, K)
    xp, idx = xph.to(dev), _batch(b)
    one = _gpu_pstep(xp, M, idx, P, Q[idx])
    two = _gpu_pstep(xp, M, idx, P, Q[idx])
    inp = _gpu_pstep(xp, M, idx, P, Q[idx], inplace=True)
    non = _gpu_pstep(xp, M, idx, P, Q[idx], nobs=False)
    for x, y, z in zip(one, two, inp):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert non[0].tobytes() == one[0].tobytes() and non[1] is None


def _gpu_ll(project, xp, M, N, Pp, k, Qp):
    """Summed log-likelihood of the observed calls at (P, Q): the ll of a Q step (at its INPUT), float64."""
    _, lls, _, _ = project.refine_heads(xp, M, None, N, [Pp], [k], [Qp], 0, 0.0, with_loglik=True)
    return float(lls[0].sum())


@pytest.mark.gpu
def test_twelve_alternating_rounds_raise_the_likelihood_and_follow_the_float64_trajectory():
    """(130, 2050, 8), P in [0.02, 0.98] so that no clip is active: the summed log-likelihood rises every half round, the final Q and P
    are within 1e-6 of the float64 trajectory (the float32 restatement: 8e-8 and 2e-7), project.polish gives the bits of the
    hand-rolled loop.  The edge cases are left out on purpose: at the clip float32 and float64 trajectories separate by up to 1.5e-3,
    and the restatement's do too.  OBSERVED on an MI355X: summed ll -285330.655 -> -271487.403 (float64: -285330.647 -> -271487.395),
    smallest half-round gain 166; after 12 rounds max |Q_gpu - Q_f64| 2.4e-7, max |P_gpu - P_f64| 2.7e-7."""
    from neural_admixture_amd import project
    from neural_admixture_amd._lib import lib
    dev = _dev()
    N, M, K = 130, 2050, 8
    Gm, P, Q = R.make_case(N, M, K, edge=False)
    assert P.min() >= 0.02 and P.max() <= 0.98
    xp = _packed(Gm).to(dev)
    P64, Q64, lls64 = PO.alternate(Gm, P, Q, 12)
    Pc = project.pad_P(P, dev)
    Qc = project.pad_Q(Q, N, K, Pc.shape[1], dev)
    qs = torch.empty(int(lib.nadm_project_scratch_floats(N, M, Pc.shape[1])), dtype=torch.float32, device=dev)
    ps = torch.empty(int(lib.nadm_project_p_scratch_floats(N, M, Pc.shape[1])), dtype=torch.float32, device=dev)
    lls = [_gpu_ll(project, xp, M, N, Pc, K, Qc)]
    for _ in range(12):
        qn, pn = torch.empty_like(Qc), torch.empty_like(Pc)
        project.em_step(xp, M, None, N, Pc, K, Qc, qn, qs)
        lls.append(_gpu_ll(project, xp, M, N, Pc, K, qn))
        project.p_step(xp, M, None, N, qn, K, Pc, pn, ps)
        lls.append(_gpu_ll(project, xp, M, N, pn, K, qn))
        Qc, Pc = qn, pn
    lls = np.asarray(lls)
    dq = float(np.abs(Qc[:, :K].cpu().numpy() - Q64).max())
    dp = float(np.abs(Pc[:, :K].cpu().numpy() - P64).max())
    print(f"summed ll {lls[0]:.3f} -> {lls[-1]:.3f} (float64: {lls64[0]:.3f} -> {lls64[-1]:.3f}), smallest half-round gain {np.diff(lls).min():.3e}; "
          f"after 12 rounds max|Q_gpu - Q_f64| = {dq:.3e}, max|P_gpu - P_f64| = {dp:.3e}")
    assert (np.diff(lls) > 0).all()
    assert dq <= 1e-6 and dp <= 1e-6
    Ps, Qs, ll0, ll1, ran = project.polish(xp, M, [P], [Q], 12, tol=0.0)
    assert ran == 12 and torch.equal(Ps[0], Pc[:, :K]) and torch.equal(Qs[0], Qc[:, :K])
    assert ll0 == pytest.approx(lls[0], rel=1e-12) and ll1 == pytest.approx(lls[-1], rel=1e-12)
    early = project.polish(xp, M, [P], [Q], 12, tol=0.5)            # nothing moves by 0.5: one round, then the stop
    once = project.polish(xp, M, [P], [Q], 1, tol=0.0)
    assert early[4] == 1 and torch.equal(early[0][0], once[0][0]) and torch.equal(early[1][0], once[1][0])
    none = project.polish(xp, M, [P], [Q], 0)                       # no round: the start, padded and cut again
    assert none[4] == 0 and none[2] == none[3] and np.array_equal(none[0][0].cpu().numpy(), P)


@pytest.mark.gpu
def test_polish_recovers_the_frequencies_where_calls_are_missing():
    """130 x 1027, K = 3, 40 % of the calls missing at every third SNP, from the fit that reads a missing call as genotype 0 and the
    true Q, ten rounds: mean P / F at the heavy SNPs in [0.97, 1.03], their RMSE below half the start's, P within 1e-5 of the float64
    restatement's.  The restatement (float64): mean P / F 0.603 -> 1.011, RMSE 0.236 -> 0.084 (the lightly missing SNPs: 0.067 -> 0.066).
    OBSERVED on an MI355X: the same figures to three digits, max |P_gpu - P_f64| 1.1e-7; project_p from the flat start 1.1e-7."""
    from neural_admixture_amd import project
    dev = _dev()
    Gm, F, Q, P0, hv = PO.make_recovery_case()
    M = Gm.shape[1]
    start = PO.recovery_figures(P0, F, hv)
    P64, _, _ = PO.alternate(Gm, P0, Q, 10)
    xp = _packed(Gm).to(dev)
    Ps, Qs, ll0, ll1, ran = project.polish(xp, M, [P0], [Q], 10, tol=0.0)
    Pg = Ps[0].cpu().numpy()
    end = PO.recovery_figures(Pg, F, hv)
    dp = float(np.abs(Pg - P64).max())
    print(f"mean P/F at the heavy SNPs {start[0]:.3f} -> {end[0]:.3f}, their RMSE {start[1]:.3f} -> {end[1]:.3f}, the others' {start[2]:.3f} -> "
          f"{end[2]:.3f}; ll {ll0:.3f} -> {ll1:.3f}; max|P_gpu - P_f64| = {dp:.3e}")
    assert ran == 10 and ll1 > ll0
    assert abs(start[0] - 0.6) < 0.03 and 0.97 <= end[0] <= 1.03
    assert end[1] < 0.5 * start[1]
    assert dp <= 1e-5
    # frequencies for a fixed Q from the flat start: the first step is the ancestry-weighted allele frequency, later ones follow the restatement
    Pq = project.project_p(xp, M, Q, iters=4, tol=0.0)
    want = np.full((M, 3), 0.5)
    for _ in range(4):
        want = PO.p_step(Gm, want, Q)[0]
    dq = float(np.abs(Pq.cpu().numpy() - want).max())
    print(f"project_p, four steps from 0.5: max|P_gpu - P_f64| = {dq:.3e}")
    assert dq <= 1e-6


@pytest.mark.gpu
def test_engine_polish_equals_the_library_free_form_and_leaves_the_parameters():
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
    bmax = 40                                                                     # rows per encoder batch: three batches
    e = na.Engine(M, C_, Hd, ks, dev, bmax)
    e.load_params(V0, P0, small)
    e.pack_from_host(torch.from_numpy(Gm))
    e.sync()
    before = [t.clone() for t in (e.pflat, e.mflat, e.vflat)]
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    parts = [e.infer_q(idx[s:s + bmax], min(bmax, N - s)) for s in range(0, N, bmax)]
    q0 = [torch.cat([q[h] for q in parts], dim=0) for h in range(len(ks))]
    Ps, Qs, ll0, ll1, ran = e.polish(4, 0.0)
    want = project.polish(e.xp, M, [e.P(h).clone() for h in range(len(ks))], q0, 4, tol=0.0)
    assert ran == 4 and want[4] == 4 and ll1 > ll0 and (ll0, ll1) == (want[2], want[3])
    for h, k in enumerate(ks):
        assert Ps[h].shape == (M, k) and Qs[h].shape == (N, k)
        assert torch.equal(Ps[h], want[0][h]) and torch.equal(Qs[h], want[1][h])
        assert not torch.equal(Ps[h], e.P(h))
    e.sync()
    for t, w in zip((e.pflat, e.mflat, e.vflat), before):
        assert torch.equal(t, w)


def _inject_missing(bed_bytes, N, snps, frac, seed):
    """PLINK .bed bytes (SNP-major, 4 samples per byte, after the 3 magic bytes) with ``frac`` of the samples' calls at ``snps`` set
    to missing (0b01)."""
    a = np.array(bed_bytes, dtype=np.uint8, copy=True)
    body = a[3:].reshape(-1, (N + 3) // 4)
    rng = np.random.default_rng(seed)
    for j in snps:
        for i in np.nonzero(rng.random(N) < frac)[0]:
            sh = 2 * (i % 4)
            body[j, i // 4] = (body[j, i // 4] & ~np.uint8(3 << sh)) | np.uint8(1 << sh)
    return a


@pytest.mark.gpu
def test_train_polish_end_to_end_on_the_demo(tmp_path, caplog):
    """The bundled demo with 40 % of the calls taken away at every 50th SNP, three epochs: with --polish 5 the logged log-likelihood
    after is at least the one before, the written .P differs from the unpolished run's at the injected SNPs, and the checkpoint's
    tensors equal those of the same run without --polish."""
    from neural_admixture_amd import cli
    _dev()
    d = np.load(f"{G}/demo_k3.npz")
    N, M = int(d["N"]), int(d["M"])
    snps = np.arange(0, M, 50)
    _inject_missing(d["bed_bytes"], N, snps, 0.4, 0).tofile(tmp_path / "demo.bed")
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    common = ["train", "--epochs", "3", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--seed", "42",
              "--batch_size", "800", "--hidden_size", "128"]
    assert cli.main(common + ["--save_dir", str(tmp_path / "plain")]) == 0
    caplog.set_level(logging.INFO)
    caplog.clear()
    assert cli.main(common + ["--save_dir", str(tmp_path / "polished"), "--polish", "5"]) == 0
    msgs = [r.getMessage() for r in caplog.records]
    ll = [float(m.split(":")[1]) for m in msgs if "Log-likelihood of the observed calls" in m]
    rounds = [int(m.split(":")[1]) for m in msgs if "Polishing rounds run" in m]
    reported = [float(m.split(":")[1].rstrip(".")) for m in msgs if m.strip().startswith("Log-likelihood:")]
    print("log-likelihood before / after polishing:", ll, "rounds:", rounds, "reported for the returned matrices:", reported)
    assert len(ll) == 2 and ll[1] >= ll[0] and rounds == [5]
    # the run reports the matrices it returns.  Its report is the float64 reduction of report.py, which clips g to [eps, 2 - eps] like the
    # reference: per genotype that moves a term of order 1 by at most eps |log r - log(1 - r)| <= 1.4e-5, the kernel's fp32 logarithms by
    # ~1e-7 -- 2e-4 relative covers both with a wide margin and is far below the gain of the polish
    assert len(reported) == 1 and reported[0] == pytest.approx(ll[1], rel=2e-4) and abs(reported[0] - ll[1]) < abs(reported[0] - ll[0])
    Pa = np.loadtxt(tmp_path / "plain" / "demo.3.P", dtype=np.float32)
    Pb = np.loadtxt(tmp_path / "polished" / "demo.3.P", dtype=np.float32)
    Qb = np.loadtxt(tmp_path / "polished" / "demo.3.Q", dtype=np.float32)
    assert Pa.shape == Pb.shape == (M, 3) and (np.abs(Pa[snps] - Pb[snps]).max(axis=1) > 0).all()
    assert Qb.shape == (N, 3) and np.abs(Qb.sum(axis=1) - 1.0).max() < 1e-5
    sa = torch.load(tmp_path / "plain" / "demo.pt", map_location="cpu", weights_only=True)
    sb = torch.load(tmp_path / "polished" / "demo.pt", map_location="cpu", weights_only=True)
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
