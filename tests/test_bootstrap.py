"""Bootstrap standard errors for Q (nadm_project_q_w, bootstrap.block_weights / bootstrap_q, Engine.bootstrap_q, the `bootstrap` mode
and `train --bootstrap`).  The numpy restatement lives in tests/bootstrap_oracle.py."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_oracle as BO  # noqa: E402
import cv_oracle as CO  # noqa: E402
import project_oracle as R  # noqa: E402
from packed_rows import dev as _dev, packed as _packed  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
SEED_WIDE = (1 << 40) + 3    # a seed with bits above 2^32


# ------------------------------------------------------------------------------------------------ CPU: the draw
def test_the_worked_values_of_the_header_reproduce():
    """include/nadm.h prints two row keys, the draws of replicate 0 over 12 blocks and the counts of replicates 0 and 1."""
    from neural_admixture_amd import bootstrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    for text in ("row_key(0, 0) = 0x01FCE552", "row_key(0, 1) = 0xB21C8E52", "8 7 0 5 2 4 11 2 4 10 11 3", "cnt = 1 0 2 1 2 1 0 1 1 0 1 2",
                 "cnt = 2 1 1 0 1 1 2 3 0 0 0 1"):
        assert text in header
    assert int(CO.row_key(0, 0)) == 0x01FCE552 and int(CO.row_key(0, 1)) == 0xB21C8E52
    assert BO.draws(12, 1, 0, 0).tolist() == [8, 7, 0, 5, 2, 4, 11, 2, 4, 10, 11, 3]
    for fn in (BO.block_counts, bootstrap.block_counts):
        assert fn(12, 1, 0, 0).tolist() == [1, 0, 2, 1, 2, 1, 0, 1, 1, 0, 1, 2]
        assert fn(12, 1, 0, 1).tolist() == [2, 1, 1, 0, 1, 1, 2, 3, 0, 0, 0, 1]
        assert fn(48, 4, 0, 0).tolist() == [1, 0, 2, 1, 2, 1, 0, 1, 1, 0, 1, 2]          # the draw knows the blocks, not the SNPs


@pytest.mark.parametrize("M, block", [(257, 1), (1027, 64), (3001, 256)])
def test_block_weights_equal_the_restatement_sum_to_nb_and_handle_a_short_last_block(M, block):
    from neural_admixture_amd import bootstrap
    nb = -(-M // block)
    seen = []
    for seed, rep in ((0, 0), (0, 1), (42, 0), (SEED_WIDE, 7)):
        w = bootstrap.block_weights(M, block, seed, rep)
        assert w.dtype == np.uint8 and w.shape == (M,)
        assert np.array_equal(w, BO.block_weights(M, block, seed, rep))
        cnt = bootstrap.block_counts(M, block, seed, rep)
        assert cnt.shape == (nb,) and int(cnt.sum()) == nb
        assert np.array_equal(w, np.repeat(cnt, block)[:M])                # every SNP of a block carries the block's count ...
        short = M - (nb - 1) * block
        assert 0 < short <= block and (w[M - short:] == cnt[-1]).all()       # ... the short last block too
        assert int(w.astype(np.int64).sum()) == int((cnt * np.minimum(block, M - np.arange(nb) * block)).sum())
        seen.append(w)
    assert all(not np.array_equal(a, b) for i, a in enumerate(seen) for b in seen[i + 1:])      # replicates and seeds differ
    assert bootstrap.n_blocks(M, block) == nb


def test_the_draw_refuses_what_it_is_not_defined_for():
    from neural_admixture_amd import bootstrap
    for args, msg in (((100, 100, 0, 0), "at least 2 blocks"), ((100, 200, 0, 0), "at least 2 blocks"), (((1 << 31) + 1, 1, 0, 0), r"M must be in 1..2\^31"),
                      ((0, 1, 0, 0), r"M must be in 1..2\^31"), ((100, 0, 0, 0), "block must be >= 1"), ((100, 1, -1, 0), "seed must be in"),
                      ((100, 1, 0, -1), "rep must be in")):
        with pytest.raises(RuntimeError, match=msg):
            bootstrap.block_weights(*args)
    w = bootstrap.block_weights(200000, 1, 5, 0)                            # shares of a Poisson(1) draw: P(0) = P(1) = 0.368
    assert abs(float((w == 0).mean()) - 0.3679) < 0.005 and abs(float((w == 1).mean()) - 0.3679) < 0.005 and int(w.max()) < 12


# ------------------------------------------------------------------------------------------------ CPU: the restatement
def test_restated_weighted_step_unit_weights_duplication_and_zero_weights():
    """w = 1 is project_oracle.em_step bit for bit (both precisions); weight 2 is the SNP written twice; a zero-weight SNP may hold
    any P and any call.  Prints how far the float32 restatement lands from float64 on the weights of the GPU test."""
    Gm, P, Q = R.make_case(70, 1027, 8)
    one = np.ones(1027, dtype=np.int64)
    for dt in (np.float64, np.float32):
        for a, b in zip(BO.em_step_w(Gm, P, Q, one, dtype=dt), R.em_step(Gm, P, Q, dtype=dt)):
            assert np.array_equal(a, b)
    w = _weights(1027)
    q64, ll64, n64 = BO.em_step_w(Gm, P, Q, w)
    twice = np.repeat(np.arange(1027), w)
    qd, lld, nd = R.em_step(Gm[:, twice], P[twice], Q)
    assert np.abs(qd - q64).max() < 1e-13 and np.array_equal(nd, n64) and np.allclose(lld, ll64, rtol=1e-12, atol=0)
    zero = w == 0
    G2, P2 = Gm.copy(), P.copy()
    G2[:, zero] = (Gm[:, zero] + 1) % 4
    P2[zero] = 0.5
    for a, b in zip(BO.em_step_w(G2, P2, Q, w), (q64, ll64, n64)):
        assert np.array_equal(a, b)
    q32, _, n32 = BO.em_step_w(Gm, P, Q, w, dtype=np.float32)
    print(f"float32 restatement of the weighted step: max |Q32 - Q64| = {float(np.abs(q32 - q64).max()):.3e}")
    assert np.array_equal(n32, n64) and np.abs(q32 - q64).max() < 2.5e-7
    p1, q1 = BO.block_em_w(Gm, np.clip(P, 0.02, 0.98), Q, None, 4)
    p2, q2 = CO.block_em(Gm, np.clip(P, 0.02, 0.98), Q, 4)
    assert np.abs(p1 - p2).max() < 1e-12 and np.abs(q1 - q2).max() < 1e-12


def test_calibration_of_the_restated_procedure():
    """Planted panel 60 x 1536, K = 3, 5 % missing, six near-pure samples.  The bootstrap SE of ONE panel (B = 50, every fit 30 rounds
    from the truth / the centre) against the spread of the estimate over 40 independently drawn panels (each fitted from the truth for
    30 rounds; standard deviation), over the entries with 0.05 < Q < 0.95 of that panel's estimate.  The ratio is
    rms(SE) / rms(spread) -- the ratio of the two root mean squares, which a single noisy spread does not dominate the way the mean
    of entrywise ratios is dominated.  It must lie in [0.75, 1.33] at block 1 and block 64: the band covers the sampling noise of 50
    replicates and 40 panels.  MEASURED (seeds as below): 1.00 at block 1, 0.98 at block 64 (the rms of the entrywise ratios reads
    1.05 and 1.03); block 256 leaves 6 blocks at this width, reads 0.95 here and is not asserted: that is the case the
    `fewer than 50 blocks` warning is for."""
    P, Q = BO.planted_truth(seed=7)
    fits = np.stack([BO.block_em_w(BO.planted_panel(P, Q, 100 + i), P, Q, None, 30)[1] for i in range(40)])
    spread = fits.std(axis=0, ddof=1)
    Gm = BO.planted_panel(P, Q, 100)
    ratios = {}
    for block in (1, 64, 256):
        qc, se, _ = BO.bootstrap_q(Gm, P, Q, 50, block, 30, 0)
        sel = (qc > 0.05) & (qc < 0.95)
        assert sel.sum() > 100
        ratios[block] = float(np.sqrt((se[sel] ** 2).mean() / (spread[sel] ** 2).mean()))
        print(f"block {block}: {BO.n_blocks(1536, block)} blocks, rms(SE) / rms(spread) = {ratios[block]:.3f} over {int(sel.sum())} entries")
    assert 0.75 <= ratios[1] <= 1.33
    assert 0.75 <= ratios[64] <= 1.33


# ------------------------------------------------------------------------------------------------ CPU: interface and refusals
def _refusal_args():
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    P = torch.full((50, 4), 0.25)
    Q = torch.full((4, 4), 0.25)
    out = torch.empty((4, 4))
    scratch = torch.empty(64)
    w = torch.ones(64, dtype=torch.uint8)
    keep = (xp, P, Q, out, scratch, w)
    a = dict(xp=xp.data_ptr(), ld=16, idx=None, b=4, M=50, P=P.data_ptr(), k=3, kp=4, Qin=Q.data_ptr(), Qout=out.data_ptr(), q_stride=4,
             eps=1e-6, qmin=1e-6, loglik=None, nobs=None, scratch=scratch.data_ptr(), w=w.data_ptr(), stream=None)
    return a, keep


@pytest.mark.parametrize("change, message", [
    (dict(w=None), "null pointer"),
    (dict(xp=None), "null pointer"), (dict(P=None), "null pointer"), (dict(Qin=None), "null pointer"), (dict(Qout=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(ld=12), "ld < ceil(M/4)"),
    (dict(k=0), "K must be in 1..NADM_MAX_K"), (dict(k=65, kp=64), "K must be in 1..NADM_MAX_K"),
    (dict(kp=8), "kp must be nadm_pad_k(k)"), (dict(k=5), "kp must be nadm_pad_k(k)"),
    (dict(q_stride=3), "q_stride < kp"),
    (dict(eps=0.0), "eps must be in [1e-9, 0.5)"), (dict(eps=0.5), "eps must be in [1e-9, 0.5)"), (dict(eps=float("nan")), "eps must be in [1e-9, 0.5)"),
    (dict(b=0), "empty batch"), (dict(b=-3), "empty batch"),
    (dict(qmin=1.0), "qmin must be in [0, 1)"),
    (dict(unaligned="w"), "w must be 16-byte aligned"), (dict(unaligned="xp"), "16-byte aligned"),
])
def test_project_q_w_refuses_before_any_launch(change, message):
    """Every refusal of nadm_project_q_w -- the set of nadm_project_q and a missing or misaligned w -- is decided on the host: it is
    reported with its message, under its own name, on a machine without a GPU."""
    from neural_admixture_amd._lib import lib, check
    a, keep = _refusal_args()
    if "unaligned" in change:
        a[change["unaligned"]] += 4
    else:
        a.update(change)
    status = lib.nadm_project_q_w(*a.values())
    assert status != 0 and message in lib.nadm_last_error().decode() and lib.nadm_last_error().decode().startswith("nadm_project_q_w: ")
    with pytest.raises(RuntimeError, match="nadm_project_q_w"):
        check(status, "project_q_w")
    del keep


def test_header_declares_the_symbol_and_the_binding_has_it():
    from neural_admixture_amd._lib import EXPORTS, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nadm.h")).read()
    assert "nadm_project_q_w(" in header and "nadm_project_q_w" in EXPORTS and hasattr(lib, "nadm_project_q_w")
    assert "#define NADM_ABI_VERSION 14" in header and lib.nadm_abi_version() == 14
    assert "| `nadm_project_q_w`" in open(os.path.join(root, "INTEGRATION.md")).read()


def test_python_layer_checks_its_arguments_without_a_gpu():
    from neural_admixture_amd import bootstrap, project
    xp = torch.zeros((4, 16), dtype=torch.uint8)
    P, Q = np.full((50, 2), 0.5), np.full((4, 2), 0.5)
    for kw, msg in ((dict(B=1), "B >= 2"), (dict(rounds=0), "rounds must be >= 1"), (dict(block=50), "at least 2 blocks"),
                    (dict(seed=-1), "seed must be in")):
        with pytest.raises(RuntimeError, match=msg):
            bootstrap.bootstrap_q(xp, 50, [P], [Q], **kw)
    with pytest.raises(RuntimeError, match="one P and one Q per head"):
        bootstrap.bootstrap_q(xp, 50, [P], [])
    with pytest.raises(RuntimeError, match="must be on a ROCm GPU"):
        bootstrap.bootstrap_q(xp, 50, [P], [Q], B=2)
    q, scratch = torch.full((4, 4), 0.25), torch.empty(64)
    for bad in (torch.ones(50), torch.ones(49, dtype=torch.uint8), torch.ones((50, 1), dtype=torch.uint8), torch.ones(100, dtype=torch.uint8)[::2]):
        with pytest.raises(RuntimeError, match="weights must be a contiguous uint8 vector of 50 entries"):
            project.em_step(xp, 50, None, 4, torch.full((50, 4), 0.25), 3, q, q, scratch, weights=bad)
    with pytest.raises(RuntimeError, match=r"sum to more than 2\^31 - 1"):
        project.check_weights(torch.full((8500000,), 255, dtype=torch.uint8), 8500000)
    project.check_weights(torch.full((8400000,), 255, dtype=torch.uint8), 8400000)


def _fake_results(nb=1536):
    from neural_admixture_amd.bootstrap import BootResult
    se = torch.tensor([[0.01, 0.02, 0.03], [0.0, 0.005, 0.005]], dtype=torch.float64)
    bias = torch.tensor([[0.001, -0.002, 0.001], [0.0, 0.0005, -0.0005]], dtype=torch.float64)
    return [BootResult(3, torch.full((2, 3), 1 / 3), se, bias, 0.0123, 7, [4, 6], False, nb),
            BootResult(2, torch.full((2, 2), 0.5), se[:, :2], bias[:, :2], 0.2, 10, [10, 3], True, nb)]


def test_written_files_and_log_lines(tmp_path, caplog):
    from neural_admixture_amd import bootstrap
    res = _fake_results()
    bootstrap.write_results(tmp_path / "o", "run", res)
    for r in res:
        se, bias = np.loadtxt(tmp_path / "o" / f"run.{r.k}.Q_se", ndmin=2), np.loadtxt(tmp_path / "o" / f"run.{r.k}.Q_bias", ndmin=2)
        assert np.array_equal(se, r.se.float().numpy().astype(np.float64)) and np.array_equal(bias, r.bias.float().numpy().astype(np.float64))
    assert (tmp_path / "o" / "run.3.Q_se").read_text().splitlines()[0].count(" ") == 2          # the .Q text format: K columns, one space
    caplog.set_level(logging.INFO)
    bootstrap.log_results(res, logging.getLogger("test_bootstrap"), 10)
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("Bootstrap SE (K=3): mean 0.01167, max 0.03000 over 2 replicates of 1536 blocks") and "0.01230" in m for m in msgs)
    assert any(m.startswith("Bootstrap SE (K=2): ") for m in msgs)
    warn = [m for m in msgs if "--boot_rounds" in m]
    assert len(warn) == 1 and "K = 2 " in warn[0] and "limit of 10 rounds" in warn[0] and "too small" in warn[0]
    assert not any("blocks of SNPs to draw from" in m for m in msgs)
    caplog.clear()
    bootstrap.log_results(_fake_results(nb=6), logging.getLogger("test_bootstrap"), 10)
    few = [r.getMessage() for r in caplog.records if "blocks of SNPs to draw from" in r.getMessage()]
    assert len(few) == 1 and "only 6 blocks" in few[0] and "--block" in few[0]


def test_cli_flags_defaults_and_refusals_before_any_data_is_read(tmp_path, monkeypatch):
    """Argument errors and missing files end the run with the offender named, before the GPU check (there is no GPU as far as the mode
    can tell) and before a genotype is read (the reader is a stand-in that fails the test)."""
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    bed = tmp_path / "x.bed"
    common = ["--name", "run", "--save_dir", str(tmp_path), "--data_path", str(bed)]
    a = cli.parse_bootstrap_args(common + ["--k", "3"])
    assert (a.replicates, a.block, a.boot_rounds, a.boot_tol, a.seed, a.out_name, a.extract, a.threads) == (200, 1, 50, 1e-5, 42, None, None, 1)
    a = cli.parse_bootstrap_args(common + ["--min_k", "2", "--max_k", "4", "-B", "20", "--block", "500", "--boot_rounds", "80", "--boot_tol", "1e-6"])
    assert (a.replicates, a.block, a.boot_rounds, a.boot_tol, a.k, a.min_k, a.max_k) == (20, 500, 80, 1e-6, None, 2, 4)
    assert cli.parse_bootstrap_args(common + ["--k", "3", "--replicates", "7"]).replicates == 7
    a = cli.parse_train_args(common + ["--k", "3"])
    assert (a.bootstrap, a.block, a.boot_rounds, a.boot_tol) == (0, 1, 50, 1e-5)

    def no_read(*args, **kw):
        raise AssertionError("the genotypes were read before the refusal")
    monkeypatch.setattr(cli, "_read", no_read)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    span = ["--min_k", "2", "--max_k", "3"]
    with pytest.raises(AssertionError, match='"bootstrap" puts standard errors on Q'):
        cli.main(["boot"] + common)
    with pytest.raises(SystemExit, match=r"--k cannot be given together with --min_k"):
        cli.main(["bootstrap"] + common + ["--k", "3", "--min_k", "2", "--max_k", "3"])
    with pytest.raises(SystemExit, match=r"provide either --k or both --min_k and --max_k"):
        cli.main(["bootstrap"] + common + ["--min_k", "2"])
    for flags, msg in ((["-B", "1"], r"--replicates must be >= 2"), (["--block", "0"], r"--block must be >= 1"),
                       (["--boot_rounds", "0"], r"--boot_rounds must be >= 1"), (["--boot_tol", "nan"], r"--boot_tol must be >= 0"),
                       (["--seed", "-1"], r"--seed must be >= 0")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(["bootstrap"] + common + span + flags)
    with pytest.raises(SystemExit, match=r"Unrecognized file format"):
        cli.main(["bootstrap"] + common[:-1] + [str(tmp_path / "x.pgen")] + span)
    np.savetxt(tmp_path / "run.2.P", np.full((10, 2), 0.5))
    np.savetxt(tmp_path / "run.2.Q", np.full((5, 2), 0.5))
    np.savetxt(tmp_path / "run.3.Q", np.full((5, 3), 1 / 3))
    with pytest.raises(SystemExit, match=r"bootstrap needs .*run\.3\.P not found"):          # a missing .P for one of several Ks
        cli.main(["bootstrap"] + common + span)
    np.savetxt(tmp_path / "run.3.P", np.full((9, 3), 0.5))
    (tmp_path / "x.fam").write_text("\n".join(["s"] * 5) + "\n")
    bed.write_bytes(bytes(3 + 2 * 10))                                     # N = 5, M = 10
    with pytest.raises(SystemExit, match=r"run\.3\.P holds a 9 x 3 matrix, the model needs 10 x 3"):
        cli.main(["bootstrap"] + common + span)
    np.savetxt(tmp_path / "run.3.P", np.full((10, 3), 0.5))
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):             # everything is in order: the GPU check is what is left
        cli.main(["bootstrap"] + common + span)
    assert not list(tmp_path.glob("*.Q_se")) and not list(tmp_path.glob("*.Q_bias"))
    train = ["train"] + common + ["--k", "3", "--bootstrap", "5"]
    with pytest.raises(SystemExit, match=r"--bootstrap is single-GPU: run it with --num_gpus 1"):
        cli.main(train + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=r"--bootstrap ignores labels: it is not available with --pops_path"):
        cli.main(train + ["--pops_path", str(tmp_path / "absent.pop")])
    with pytest.raises(SystemExit, match=r"--bootstrap must be >= 2"):
        cli.main(["train"] + common + ["--k", "3", "--bootstrap", "1"])
    with pytest.raises(SystemExit, match=r"--boot_rounds must be >= 1"):
        cli.main(train + ["--boot_rounds", "0"])
    with pytest.raises(SystemExit, match=r"needs a ROCm GPU"):
        cli.main(train)


def test_train_refuses_bootstrap_on_sharded_and_supervised_runs():
    from neural_admixture_amd.train import train
    args = (1, 8, 1e-3, 3, 0, None, torch.device("cpu"))
    with pytest.raises(ValueError, match="bootstrap needs a single-GPU, unsupervised run"):
        train(*args, 2, 8, True, None, None, bootstrap=5)
    with pytest.raises(ValueError, match="bootstrap needs a single-GPU, unsupervised run"):
        train(*args, 1, 8, True, None, ["a", "b"], bootstrap=5)
    with pytest.raises(ValueError, match="bootstrap must be 0 or a number of replicates >= 2"):
        train(*args, 1, 8, True, None, None, bootstrap=1)
    with pytest.raises(ValueError, match="boot_rounds and boot_block must be >= 1"):
        train(*args, 1, 8, True, None, None, bootstrap=5, boot_rounds=0)


def test_sharded_and_cpu_engines_refuse_bootstrap_q():
    from neural_admixture_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.mode, e.world, e._plan, e.xp = "dp", 2, None, None
    with pytest.raises(NotImplementedError, match="Engine.bootstrap_q is single-GPU"):
        e.bootstrap_q()
    e.mode, e.world = "snp", 2
    with pytest.raises(NotImplementedError, match="Engine.bootstrap_q is single-GPU"):
        e.bootstrap_q(B=4)
    e.mode, e.world = "single", 1
    with pytest.raises(RuntimeError, match="Engine.bootstrap_q needs the HIP engine with its packed matrix resident"):
        e.bootstrap_q(B=4, rounds=3)


def test_public_names():
    import neural_admixture_amd as na
    for name in ("bootstrap_q", "block_weights"):
        assert callable(getattr(na, name)) and name in na.__all__


# ------------------------------------------------------------------------------------------------ GPU: one weighted step
@functools.lru_cache(maxsize=None)
def _case(M, K):
    Gm, P, Q = R.make_case(130, M, K, edge=True)
    return Gm, P, Q, _packed(Gm)


def _weights(M):
    """A per-SNP draw with one SNP at the largest weight, zeros over the last partial 16-SNP word and, at M = 1027, over the whole
    second 256-SNP chunk (M = 257: the zero tail IS the second chunk)."""
    w = BO.block_weights(M, 1, 3, 0).astype(np.uint8)
    w[5] = 255
    if M >= 512:
        w[256:512] = 0
    w[M // 16 * 16:] = 0
    assert w.max() == 255 and (w[:256] > 1).any() and (w[:256] == 0).any()
    return w


def _gpu_step(xp, M, idx, P, Q, w=None, loglik=True, inplace=False):
    """One nadm_project_q_w call (w = None: nadm_project_q) -> (Q_out [b, K] numpy, ll [b] or None, nobs [b])."""
    from neural_admixture_amd import project
    from neural_admixture_amd._lib import lib
    dev = xp.device
    b, K = Q.shape
    Pp = project.pad_P(P, dev)
    qin = project.pad_Q(Q, b, K, Pp.shape[1], dev)
    qout = qin if inplace else torch.full_like(qin, 7.0)
    ll = torch.full((b,), 7.0, dtype=torch.float64, device=dev) if loglik else None
    no = torch.full((b,), -7, dtype=torch.int32, device=dev)
    scratch = torch.full((int(lib.nadm_project_scratch_floats(b, M, Pp.shape[1])),), 7.0, dtype=torch.float32, device=dev)
    wd = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.uint8)).to(dev)
    project.em_step(xp, M, None if idx is None else torch.from_numpy(idx).to(dev), b, Pp, K, qin, qout, scratch, R.EPS, R.QMIN, ll, no, weights=wd)
    torch.cuda.synchronize()
    assert not qout[:, K:].any()                             # padded columns stay 0
    return qout[:, :K].cpu().numpy(), None if ll is None else ll.cpu().numpy(), no.cpu().numpy()


ONE_STEP = [(b, M, K) for b in (1, 70, 130) for M in (257, 1027) for K in (2, 3, 8, 9, 16, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("b, M, K", ONE_STEP)
def test_one_weighted_step_against_float64(b, M, K):
    """max |Q_gpu - Q_f64| <= 1e-6 (the project's bound for this kernel; the float32 restatement lands ~3e-8 from float64 on these
    weights), n == sum of w over the observed calls exactly, ll within max(8 e32, 1e-6) relative, e32 = the float32 restatement's own
    relative error (test_project_q's rule).  b = 70 goes through a gather list (the rows in reverse).  Every case prints its figures
    before it asserts.  OBSERVED on an MI355X over the grid (36 cases): max |Q_gpu - Q_f64| 8.9e-9 .. 2.7e-7 (the largest at b = 130,
    M = 257, K = 2); ll relative error 2.4e-9 .. 4.1e-7 against tolerances of 8.2e-5 .. 1.6e-3."""
    dev = _dev()
    Gm, P, Q, xph = _case(M, K)
    w = _weights(M)
    idx = np.arange(b, dtype=np.int32)[::-1].copy() if b == 70 else None
    Gb, Qb = (Gm[:b] if idx is None else Gm[idx]), Q[:b].copy()
    q64, ll64, n64 = BO.em_step_w(Gb, P, Qb, w)
    _, ll32, _ = BO.em_step_w(Gb, P, Qb, w, dtype=np.float32)
    nz = ll64 != 0.0
    e32 = float((np.abs(ll32 - ll64)[nz] / np.abs(ll64[nz])).max()) if nz.any() else 0.0
    tol = max(8.0 * e32, 1e-6)
    q, ll, n = _gpu_step(xph.to(dev), M, idx, P, Qb, w)
    dq = float(np.abs(q - q64).max())
    rel = np.abs(ll - ll64) / np.maximum(np.abs(ll64), 1e-300)
    print(f"b={b} M={M} K={K}: max|Q_gpu - Q_f64| = {dq:.3e}, ll rel err = {float(rel[nz].max()) if nz.any() else 0.0:.3e}, e32 = {e32:.3e}, "
          f"tol = {tol:.3e}")
    assert np.array_equal(n, n64) and np.array_equal(n64, ((Gb != 3) * w[None, :].astype(np.int64)).sum(axis=1))
    assert dq <= 1e-6
    assert np.abs(q.sum(axis=1) - 1.0).max() < 1e-6
    assert (np.abs(ll - ll64) <= tol * np.abs(ll64)).all()
    assert (ll[n64 == 0] == 0.0).all() and np.array_equal(q[n64 == 0], Qb[n64 == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("loglik", [True, False])
@pytest.mark.parametrize("K", [8, 20])
def test_unit_weights_give_the_bits_of_the_unweighted_step(K, loglik):
    dev = _dev()
    M, b = 1027, 130
    Gm, P, Q, xph = _case(M, K)
    xp = xph.to(dev)
    want = _gpu_step(xp, M, None, P, Q[:b], None, loglik)
    got = _gpu_step(xp, M, None, P, Q[:b], np.ones(M, dtype=np.uint8), loglik)
    for a, g in zip(want, got):
        assert (a is None and g is None) or a.tobytes() == g.tobytes()
    assert (want[1] is None) == (not loglik)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 16, 20])
def test_a_zero_weight_snp_contributes_exactly_nothing(K):
    """Other rows of P and other calls (observed ones turned missing and back, other genotypes) at the SNPs of weight 0 -- the whole
    second chunk among them, which the kernel skips: Q, ll and n come out bit-identical."""
    dev = _dev()
    M, b = 1027, 70
    Gm, P, Q, xph = _case(M, K)
    w = _weights(M)
    zero = w == 0
    assert zero[256:512].all() and zero[:256].any() and zero[1024:].all()
    want = _gpu_step(xph.to(dev), M, None, P, Q[:b], w)
    G2, P2 = Gm.copy(), P.copy()
    G2[:, zero] = (Gm[:, zero] + 1 + (np.arange(130)[:, None] % 3)) % 4
    P2[zero] = 1.0 - 0.5 * P[zero][:, ::-1]
    assert (G2[:b] != Gm[:b]).any() and not np.array_equal(P2, P)
    got = _gpu_step(_packed(G2, dirty=True).to(dev), M, None, P2, Q[:b], w)
    for a, g in zip(want, got):
        assert a.tobytes() == g.tobytes()
    w1 = w.copy()
    w1[300] = 1                                              # (with a weight there the step does see those SNPs)
    assert not np.array_equal(_gpu_step(xph.to(dev), M, None, P, Q[:b], w1)[0], want[0])


@pytest.mark.gpu
def test_weight_two_is_the_snp_written_twice():
    """The weighted step with w in {1, 2} against the UNWEIGHTED step on the host-built matrix that holds those SNPs twice: a check
    that does not go through the restatement's reading of the weights.  Not bitwise (another summation order): max |dQ| <= 1e-6."""
    dev = _dev()
    b, M, K = 70, 513, 8
    Gm, P, Q = R.make_case(b, M, K, seed=9)
    w = (1 + (np.random.default_rng(2).random(M) < 0.4)).astype(np.uint8)
    assert set(w.tolist()) == {1, 2}
    twice = np.repeat(np.arange(M), w)
    q, ll, n = _gpu_step(_packed(Gm).to(dev), M, None, P, Q, w)
    qd, lld, nd = _gpu_step(_packed(np.ascontiguousarray(Gm[:, twice])).to(dev), len(twice), None, np.ascontiguousarray(P[twice]), Q, None)
    dq = float(np.abs(q - qd).max())
    print(f"weight 2 against duplication: max |dQ| = {dq:.3e}")
    assert dq <= 1e-6 and np.array_equal(n, nd) and np.allclose(ll, lld, rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 20])
def test_two_launches_agree_bit_for_bit_and_in_place_equals_out_of_place(K):
    dev = _dev()
    M, b = 1027, 130
    Gm, P, Q, xph = _case(M, K)
    xp, w = xph.to(dev), _weights(M)
    first = _gpu_step(xp, M, None, P, Q[:b], w)
    for other in (_gpu_step(xp, M, None, P, Q[:b], w), _gpu_step(xp, M, None, P, Q[:b], w, inplace=True)):
        for a, g in zip(first, other):
            assert a.tobytes() == g.tobytes()


# ------------------------------------------------------------------------------------------------ GPU: the driver
@functools.lru_cache(maxsize=None)
def _driver_case():
    P, Q = BO.planted_truth(seed=7)
    return BO.planted_panel(P, Q, 100), P.astype(np.float32), Q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _driver_want(block, dtype):
    Gm, P, Q = _driver_case()
    return BO.bootstrap_q(Gm, P, Q, 8, block, 10, 5, dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [1, 64])
def test_bootstrap_q_against_the_float64_procedure(block):
    """bootstrap_q at (60, 1536, K = 3), B = 8, rounds = 10, tol = 0: the centre is polish's output bit for bit; se and bias against
    the float64 restatement of the whole procedure within 8 x the float32 restatement's own distance from it, at least 1e-6; every
    fit runs its 10 rounds, so hit_limit is set.  MEASURED on the CPU, float32 restatement against float64: block 1: se 2.1e-08,
    bias 4.5e-08; block 64: se 2.2e-08, bias 4.3e-08, the centre 5.9e-08 (the case prints them): 8 x that stays below the floor, so
    the bound in force is 1e-6, against a mean se of 0.010.  OBSERVED on an MI355X, GPU against float64: block 1: se 6.4e-08, bias
    1.0e-07; block 64: se 7.0e-08, bias 1.4e-07; the centre 2.1e-07."""
    from neural_admixture_amd import bootstrap, project
    dev = _dev()
    Gm, P, Q = _driver_case()
    N, M = Gm.shape
    xp = _packed(Gm).to(dev)
    qc64, se64, bias64 = _driver_want(block, np.float64)
    _, se32, bias32 = _driver_want(block, np.float32)
    d_se, d_bias = float(np.abs(se32 - se64).max()), float(np.abs(bias32 - bias64).max())
    res = bootstrap.bootstrap_q(xp, M, [P], [Q], B=8, block=block, rounds=10, tol=0.0, seed=5)
    assert len(res) == 1
    r = res[0]
    _, Qp, _, _, ran = project.polish(xp, M, [P], [Q], 10, 0.0)
    assert torch.equal(r.q_centre, Qp[0]) and ran == 10 == r.centre_rounds
    se, bias = r.se.cpu().numpy(), r.bias.cpu().numpy()
    g_se, g_bias = float(np.abs(se - se64).max()), float(np.abs(bias - bias64).max())
    print(f"block {block}: float32 restatement - float64: se {d_se:.3e}, bias {d_bias:.3e}; GPU - float64: se {g_se:.3e}, bias {g_bias:.3e}; "
          f"centre {float(np.abs(r.q_centre.cpu().numpy() - qc64).max()):.3e}; mean se {float(se.mean()):.4f}")
    assert r.se.dtype == torch.float64 and se.shape == bias.shape == (N, 3) and r.k == 3
    assert g_se <= max(8.0 * d_se, 1e-6)
    assert g_bias <= max(8.0 * d_bias, 1e-6)
    assert r.rounds_run == [10] * 8 and r.hit_limit and r.n_blocks == -(-M // block)
    assert abs(r.centre_shift - float(np.abs(r.q_centre.cpu().numpy() - Q).max())) < 1e-7
    loose = bootstrap.bootstrap_q(xp, M, [P], [r.q_centre], B=2, block=block, rounds=10, tol=1.0, seed=5)[0]      # tol ends every fit at once
    assert loose.rounds_run == [1, 1] and loose.centre_rounds == 1 and not loose.hit_limit


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_bootstrap_end_to_end_on_the_demo(tmp_path, caplog):
    """Train the demo for a few epochs with --bootstrap 4, then run the `bootstrap` mode with -B 4 on the written files: both write
    {name}.3.Q_se and .Q_bias of shape N x 3, finite, with a standard error > 0 somewhere, and log the line per K and the warning that
    names --boot_rounds (3 rounds at tolerance 0 always end at the limit)."""
    from neural_admixture_amd import cli
    d = np.load(f"{G}/demo_k3.npz")
    N = int(d["N"])
    d["bed_bytes"].tofile(tmp_path / "demo.bed")
    (tmp_path / "demo.fam").write_text("\n".join(["s"] * N) + "\n")
    out = tmp_path / "out"
    caplog.set_level(logging.INFO)
    refit = ["--block", "64", "--boot_rounds", "3", "--boot_tol", "0"]
    assert cli.main(["train", "--epochs", "5", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "--seed", "42", "--batch_size", "800", "--hidden_size", "128", "--bootstrap", "4"] + refit) == 0
    assert cli.main(["bootstrap", "--k", "3", "--name", "demo", "--data_path", str(tmp_path / "demo.bed"), "--save_dir", str(out),
                     "-B", "4", "--out_name", "again"] + refit) == 0
    mats = {}
    for name in ("demo", "again"):
        for ext in ("Q_se", "Q_bias"):
            a = np.loadtxt(out / f"{name}.3.{ext}", ndmin=2)
            assert a.shape == (N, 3) and np.isfinite(a).all()
            mats[name, ext] = a
        assert (mats[name, "Q_se"] >= 0).all() and mats[name, "Q_se"].max() > 0 and np.abs(mats[name, "Q_bias"]).max() > 0
    # the mode reads the .P / .Q that train wrote (18 digits: the same float32) and draws with the same default seed
    assert np.array_equal(mats["demo", "Q_se"], mats["again", "Q_se"]) and np.array_equal(mats["demo", "Q_bias"], mats["again", "Q_bias"])
    msgs = [r.getMessage() for r in caplog.records]
    assert len([m for m in msgs if m.startswith("Bootstrap SE (K=3): mean ")]) == 2
    assert len([m for m in msgs if "--boot_rounds" in m and "limit of 3 rounds" in m]) == 2
    assert any("Bootstrap over SNPs: 4 replicates, blocks of 64" in m for m in msgs) and any("Standard errors and biases of Q saved" in m for m in msgs)
