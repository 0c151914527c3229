"""Semi-supervised training: a population file in which some samples carry no label (ADMIXTURE's ``-`` lines).

An unlabelled sample has class index -1 (NADM_LABEL_NONE).  It takes part in the reconstruction loss like any other sample, stays
out of the supervised term -- ``CrossEntropyLoss(reduction='sum')`` with an ignored target: nothing added to the loss, nothing to
the gradient, no renormalisation -- and out of the class means of the decoder init.  The expected values of a step are COMPOSED
from the oracle's public pieces (``semi_step_grads`` below: ``oracle.supervised_term`` on the labelled rows, zero rows for the
rest); the first CPU tests show that this composition means what torch's own loss means.

Tolerances.  One step against the composed oracle: those of tests/test_gpu_parity.py's test_one_step_against_reference_fixture /
test_production_step_against_reference_fixture for the same fixture (loss 5e-6 relative, Z 5e-6, Q 2e-6, gradients 2e-5 of their
maximum, parameters after a step 5e-6) -- the supervised path those tests gate is the same arithmetic.  Integer sums and the
P init from them: exact equality."""
import ctypes as C
import importlib
import logging
import os

import numpy as np
import pytest
import torch

from oracle import nadm_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
F32 = np.float32
NONE = -1


def mx(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def rel(a, b):
    return mx(a, b) / (float(np.abs(b).max()) + 1e-30)


# ------------------------------------------------------------------------------------------------ the composed oracle
def semi_supervised_term(Q: np.ndarray, labels: np.ndarray):
    """(loss, dQ) of the supervised term with labels in [-1, k): oracle.supervised_term on the labelled rows, zero rows
    inserted for the unlabelled ones."""
    lab = labels >= 0
    dq = np.zeros_like(Q, dtype=F32)
    if not lab.any():
        return 0.0, dq
    loss, dq_lab = O.supervised_term(Q[lab], labels[lab])
    dq[lab] = dq_lab
    return loss, dq


def semi_step_grads(p: O.Params, Gm: np.ndarray, labels: np.ndarray):
    """oracle.step_grads for a single head with labels in [-1, k), composed from the oracle's public pieces in its own order."""
    X = O.decode_x(Gm)
    Z, rinv, Zn, H, Qs = O.encoder_forward(p, X)
    loss, dP, dQ = O.decoder_grads(Qs[0], p.P[0], X)
    ls, dq_sup = semi_supervised_term(Qs[0], labels)
    loss += ls
    dQ = (dQ + dq_sup).astype(F32)
    grads, dZ = O.mlp_backward(p, Z, rinv, Zn, H, Qs, [dQ])
    grads["P0"] = dP
    grads["V"] = (X.T @ dZ).astype(F32)
    return loss, grads, {"Z": Z, "Qs": Qs}


def fixture_with_holes():
    """one_step_supervised.npz (b = 64, M = 509, K = 5, Hd = 64) with a fixed third of the labels taken away."""
    d = np.load(f"{G}/one_step_supervised.npz")
    labels = d["labels"].astype(np.int64).copy()
    labels[np.random.default_rng(64).permutation(len(labels))[: len(labels) // 3]] = NONE
    assert all((labels == k).any() for k in range(int(d["ks"][0])))         # every class keeps a labelled row
    return d, labels


# ------------------------------------------------------------------------------------------------ CPU tests
def test_label_mapping_and_host_init_with_unlabelled_samples():
    from neural_admixture_amd.train import supervised_init
    d, labels = fixture_with_holes()
    Gm, K = d["G"], int(d["ks"][0])
    full = [f"pop{int(c)}" for c in d["labels"]]
    pops = ["-" if y < 0 else a for a, y in zip(full, labels)]
    hole = np.asarray([a == "-" for a in pops])
    assert 0.3 < hole.mean() < 0.36
    y, P = supervised_init(Gm, pops, K, unlabelled=("-",))
    assert y.dtype == np.int64 and np.array_equal(y < 0, hole) and (y[hole] == NONE).all()
    assert np.array_equal(y[~hole], O.labels_from_pops([a for a in pops if a != "-"]))
    assert P.dtype == np.float32 and mx(P, O.supervised_p_init(Gm[~hole], y[~hole], K)) < 1e-6
    y1, P1 = supervised_init(Gm, pops, K, unlabelled="-")                    # one token as a plain string
    assert np.array_equal(y1, y) and np.array_equal(P1, P)
    # the default: every entry is a class name -- today's output, "-" included as a class of its own
    y0, P0 = supervised_init(Gm, full, K)
    y0e, P0e = supervised_init(Gm, full, K, unlabelled=())
    assert np.array_equal(y0, O.labels_from_pops(full)) and np.array_equal(y0, y0e) and np.array_equal(P0, P0e)
    assert mx(P0, O.supervised_p_init(Gm, y0, K)) < 1e-6
    yd, _ = supervised_init(Gm, pops, K + 1)
    assert yd.min() == 0 and np.array_equal(yd == 0, hole)                   # "-" sorts first
    # a class that lost every label is a class that does not exist
    gone = ["-" if a == "pop3" else a for a in pops]
    with pytest.raises(AssertionError):
        supervised_init(Gm, gone, K, unlabelled=("-",))
    with pytest.raises(AssertionError):                                      # ... and so is "everything unlabelled"
        supervised_init(Gm, ["-"] * len(pops), K, unlabelled=("-",))


def test_composed_supervised_term_is_cross_entropy_with_an_ignored_target():
    """semi_supervised_term == 100 * CrossEntropyLoss(reduction='sum', ignore_index=-1)(Q, y) with autograd on the CPU: loss to 1e-6
    relative, gradient (per unit weight, so of probabilities in [0, 1]) to 1e-6 absolute -- fp32 rounding."""
    d, labels = fixture_with_holes()
    rng = np.random.default_rng(3)
    cases = [(d["Q0_0"].astype(F32), labels),
             (O.softmax_rows(rng.standard_normal((300, 7)).astype(F32) * 3), np.where(np.arange(300) < 256, NONE, np.arange(300) % 7)),
             (O.softmax_rows(rng.standard_normal((9, 3)).astype(F32)), np.full(9, NONE))]
    for Q, y in cases:
        loss, dq = semi_supervised_term(Q, y.astype(np.int64))
        q = torch.tensor(Q, dtype=torch.float32, requires_grad=True)
        ce = torch.nn.CrossEntropyLoss(reduction="sum", ignore_index=-1)(q, torch.tensor(y, dtype=torch.int64))
        ce.backward()
        want = O.SUPERVISED_WEIGHT * float(ce.detach())
        assert abs(loss - want) <= 1e-6 * max(abs(want), 1.0), (loss, want)
        assert mx(dq / F32(O.SUPERVISED_WEIGHT), q.grad.numpy()) < 1e-6
        assert not dq[y < 0].any()


REF_NAMES = {"V": "V", "g": "batch_norm_weight", "W1": "common_encoder_0_weight", "b1": "common_encoder_0_bias",
             "Wk0": "multihead_encoder_heads_0_weight", "bk0": "multihead_encoder_heads_0_bias", "P0": "decoders_decoders_0_weight"}


def reference_fixture(case):
    """tests/golden/one_step_semisupervised.npz: three steps of the reference's own _run_step_supervised with the unlabelled samples'
    targets at torch's ignore_index (make_semisupervised_golden.py).  ``case``: "unif" (P0 uniform in [0.02, 0.98], well conditioned)
    or "mean" (P0 = class means of the raw codes over the labelled rows -- values up to 2: most of the reconstruction sits at the
    clamp, single gradient elements divide by the 1e-12 floor, and the gradients of two summation orders agree like one_step_edge's)."""
    d = np.load(f"{G}/one_step_semisupervised.npz")
    _, labels = fixture_with_holes()
    assert np.array_equal(d["labels"], labels)
    p = O.make_params(int(d["seed"]), d["V0"], d[f"{case}_P0"], int(d["Hd"]), [int(k) for k in d["ks"]])
    return d, labels, p, (lambda key: d[f"{case}_{key}"])


@pytest.mark.parametrize("case", ["unif", "mean"])
def test_composed_oracle_against_the_reference_with_ignored_targets(case):
    """The composed oracle is what the reference computes when it ignores a target.  Tolerances: tests/test_oracle_golden.py's
    test_one_step -- the well-conditioned case its plain ones, the class-mean start those of one_step_edge (gradients 3e-3, dP
    included: with P up to 2 one rounding decides on which side of the clamp's bound a reconstruction lands; P after the step 5e-5,
    no other parameter), and of that case the FIRST step only: Adam's first update is lr * sign(gradient), so an
    element whose ill-conditioned gradient changes sign with the summation order starts step 2 from another point 2 * lr away."""
    d, labels, p, ref = reference_fixture(case)
    assert mx(p.W1, ref("init_common_encoder_0_weight")) == 0 and mx(p.Wk[0], ref("init_multihead_encoder_heads_0_weight")) == 0
    if case == "mean":
        from neural_admixture_amd.train import supervised_init
        pops = ["-" if c < 0 else f"pop{c}" for c in labels]
        assert mx(supervised_init(d["G"], pops, len(p.P[0][0]), unlabelled=("-",))[1], ref("P0")) < 1e-6
    edge = case == "mean"
    gtol = 3e-3 if edge else 1e-5
    opt = O.Adam(p, float(d["lr"]))
    for s in range(1 if edge else 3):
        loss, grads, aux = semi_step_grads(p, d["G"], labels)
        assert abs(loss - float(ref(f"loss{s}"))) / float(ref(f"loss{s}")) < 2e-6
        if s == 0:
            assert mx(aux["Z"], ref("Z0")) < 2e-6 and mx(aux["Qs"][0], ref("Q0_0")) < 1e-6
            for k_, n in REF_NAMES.items():
                assert rel(grads[k_], ref(f"grad0_{n}")) < gtol, (k_, rel(grads[k_], ref(f"grad0_{n}")))
        opt.step(p, grads)
        if not edge:
            for k_ in ("V", "W1", "g"):
                assert mx(p.tensors()[k_], ref(f"after{s}_{REF_NAMES[k_]}")) < 2e-6
        assert mx(p.P[0], ref(f"after{s}_decoders_decoders_0_weight")) < (5e-5 if edge else 1e-6)
    # were the unlabelled rows to count, the first loss would be off by about 100 * 21 * log(5)
    full, _, _ = O.step_grads(O.make_params(int(d["seed"]), d["V0"], ref("P0"), int(d["Hd"]), [5]), d["G"], np.where(labels < 0, 0, labels))
    assert abs(full - float(ref("loss0"))) > 1000


def test_cli_unlabelled_token_and_loss_weight_reach_train(monkeypatch):
    import neural_admixture_amd  # noqa: F401
    from neural_admixture_amd import cli
    base = ["--save_dir", "o", "--data_path", "x.bed", "--name", "n", "--k", "3"]
    a = cli.parse_train_args(base)
    assert a.unlabelled == "-" and a.supervised_loss_weight == 100
    b = cli.parse_train_args(base + ["--unlabelled", "NA", "--supervised_loss_weight", "25", "--pops_path", "p.pop"])
    assert b.unlabelled == "NA" and b.supervised_loss_weight == 25.0
    seen = {}

    def fake_train(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return [np.zeros((4, 3), F32)], [np.zeros((2, 3), F32)], object()

    train_mod, io_mod = importlib.import_module("neural_admixture_amd.train"), importlib.import_module("neural_admixture_amd.io")
    monkeypatch.setattr(train_mod, "train", fake_train)
    monkeypatch.setattr(io_mod, "save_model", lambda *a_, **k_: None)
    monkeypatch.setattr(io_mod, "write_outputs", lambda *a_, **k_: None)
    pops = ["a", "NA", "b", "c"]
    cli._train_worker(0, b, 1, None, None, pops, 0.0)
    assert seen["kw"]["supervised_loss_weight"] == 25.0 and tuple(seen["kw"]["unlabelled"]) == ("NA",)
    assert seen["args"][11] is pops
    cli._train_worker(0, a, 1, None, None, None, 0.0)                        # no population file: nothing is unlabelled
    assert seen["kw"]["unlabelled"] is None and seen["kw"]["supervised_loss_weight"] == 100


def test_train_takes_the_new_keywords_only_by_name():
    import inspect
    import neural_admixture_amd as na
    from neural_admixture_amd.train import supervised_init
    params = inspect.signature(na.train).parameters
    assert params["unlabelled"].kind is inspect.Parameter.KEYWORD_ONLY and params["unlabelled"].default is None
    assert params["supervised_loss_weight"].kind is inspect.Parameter.KEYWORD_ONLY and params["supervised_loss_weight"].default == 100.0
    assert list(inspect.signature(supervised_init).parameters) == ["data_np", "pops", "K", "unlabelled", "device"]


# ------------------------------------------------------------------------------------------------ GPU tests
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _sums_case(K, seed=5):
    """N = 700 rows of M = 4099 SNPs (no multiple of 4 or 16; 257 words: two tiles), 2 % missing; about 30 % of the rows unlabelled,
    class 0 with ONE row, class 1 with more than 300, the others sharing the rest."""
    N, M = 700, 4099
    rng = np.random.default_rng(seed)
    Gm = rng.integers(0, 3, size=(N, M), dtype=np.uint8)
    Gm[rng.random((N, M)) < 0.02] = 3
    y = np.full(N, NONE, dtype=np.int64)
    rows = rng.permutation(N)[: int(0.7 * N)]
    y[rows[0]] = 0
    y[rows[1:312]] = 1
    if K > 2:
        y[rows[312:]] = 2 + rng.integers(0, K - 2, size=len(rows) - 312)
    else:
        y[rows[312:]] = 1
    return Gm, y


def _packed(Gm, ld, dirty):
    """Packed rows [N, ld] on the host; ``dirty``: with every bit that holds no SNP set -- the bytes past ceil(M/4) and the unused
    fields of the last byte."""
    from neural_admixture_amd._lib import lib, check, ptr
    N, M = Gm.shape
    out = torch.empty((N, ld), dtype=torch.uint8)
    check(lib.nadm_pack2bit_host(ptr(torch.from_numpy(np.ascontiguousarray(Gm))), ptr(out), N, M, ld), "pack2bit_host")
    if dirty:
        a = out.numpy()
        a[:, (M + 3) // 4:] = 0xFF
        if M % 4:
            a[:, M // 4] |= (0xFF << (2 * (M % 4))) & 0xFF
    return out


def _call_class_sums(xp, ld, y, K, M, sums):
    """One nadm_class_sums call over the rows of xp (device, [len(y), ld]) with host labels y."""
    from neural_admixture_amd._lib import lib, check, ptr
    order = np.argsort(y, kind="stable")
    start = np.searchsorted(y[order], np.arange(K + 1)).astype(np.int64)
    idx = torch.from_numpy(order.astype(np.int32)).to(xp.device)
    check(lib.nadm_class_sums(ptr(xp), ld, len(y), M, ptr(idx), start.ctypes.data_as(C.POINTER(C.c_int64)), K, ptr(sums), None), "class_sums")
    torch.cuda.synchronize()


def _want_sums(Gm, y, K):
    return np.stack([Gm[y == k].astype(np.int64).sum(axis=0) for k in range(K)])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5, 17])
def test_class_sums_equal_numpy_integer_sums(K):
    from neural_admixture_amd.train import class_sums_gpu
    dev = _dev()
    Gm, y = _sums_case(K)
    N, M = Gm.shape
    ld = 1056                                                # ceil(M/4) = 1025: 31 bytes of padding, all of them dirty
    assert (y == 0).sum() == 1 and (y == 1).sum() > 300 and 0.29 < (y < 0).mean() < 0.31
    xp = _packed(Gm, ld, dirty=True).to(dev)
    want = _want_sums(Gm, y, K)
    one = torch.zeros((K, M), dtype=torch.int32, device=dev)
    _call_class_sums(xp, ld, y, K, M, one)
    assert np.array_equal(one.cpu().numpy().astype(np.int64), want)
    two = torch.zeros((K, M), dtype=torch.int32, device=dev)                 # two calls over row halves add up to the one call
    h = N // 2
    _call_class_sums(xp[:h], ld, y[:h], K, M, two)
    assert np.array_equal(two.cpu().numpy().astype(np.int64), _want_sums(Gm[:h], y[:h], K))
    _call_class_sums(xp[h:], ld, y[h:], K, M, two)
    assert torch.equal(one, two)
    none = torch.zeros((K, M), dtype=torch.int32, device=dev)                # no labelled row: a zeroed array stays zero
    _call_class_sums(xp, ld, np.full(N, NONE, dtype=np.int64), K, M, none)
    assert not none.any()
    # the streaming wrapper (host rows packed and sent 256 at a time) adds up to the same
    assert np.array_equal(class_sums_gpu(Gm, y, K, dev, chunk_rows=256).astype(np.int64), want)


@pytest.mark.gpu
def test_class_sums_refuses_what_it_cannot_sum():
    from neural_admixture_amd._lib import lib, ptr
    dev = _dev()
    xp = torch.zeros((4, 16), dtype=torch.uint8, device=dev)
    sums = torch.zeros((2, 50), dtype=torch.int32, device=dev)
    idx = torch.arange(4, dtype=torch.int32, device=dev)

    def call(ld=16, rows=4, M=50, K=2, start=(0, 2, 4)):
        st = (C.c_int64 * len(start))(*start)
        return lib.nadm_class_sums(ptr(xp), ld, rows, M, ptr(idx), st, K, ptr(sums), None)
    assert call() == 0
    assert call(K=0, start=(0,)) != 0 and call(K=65, start=tuple(range(66))) != 0
    assert call(ld=12) != 0 and call(ld=14) != 0                             # ld < ceil(M/4); ld no multiple of 4
    assert call(start=(0, 3, 2)) != 0 and call(start=(0, 3, 6)) != 0         # decreasing; more rows listed than there are
    assert call(rows=1431655765, start=(0, 0, 0)) == 0                       # the largest row count whose sums fit (nothing listed: no launch)
    assert call(rows=1431655766, start=(0, 0, 0)) != 0 and b"32 bits" in lib.nadm_last_error()
    torch.cuda.synchronize()
    assert sums.cpu().numpy().sum() == 0                                     # (all-zero genotypes: the accepted call added nothing)


@pytest.mark.gpu
def test_supervised_init_on_the_device_equals_the_host_path_bit_for_bit():
    from neural_admixture_amd.io import PackedGenotypes
    from neural_admixture_amd.layout import ModelLayout
    from neural_admixture_amd.train import supervised_init
    dev = _dev()
    K = 5
    Gm, y = _sums_case(K)
    N, M = Gm.shape
    pops = ["-" if c < 0 else f"pop{c}" for c in y]
    yh, Ph = supervised_init(Gm, pops, K, unlabelled=("-",))
    assert np.array_equal(yh, y) and Ph.dtype == np.float32
    yd, Pd = supervised_init(Gm, pops, K, unlabelled=("-",), device=dev)                     # uint8 rows, packed and streamed
    assert np.array_equal(yd, yh) and np.array_equal(Pd, Ph) and Pd.dtype == np.float32
    ld = ModelLayout.row_stride(M)
    packed = _packed(Gm, ld, dirty=False)
    for pk in (packed, packed.to(dev)):                                                      # host-resident and GPU-resident matrix
        data = PackedGenotypes(pk, N, M)
        assert np.array_equal(data.unpack_rows(0, N), Gm)
        yp, Pp = supervised_init(data, pops, K, unlabelled=("-",), device=dev)
        assert np.array_equal(yp, yh) and np.array_equal(Pp, Ph)
        yq, Pq = supervised_init(data, pops, K, unlabelled=("-",))                           # the host loop over unpack_rows
        assert np.array_equal(yq, yh) and np.array_equal(Pq, Ph)
    # fully labelled: the device path against today's host output
    full = [f"pop{c % K}" for c in range(N)]
    y0, P0 = supervised_init(Gm, full, K)
    y1, P1 = supervised_init(Gm, full, K, device=dev)
    assert np.array_equal(y0, y1) and np.array_equal(P0, P1)


def _engine_for(Gm, p, labels, K):
    from test_gpu_parity import make_engine
    e = make_engine(Gm, p, Gm.shape[0])
    if labels is not None:
        e.set_labels(labels, K, O.SUPERVISED_WEIGHT)
    return e


def _check_three_steps(Gm, p0, labels, lr, production):
    """Three steps on the engine -- the unfused sequence forward / backward / adam, or the production step train_step -- against
    three steps of the composed oracle: loss of every step, Z, Q and every gradient of the first (unfused sequence: the production
    step leaves no gradients to read), every parameter after each step."""
    from test_gpu_parity import engine_grads, split_small
    K, b = p0.ks[0], Gm.shape[0]
    p = p0.copy()
    e = _engine_for(Gm, p, labels, K)
    idx = torch.arange(b, dtype=torch.int32, device=e.device)
    opt = O.Adam(p, lr)
    for s in range(3):
        loss, grads, aux = semi_step_grads(p, Gm, labels)
        if production:
            e.train_step(idx, b, lr, with_loss=True)
        else:
            e.forward(idx, b)
            e.backward(idx, b, True)
        torch.cuda.synchronize()
        _, last = e.read_loss()
        print(f"step {s}: loss {last!r} oracle {loss!r} rel {abs(last - loss) / loss:.2e}")
        assert abs(last - loss) / loss < 5e-6
        if not production:
            if s == 0:
                L = e.lay
                g = engine_grads(e)
                Q = e.Q.cpu().numpy()[: b * L.SP].reshape(b, L.SP)[:, :K]
                figs = {k_: rel(g[k_], grads[k_]) for k_ in grads}
                print("Z", mx(e.Z.cpu().numpy()[: b * L.CP].reshape(b, L.CP)[:, :L.C], aux["Z"]), "Q", mx(Q, aux["Qs"][0]), "grads", figs)
                assert mx(e.Z.cpu().numpy()[: b * L.CP].reshape(b, L.CP)[:, :L.C], aux["Z"]) < 5e-6
                assert mx(Q, aux["Qs"][0]) < 2e-6
                assert set(figs) == {"V", "g", "W1", "b1", "Wk0", "bk0", "P0"}
                for k_, v in figs.items():
                    assert v < 2e-5, (k_, v)
            e.adam(lr)
            torch.cuda.synchronize()
        opt.step(p, grads)
        sm = split_small(e.lay, e.small.cpu().numpy())
        got = {"V": e.V().cpu().numpy(), "P0": e.P(0).cpu().numpy(), "g": sm["g"], "W1": sm["W1"], "b1": sm["b1"], "Wk0": sm["Wk0"], "bk0": sm["bk0"]}
        figs = {k_: mx(got[k_], v) for k_, v in p.tensors().items()}
        print(f"after step {s}:", figs)
        for k_, v in figs.items():
            assert v < 5e-6, (s, k_, v)


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["unfused", "train_step"])
def test_one_step_with_unlabelled_rows_against_the_composed_oracle(production):
    d, labels = fixture_with_holes()
    p = O.make_params(int(d["seed"]), d["V0"], d["P0"], int(d["Hd"]), [int(k) for k in d["ks"]])
    _check_three_steps(d["G"], p, labels, float(d["lr"]), production)


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["unfused", "train_step"])
@pytest.mark.parametrize("case", ["unif", "mean"])
def test_one_step_with_unlabelled_rows_against_the_reference_fixture(case, production):
    """The engine against the tensors captured from the reference itself (targets of the unlabelled rows at its ignore_index).
    Tolerances: test_gpu_parity's test_one_step_against_reference_fixture / test_production_step_against_reference_fixture -- the
    well-conditioned case their plain ones; the class-mean start those of one_step_edge (gradients 3e-3, P after the step 1e-4, no
    other parameter) for the first step only (see the CPU test above).  dP takes the 3e-3 too: with P up to 2 a reconstruction lands
    on either side of the clamp's bound by one rounding, which switches that element's gradient -- 5e11 at the floor -- on or off."""
    from test_gpu_parity import engine_grads, split_small
    d, labels, p, ref = reference_fixture(case)
    K, b, lr, edge = 5, d["G"].shape[0], float(d["lr"]), case == "mean"
    e = _engine_for(d["G"], p, labels, K)
    idx = torch.arange(b, dtype=torch.int32, device=e.device)
    for s in range(1 if edge else 3):
        if production:
            e.train_step(idx, b, lr, with_loss=True)
        else:
            e.forward(idx, b)
            e.backward(idx, b, True)
        torch.cuda.synchronize()
        _, last = e.read_loss()
        print(f"{case} step {s}: loss {last!r} reference {float(ref(f'loss{s}'))!r}")
        assert abs(last - float(ref(f"loss{s}"))) / float(ref(f"loss{s}")) < 5e-6
        if not production:
            if s == 0:
                L = e.lay
                g = engine_grads(e)
                Q = e.Q.cpu().numpy()[: b * L.SP].reshape(b, L.SP)[:, :K]
                figs = {k_: rel(g[k_], ref(f"grad0_{n}")) for k_, n in REF_NAMES.items()}
                print("Z", mx(e.Z.cpu().numpy()[: b * L.CP].reshape(b, L.CP)[:, :L.C], ref("Z0")), "Q", mx(Q, ref("Q0_0")), "grads", figs)
                assert mx(e.Z.cpu().numpy()[: b * L.CP].reshape(b, L.CP)[:, :L.C], ref("Z0")) < 5e-6 and mx(Q, ref("Q0_0")) < 2e-6
                for k_, v in figs.items():
                    assert v < (3e-3 if edge else 2e-5), (k_, v)
            e.adam(lr)
            torch.cuda.synchronize()
        sm = split_small(e.lay, e.small.cpu().numpy())
        got = {"V": e.V().cpu().numpy(), "g": sm["g"], "W1": sm["W1"], "b1": sm["b1"], "Wk0": sm["Wk0"]}
        figs = {k_: mx(v, ref(f"after{s}_{REF_NAMES[k_]}")) for k_, v in got.items()}
        figs["P0"] = mx(e.P(0).cpu().numpy(), ref(f"after{s}_decoders_decoders_0_weight"))
        print(f"after step {s}:", figs)
        assert figs["P0"] < (1e-4 if edge else 5e-6)
        if not edge:
            for k_, v in figs.items():
                assert v < 5e-6, (s, k_, v)


def _loop_case():
    """b = 300 > 256 rows: the one-block kernel's threads take a second row.  M = 203, K = 5, Hd = 64."""
    N, M, K, Hd = 300, 203, 5, 64
    Gm = O.synth_genotypes(N, M, K, seed=31, missing=0.03)
    rng = np.random.default_rng(31)
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(F32)
    P0 = rng.uniform(0.02, 0.98, size=(K, M)).astype(F32)
    return Gm, O.make_params(31, V0, P0, Hd, [K]), K


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["unfused", "train_step"])
def test_more_than_256_rows_with_the_first_256_unlabelled(production):
    Gm, p, K = _loop_case()
    labels = np.where(np.arange(300) < 256, NONE, np.arange(300) % K).astype(np.int64)
    _check_three_steps(Gm, p, labels, 2e-3, production)


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["unfused", "train_step"])
def test_a_batch_without_any_labelled_row_is_the_unsupervised_step_bit_for_bit(production):
    Gm, p, K = _loop_case()
    b = Gm.shape[0]
    out = []
    for labels in (np.full(b, NONE, dtype=np.int64), None):
        e = _engine_for(Gm, p.copy(), labels, K)
        assert (e.labels is None) == (labels is None)
        idx = torch.arange(b, dtype=torch.int32, device=e.device)
        losses = []
        for _ in range(2):
            if production:
                e.train_step(idx, b, 2e-3, with_loss=True)
            else:
                e.forward(idx, b)
                e.backward(idx, b, True)
                e.adam(2e-3)
            torch.cuda.synchronize()
            losses.append(e.read_loss()[1])
        out.append((losses, e.pflat.cpu().numpy().copy(), e.small.cpu().numpy().copy()))
    assert out[0][0] == out[1][0] and np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.gpu
def test_set_labels_takes_minus_one_and_nothing_below():
    Gm, p, K = _loop_case()
    e = _engine_for(Gm, p, None, K)
    y = np.arange(300) % K
    y[::3] = NONE
    e.set_labels(y, K)                                       # (raises "label out of range" without the feature)
    assert int(e.labels.min()) == NONE and e.labels.dtype == torch.int32
    y[0] = -2
    with pytest.raises(RuntimeError, match="label out of range"):
        e.set_labels(y, K)
    y[0] = K
    with pytest.raises(RuntimeError, match="label out of range"):
        e.set_labels(y, K)


# ------------------------------------------------------------------------------------------------ end to end
def _three_populations(N=240, M=2048, K=3, seed=17):
    """Three well-separated populations: independent allele frequencies in [0.02, 0.48] (mean code below 1: the reader flips nothing),
    80 samples each in shuffled order, 1 % missing calls; 20 samples per population keep their label."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.02, 0.48, size=(K, M))
    z = rng.permutation(np.repeat(np.arange(K), N // K))
    Gm = rng.binomial(2, f[z]).astype(np.uint8)
    Gm[rng.random((N, M)) < 0.01] = 3
    names = np.asarray(["north", "east", "west"])           # sorted: east, north, west
    pops = np.full(N, "-", dtype=object)
    for k in range(K):
        pops[np.flatnonzero(z == k)[:20]] = names[k]
    return Gm, z, names, [str(a) for a in pops]


def _write_bed(tmp_path, Gm):
    N, M = Gm.shape
    inv = np.array([3, 2, 0, 1], dtype=np.uint8)                           # genotype code -> PLINK 2-bit code
    pad = np.zeros((M, (N + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :N] = inv[Gm.T]
    bed = (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)
    (tmp_path / "s.bed").write_bytes(bytes([0x6C, 0x1B, 0x01]) + bed.tobytes())
    (tmp_path / "s.fam").write_text("\n".join(["s"] * N) + "\n")


@pytest.mark.gpu
def test_semi_supervised_run_through_train_and_through_the_cli(tmp_path, caplog):
    """train(..., pops with "-" entries, unlabelled=("-",)) and `train --pops_path` on a .bed + .pop pair: shapes, P in [0, 1], column j
    of Q = the j-th sorted class name, every LABELLED sample's largest Q is its own class, the log reports the counts.  Nothing is
    asserted about the unlabelled samples: neither the project nor the reference has a yardstick for them; their agreement with the
    generating population is printed."""
    import neural_admixture_amd as na
    from neural_admixture_amd import cli
    from neural_admixture_amd.io import read_bed_packed
    from neural_admixture_amd.svd import RSVD
    dev = _dev()
    Gm, z, names, pops = _three_populations()
    N, M = Gm.shape
    K, epochs = 3, 10
    assert Gm.mean() < 1.0 and Gm[Gm != 3].mean() < 1.0
    _write_bed(tmp_path, Gm)
    (tmp_path / "s.pop").write_text("\n".join(pops) + "\n")
    data = read_bed_packed(str(tmp_path / "s.bed"))
    assert np.array_equal(data.unpack_rows(0, N), Gm)
    V = RSVD(data, N, M, 8, 13)
    caplog.set_level(logging.INFO)
    Ps, Qs, _ = na.train(epochs, 64, 2e-3, K, 13, data, dev, 1, 128, True, V, pops, None, None, 8, unlabelled=("-",))
    assert "Labelled samples: 60, unlabelled samples: 180." in caplog.text
    assert Ps[0].shape == (M, K) and Qs[0].shape == (N, K) and np.isfinite(Qs[0]).all()
    assert float(Ps[0].min()) >= 0.0 and float(Ps[0].max()) <= 1.0
    assert mx(Qs[0].sum(axis=1), 1.0) < 1e-5
    order = sorted(names)                                    # column j of Q is the j-th sorted class name
    lab = np.asarray([a != "-" for a in pops])
    want = np.asarray([order.index(a) if a != "-" else -1 for a in pops])
    assert np.array_equal(Qs[0].argmax(axis=1)[lab], want[lab])
    truth = np.asarray([order.index(names[k]) for k in z])
    print(f"unlabelled samples whose largest Q is their generating population: {int((Qs[0].argmax(axis=1) == truth)[~lab].sum())} of {int((~lab).sum())}"
          f" (mean Q of it {float(Qs[0][np.arange(N), truth][~lab].mean()):.3f}); labelled: mean Q of the label {float(Qs[0][np.arange(N), truth][lab].mean()):.3f}")
    # a fully labelled run prints no such line
    caplog.clear()
    full = [str(names[k]) for k in z]
    na.train(2, 64, 2e-3, K, 13, data, dev, 1, 128, True, V, full, None, None, 8)
    assert "nlabelled" not in caplog.text
    # the command line: "-" lines of the .pop file are the unlabelled samples
    caplog.clear()
    out = tmp_path / "out"
    assert cli.main(["train", "--epochs", str(epochs), "--k", str(K), "--name", "semi", "--data_path", str(tmp_path / "s.bed"), "--save_dir", str(out),
                     "--seed", "13", "--batch_size", "64", "--hidden_size", "128", "--pops_path", str(tmp_path / "s.pop")]) == 0
    assert "Labelled samples: 60, unlabelled samples: 180." in caplog.text
    Q = np.loadtxt(out / "semi.3.Q", dtype=np.float32)
    P = np.loadtxt(out / "semi.3.P", dtype=np.float32)
    assert Q.shape == (N, K) and P.shape == (M, K) and P.min() >= 0.0 and P.max() <= 1.0
    assert np.array_equal(Q, Qs[0])                          # (the resident matrix, summed in one call: the same init, the same run)
    # a lower weight reaches the step: another trajectory
    Ps25, Qs25, _ = na.train(2, 64, 2e-3, K, 13, data, dev, 1, 128, True, V, pops, None, None, 8, unlabelled=("-",), supervised_loss_weight=25.0)
    Ps100, Qs100, _ = na.train(2, 64, 2e-3, K, 13, data, dev, 1, 128, True, V, pops, None, None, 8, unlabelled=("-",))
    assert not np.array_equal(Qs25[0], Qs100[0])
