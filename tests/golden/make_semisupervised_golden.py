#!/usr/bin/env python3
"""Generate tests/golden/one_step_semisupervised.npz by RUNNING THE REFERENCE on CPU: three steps of its own
``NeuralAdmixture._run_step_supervised`` on a batch in which a third of the samples have no label.

The reference's supervised loss is ``CrossEntropyLoss(reduction='sum')`` (model/neural_admixture.py:293) with torch's default
``ignore_index`` of -100, so a target of -100 is a sample it leaves out of the term; this engine writes such a sample as -1.  Inputs:
the genotypes, V0, labels, seed, Hd and lr of one_step_supervised.npz (b = 64, M = 509, K = 5, Hd = 64), the labels with a fixed third
set to "none" (the choice of tests/test_semi_supervised.py::fixture_with_holes).  Two cases, keys prefixed with the case's name:
  mean_  P0 = the supervised init from the LABELLED rows only, per-class mean of the raw codes (model/train.py:82).  Values up to 2
         saturate most of the reconstruction at the clamp, where single gradient elements divide by the 1e-12 floor: loss, Z and Q
         of the first step are rounding-level pins, gradients agree between two summation orders to ~1e-3 only (like one_step_edge).
  unif_  P0 = one_step_supervised.npz's own (uniform in [0.02, 0.98]): well conditioned, every quantity a rounding-level pin.
Recorded like make_golden.py's one-step cases: initial state, loss of every step, Z / Q / every gradient of the first, every
parameter after each step -- data only.

Like make_golden.py this runs only where the reference is present and imports it from a scratch copy (no Cython build needed
for this case):
    mkdir -p /tmp/refbuild && cp -r <reference>/neural_admixture /tmp/refbuild/
    printf '__version__ = "0.0.0+scratch"\\n__version_tuple__ = (0, 0, 0)\\n' > /tmp/refbuild/neural_admixture/_version.py
    NADM_REF=/tmp/refbuild python3 tests/golden/make_semisupervised_golden.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("NADM_REF", "/tmp/refbuild")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))

from neural_admixture.model.neural_admixture import NeuralAdmixture  # noqa: E402

IGNORE = -100          # torch.nn.CrossEntropyLoss's default ignore_index
NONE = -1              # NADM_LABEL_NONE


def run_case(G, V0, P0, labels, K, Hd, seed, lr):
    b, C = G.shape[0], V0.shape[1]
    out = dict(P0=P0)
    torch.set_float32_matmul_precision("highest")
    torch.manual_seed(seed)
    na = NeuralAdmixture(K, 1, b, lr, torch.device("cpu"), seed, 0, True, None, None, None)
    na.initialize_model(torch.tensor(P0), Hd, C, torch.tensor(V0), [K])
    na.optimizer = na.raw_model.create_custom_adam(device=torch.device("cpu"), lr=lr)
    model = na.raw_model
    state = lambda: {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    flat = lambda prefix, sd: {f"{prefix}{k.replace('.', '_')}": v for k, v in sd.items()}
    out.update(flat("init_", state()))
    Gt = torch.tensor(G)
    yt = torch.tensor(np.where(labels < 0, IGNORE, labels), dtype=torch.int64)
    for s in range(3):
        loss = na._run_step_supervised(Gt, yt)
        loss.backward()
        out[f"loss{s}"] = np.float64(loss.item())
        if s == 0:
            with torch.no_grad():
                (_, probs), X = model(Gt)
                out["Z0"] = (X @ model.V).numpy().copy()
                out["Q0_0"] = probs[0].numpy().copy()
            out.update({f"grad0_{n.replace('.', '_')}": p.grad.detach().numpy().copy() for n, p in model.named_parameters()})
        na.optimizer.step()
        model.restrict_P()
        out.update(flat(f"after{s}_", state()))
    return out


def main():
    d = np.load(os.path.join(OUT, "one_step_supervised.npz"))
    G, V0, K, Hd, seed, lr = d["G"], d["V0"], int(d["ks"][0]), int(d["Hd"]), int(d["seed"]), float(d["lr"])
    b = G.shape[0]
    labels = d["labels"].astype(np.int64).copy()
    labels[np.random.default_rng(64).permutation(b)[: b // 3]] = NONE
    out = dict(G=G, V0=V0, ks=np.asarray([K]), Hd=Hd, seed=seed, lr=lr, labels=labels)
    P_mean = np.vstack([G[labels == k].astype(np.float32).mean(axis=0) for k in range(K)]).astype(np.float32)
    for case, P0 in (("mean", P_mean), ("unif", d["P0"])):
        r = run_case(G, V0, P0, labels, K, Hd, seed, lr)
        out.update({f"{case}_{k}": v for k, v in r.items()})
        print("one_step_semisupervised", case, "losses", [r[f"loss{s}"] for s in range(3)], "labelled", int((labels >= 0).sum()), "of", b)
    np.savez_compressed(os.path.join(OUT, "one_step_semisupervised.npz"), **out)


if __name__ == "__main__":
    main()
