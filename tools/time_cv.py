"""Times of the cross-validation kernels (include/nadm.h: nadm_cv_mask, nadm_cv_deviance; cv.py) on a resident synthetic matrix.

Two legs (admixture-model genotypes from nadm_synth_packed, 2 % missing):
  1. b x M (default 100000 x 500000), K = 8: one nadm_cv_mask call (out of place), one nadm_cv_deviance call and, as the
     comparison, one nadm_snp_hwe call at the same shape (it shares the SNP-owner sweep) -- device events, `--rounds` rounds, the
     three alternating; median and quartiles.
  2. N2 x M2 (default 2504 x 600000), K = 7: a full cv.cv_error (5 folds, at most 50 rounds, tol 1e-5) from the model the
     genotypes were drawn from -- wall clock around a synchronised call, with the rounds each fold's refit ran.
    python tools/time_cv.py [--b 100000] [--M 500000] [--K 8] [--rounds 10] [--N2 2504] [--M2 600000] [--K2 7] [--out profiles/cv.txt]
"""
import argparse
import ctypes as C
import functools
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd import cv  # noqa: E402
from _timing import quart, synth_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=100_000)
ap.add_argument("--M", type=int, default=500_000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--N2", type=int, default=2504)
ap.add_argument("--M2", type=int, default=600_000)
ap.add_argument("--K2", type=int, default=7)
ap.add_argument("--out", default="profiles/cv.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_cv.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)
FOLDS, SEED = 5, 42


def kernel_leg():
    b, M, K = a.b, a.M, a.K
    xp, P, Q, kp, ld = synth(b, M, K)
    xo = torch.empty_like(xp)
    dv, nh = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    U, Hexp = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    nn, Hobs = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    c_scr = torch.empty(int(lib.nadm_cv_deviance_scratch_floats(b, M)), dtype=torch.float32, device=dev)
    h_scr = torch.empty(int(lib.nadm_snp_hwe_scratch_floats(b, M)), dtype=torch.float32, device=dev)

    def mask():
        check(lib.nadm_cv_mask(ptr(xp), ld, b, 0, M, SEED, FOLDS, 0, ptr(xo), st), "cv_mask")

    def deviance():
        check(lib.nadm_cv_deviance(ptr(xp), ld, b, 0, M, ptr(Q), kp, K, kp, ptr(P), 1e-6, SEED, FOLDS, 0, ptr(dv), ptr(nh), ptr(c_scr), st),
              "cv_deviance")

    def hwe():
        check(lib.nadm_snp_hwe(ptr(xp), ld, None, b, M, ptr(Q), kp, K, kp, ptr(P), 1e-6, 0.0, ptr(U), ptr(Hexp), ptr(nn), ptr(Hobs),
                               ptr(h_scr), st), "snp_hwe")

    legs = (("nadm_cv_mask", mask), ("nadm_cv_deviance", deviance), ("nadm_snp_hwe", hwe))
    for _, f in legs:                                        # warm-up: code objects loaded, buffers touched
        f()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, f in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    held, obs = int(nh.sum(dtype=torch.int64)), int(nn.sum(dtype=torch.int64))
    lines = [f"tools/time_cv.py: b = {b} resident rows, M = {M}, K = {K} (kp = {kp}), ld = {ld}, {FOLDS} folds; {torch.cuda.get_device_name(0)}",
             f"device events, {a.rounds} rounds, the three alternating; ms per call: median [quartiles]"]
    for name, _ in legs:
        q = quart(t[name])
        moved = (2 if name == "nadm_cv_mask" else 1) * b * ld
        lines.append(f"  {name:<18}{q[1]:9.3f}  [{q[0]:.3f}, {q[2]:.3f}]   {b * M / q[1] / 1e6:8.1f} G genotypes/s   "
                     f"{moved / q[1] / 1e9:.3f} TB/s of packed bytes ({'read + written' if name == 'nadm_cv_mask' else 'read once'})")
    lines.append(f"  nadm_cv_deviance / nadm_snp_hwe = {quart(t['nadm_cv_deviance'])[1] / quart(t['nadm_snp_hwe'])[1]:.3f}; "
                 f"{int(lib.nadm_cv_deviance_slices(b, M))} sample slice(s), partials {c_scr.numel() * 4 / 1e6:.1f} MB; packed matrix "
                 f"{b * ld / 1e9:.2f} GB; fold 0 holds {held} of {obs} observed calls ({held / max(obs, 1):.4f})")
    return lines


def cv_leg():
    N, M, K = a.N2, a.M2, a.K2
    xp, P, Q, kp, ld = synth(N, M, K)
    Ps, Qs = [P[:, :K].clone()], [Q[:, :K].clone()]
    cv.cv_error(xp, M, Ps, Qs, folds=2, rounds=1, tol=0.0, seed=SEED)       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = cv.cv_error(xp, M, Ps, Qs, folds=FOLDS, rounds=50, tol=1e-5, seed=SEED)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return [f"cv.cv_error: N = {N}, M = {M}, K = {K}, {FOLDS} folds, at most 50 rounds, tol 1e-5, from the model the genotypes were drawn from",
            f"  wall clock {dt:.2f} s; rounds per fold {res.rounds_run} (hit_limit {res.hit_limit}); CV error {res.error:.5f} +- {res.se:.5f}, "
            f"{res.n_held} held-out calls; {dt / max(sum(res.rounds_run), 1) * 1e3:.1f} ms per refit round, masks and scoring included"]


out = kernel_leg()
torch.cuda.empty_cache()
out += cv_leg()
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
