"""Times of the bootstrap for Q (include/nadm.h: nadm_project_q_w; bootstrap.py) on a resident synthetic matrix.

Two legs (admixture-model genotypes from nadm_synth_packed, 2 % missing):
  1. b x M (default 1024 x 500000), K = 8: one nadm_project_q call -- the yardstick -- against one nadm_project_q_w call with the
     weights of a per-SNP draw (block 1: a third of the SNPs at weight 0, no chunk empty) and with those of a block-256 draw (a third
     of the 256-SNP chunks empty: the early return) -- device events, `--rounds` rounds, the three alternating; median and quartiles.
  2. N2 x M2 (default 2504 x 600000), K = 7: a full bootstrap.bootstrap_q (B replicates, block 1, at most 50 rounds, tol 1e-5) from
     the model the genotypes were drawn from -- wall clock around a synchronised call, with the rounds the fits ran.
    python tools/time_bootstrap.py [--b 1024] [--M 500000] [--K 8] [--rounds 20] [--N2 2504] [--M2 600000] [--K2 7] [--B 200]
                                   [--out profiles/bootstrap.txt]
"""
import argparse
import ctypes as C
import functools
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib  # noqa: E402
from neural_admixture_amd import bootstrap, project  # noqa: E402
from _timing import quart, synth_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=1024)
ap.add_argument("--M", type=int, default=500_000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--N2", type=int, default=2504)
ap.add_argument("--M2", type=int, default=600_000)
ap.add_argument("--K2", type=int, default=7)
ap.add_argument("--B", type=int, default=200)
ap.add_argument("--out", default="profiles/bootstrap.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_bootstrap.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)
SEED = 42


def kernel_leg():
    b, M, K = a.b, a.M, a.K
    xp, P, Q, kp, ld = synth(b, M, K)
    qout = torch.empty_like(Q)
    scratch = torch.empty(int(lib.nadm_project_scratch_floats(b, M, kp)), dtype=torch.float32, device=dev)
    w1 = torch.from_numpy(bootstrap.block_weights(M, 1, SEED, 0)).to(dev)
    w256 = torch.from_numpy(bootstrap.block_weights(M, 256, SEED, 0)).to(dev)
    legs = (("nadm_project_q", None), ("nadm_project_q_w, block 1", w1), ("nadm_project_q_w, block 256", w256))

    def step(w):
        project.em_step(xp, M, None, b, P, K, Q, qout, scratch, weights=w)

    for _, w in legs:                                        # warm-up: code objects loaded, buffers touched
        step(w)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, w in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(w)
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    lines = [f"tools/time_bootstrap.py: b = {b} resident rows, M = {M}, K = {K} (kp = {kp}), ld = {ld}; {torch.cuda.get_device_name(0)}",
             f"one Q step without loglik (accumulate + fold), device events, {a.rounds} rounds, the three alternating; ms per call: median [quartiles]"]
    base = quart(t["nadm_project_q"])[1]
    for name, w in legs:
        q = quart(t[name])
        zero = "" if w is None else f"   {float((w == 0).float().mean()):.3f} of the SNPs at weight 0"
        lines.append(f"  {name:<30}{q[1]:9.3f}  [{q[0]:.3f}, {q[2]:.3f}]   {b * M / q[1] / 1e6:8.1f} G genotypes/s   x{q[1] / base:.3f} of the unweighted step{zero}")
    return lines


def bootstrap_leg():
    N, M, K = a.N2, a.M2, a.K2
    xp, P, Q, kp, ld = synth(N, M, K)
    Ps, Qs = [P[:, :K].clone()], [Q[:, :K].clone()]
    bootstrap.bootstrap_q(xp, M, Ps, Qs, B=2, block=1, rounds=1, tol=0.0, seed=SEED)       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = bootstrap.bootstrap_q(xp, M, Ps, Qs, B=a.B, block=1, rounds=50, tol=1e-5, seed=SEED)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    total = res.centre_rounds + sum(res.rounds_run)
    return [f"bootstrap.bootstrap_q: N = {N}, M = {M}, K = {K}, B = {a.B}, block 1, at most 50 rounds, tol 1e-5, from the model the genotypes were drawn from",
            f"  wall clock {dt:.2f} s; the centre ran {res.centre_rounds} rounds, the replicates {min(res.rounds_run)} .. {max(res.rounds_run)} "
            f"(hit_limit {res.hit_limit}); mean SE {float(res.se.mean()):.5f}, max SE {float(res.se.max()):.5f}; "
            f"{dt / max(total, 1) * 1e3:.1f} ms per round, the draws, their upload and the log-likelihood passes included"]


out = kernel_leg()
torch.cuda.empty_cache()
out += bootstrap_leg()
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
