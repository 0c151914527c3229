"""Times of the residual PCA given Q and P (include/nadm.h: nadm_resid_project, nadm_resid_project_t; residpca.py) on a resident
synthetic matrix.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events for the products (the legs alternating), the wall
clock around the synchronised call for a whole resid_pca(); median and quartiles:
  nadm_resid_project    Y, ss, nobs with 32 columns over all rows (`--products` shape, default 100000 x 500000 at K = 8), over row
                        blocks of 32768
  nadm_resid_project_t  O, nobs_snp from Yin with 32 columns at the same shape
  nadm_obs_project(_t)  the observed-calls pair products of the `pca` mode at the same shape and columns in the same run: the same
                        pass over the matrix without the K multiply-adds of pi, on the matrix pipe
  nadm_snp_info         pse.p_info at the same shape: the sweep of the transposed product with K (K + 1) / 2 sums instead of 32
  residpca.resid_pca    the full default run (10 PCs, 10 extra columns, 10 rounds) at `--full` (default 2504 x 600000 at K = 7);
                        `--full_rounds` rounds after a first one that loads the code objects
    python tools/time_residpca.py [--rounds 5] [--full_rounds 2] [--out profiles/residpca.txt]
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
from neural_admixture_amd import pca, pse, residpca  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--full_rounds", type=int, default=2)
ap.add_argument("--products", default="100000x500000x8")
ap.add_argument("--full", default="2504x600000x7")
ap.add_argument("--columns", type=int, default=32)
ap.add_argument("--out", default="profiles/residpca.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_residpca.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)


def fmt(v):
    q = quart(v)
    return f"{q[1]:10.3f}  [{q[0]:.3f}, {q[2]:.3f}]", q[1]


def products_leg(N, M, K, cols):
    xp, P, Q, kp, ld = synth(N, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    CP = pca.pad_columns(cols)
    W = torch.zeros((M, CP), dtype=torch.float32, device=dev)
    W2 = torch.zeros((M, CP), dtype=torch.float32, device=dev)
    Yin = torch.zeros((N, CP), dtype=torch.float32, device=dev)
    for t in (W, W2, Yin):
        t[:, :cols].normal_()
    bb = min(N, residpca.ROW_BLOCK)
    fs = torch.empty(max(int(lib.nadm_resid_project_scratch_floats(bb, M, CP)), 4), dtype=torch.float32, device=dev)
    ts = torch.empty(max(int(lib.nadm_resid_project_t_scratch_floats(bb, M, kp, CP)), 4), dtype=torch.float32, device=dev)
    ofs = torch.empty(max(int(lib.nadm_obs_project_scratch_floats(N, M, CP)), 4), dtype=torch.float32, device=dev)
    ots = torch.empty(max(int(lib.nadm_obs_project_t_scratch_floats(N, M, CP)), 4), dtype=torch.float32, device=dev)
    keep = {}
    # the products take padded operands as resid_pca hands them over: the padding of P and Q is not part of a call
    legs = {
        "nadm_resid_project": lambda: keep.update(Y=residpca._project(xp, M, K, P, Q, None, N, W, cols, residpca.PIMIN, residpca.EPS, fs)),
        "nadm_resid_project_t": lambda: keep.update(O=residpca._project_t(xp, M, K, P, Q, None, N, Yin, cols, residpca.PIMIN, residpca.EPS, ts)),
        "nadm_obs_project": lambda: keep.update(Yo=pca.obs_project(xp, M, W, W2, cols, None, ofs)),
        "nadm_obs_project_t": lambda: keep.update(Oo=pca.obs_project_t(xp, M, Yin, cols, None, ots)),
        "nadm_snp_info": lambda: keep.update(I=pse.p_info(xp, M, Pk, Qk)),
    }
    for f in legs.values():                                   # warm-up: code objects loaded, buffers touched
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            t[k].append(timed(f))
    lines = [f"N = {N} resident rows, M = {M}, K = {K} (kp = {kp}), {cols} columns (CP = {CP}), ld = {ld}; device events, {a.rounds} rounds, "
             "the legs alternating; ms per call: median [quartiles]"]
    packed_gb = N * ld / 1e9
    for k, v in t.items():
        s, med = fmt(v)
        lines.append(f"  {k:<22}{s}   {N * M / med / 1e6:.1f} G genotypes/s, {packed_gb / med * 1e3:.0f} GB/s of packed matrix")
    blocks = -(-N // residpca.ROW_BLOCK)
    lines.append(f"  split: {blocks} row block(s) of at most {residpca.ROW_BLOCK}; forward {int(lib.nadm_resid_project_ranges(bb, M))} range(s) of "
                 f"{int(lib.nadm_resid_project_chunks(bb, M))} chunk(s), partials {fs.numel() * 4 / 1e6:.1f} MB; transposed "
                 f"{int(lib.nadm_resid_project_t_slices(bb, M))} slice(s), image and partials {ts.numel() * 4 / 1e6:.1f} MB")
    n = keep["Y"][2]
    lines.append(f"  included calls per sample: median {int(n.median())} of {M}")
    return lines


def full_leg(N, M, K):
    xp, P, Q, _, _ = synth(N, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    keep = {}

    def full():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep["r"] = residpca.resid_pca(xp, M, Pk, Qk)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    full()
    s, _ = fmt([full() for _ in range(a.full_rounds)])
    r = keep["r"]
    return [f"N = {N} resident rows, M = {M}, K = {K}; residpca.resid_pca with its defaults (10 PCs, 20 columns, 10 rounds, pimin 0.01); wall "
            f"clock, {a.full_rounds} rounds after one that loads the code; ms per call: median [quartiles]",
            f"  residpca.resid_pca    {s}   M_eff = {r.M_eff}, N_eff = {r.N_eff}, mean variance {r.total / r.N_eff:.4f}, edge {r.edge:.4f}; "
            "eigenvalue / edge " + " ".join(f"{v:.3f}" for v in r.ratio[:6]) + " ..."]


out = [f"tools/time_residpca.py: {torch.cuda.get_device_name(0)}"]
out += products_leg(*(int(x) for x in a.products.split("x")), a.columns)
torch.cuda.empty_cache()
out += full_leg(*(int(x) for x in a.full.split("x")))
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
