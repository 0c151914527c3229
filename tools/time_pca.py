"""Times of the standardised PCA (include/nadm.h: nadm_obs_project, nadm_obs_project_t; pca.py) on a resident synthetic matrix.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events for the products (the two legs alternating), the wall
clock around the synchronised call for a whole pca(); median and quartiles:
  nadm_obs_project    Y = (g o) W1 + o W2 with 32 columns over all rows (`--products` shape, default 100000 x 500000)
  nadm_obs_project_t  O1, O2 from Yin with 32 columns at the same shape
  pca.pca             the full default run (10 PCs, 10 extra columns, 10 rounds) at every `--full` shape (default 2504 x 600000 and
                      100000 x 500000); `--full_rounds` rounds after a first one that loads the code objects
    python tools/time_pca.py [--rounds 5] [--full_rounds 2] [--out profiles/pca.txt]
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
from neural_admixture_amd import pca  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--full_rounds", type=int, default=2)
ap.add_argument("--products", default="100000x500000")
ap.add_argument("--full", default="2504x600000,100000x500000")
ap.add_argument("--columns", type=int, default=32)
ap.add_argument("--out", default="profiles/pca.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_pca.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)
K = 6


def fmt(v):
    q = quart(v)
    return f"{q[1]:10.3f}  [{q[0]:.3f}, {q[2]:.3f}]", q[1]


def products_leg(N, M, cols):
    xp, _, _, _, ld = synth(N, M, K)
    CP = pca.pad_columns(cols)
    W1 = torch.zeros((M, CP), dtype=torch.float32, device=dev)
    W2 = torch.zeros((M, CP), dtype=torch.float32, device=dev)
    Yin = torch.zeros((N, CP), dtype=torch.float32, device=dev)
    for t in (W1, W2, Yin):
        t[:, :cols].normal_()
    fs = torch.empty(max(int(lib.nadm_obs_project_scratch_floats(N, M, CP)), 4), dtype=torch.float32, device=dev)
    ts = torch.empty(max(int(lib.nadm_obs_project_t_scratch_floats(N, M, CP)), 4), dtype=torch.float32, device=dev)
    keep = {}

    def fwd():
        keep["Y"] = pca.obs_project(xp, M, W1, W2, cols, None, fs)

    def tr():
        keep["O"] = pca.obs_project_t(xp, M, Yin, cols, None, ts)

    fwd(), tr()                                               # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    t = {"nadm_obs_project": [], "nadm_obs_project_t": []}
    for _ in range(a.rounds):
        t["nadm_obs_project"].append(timed(fwd))
        t["nadm_obs_project_t"].append(timed(tr))
    lines = [f"N = {N} resident rows, M = {M}, {cols} columns (CP = {CP}), ld = {ld}; device events, {a.rounds} rounds, the legs alternating; "
             "ms per call: median [quartiles]"]
    packed_gb = N * ld / 1e9
    for k, v in t.items():
        s, med = fmt(v)
        # 2 operands (g o and o) x 3 pieces x 2 flop per (sample, SNP, column) on the matrix pipe
        lines.append(f"  {k:<20}{s}   {N * M / med / 1e6:.1f} G genotypes/s, {packed_gb / med * 1e3:.0f} GB/s of packed matrix, "
                     f"{12.0 * N * M * CP / med / 1e9:.1f} Tflop/s of bf16 pieces")
    lines.append(f"  split: {int(lib.nadm_obs_project_ranges(N, M))} range(s) of {int(lib.nadm_obs_project_chunks(N, M))} chunk(s), partials "
                 f"{fs.numel() * 4 / 1e6:.1f} MB; {int(lib.nadm_obs_project_t_slices(N, M))} slice(s), partials {ts.numel() * 4 / 1e6:.1f} MB")
    return lines


def full_leg(N, M):
    xp, _, _, _, _ = synth(N, M, K)
    keep = {}

    def full():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep["r"] = pca.pca(xp, M)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    full()
    s, _ = fmt([full() for _ in range(a.full_rounds)])
    r = keep["r"]
    return [f"N = {N} resident rows, M = {M}; pca.pca with its defaults (10 PCs, 20 columns, 10 rounds); wall clock, {a.full_rounds} rounds "
            "after one that loads the code; ms per call: median [quartiles]",
            f"  pca.pca             {s}   M_eff = {r.M_eff}; eigenvalues " + " ".join(f"{v:.3f}" for v in r.eigenvalues[:6]) + " ..."]


out = [f"tools/time_pca.py: {torch.cuda.get_device_name(0)}"]
out += products_leg(*(int(x) for x in a.products.split("x")), a.columns)
for shape in a.full.split(","):
    torch.cuda.empty_cache()
    out += full_leg(*(int(x) for x in shape.split("x")))
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
