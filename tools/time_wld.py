"""Times of the weighted-LD sums of admixture dating (include/nadm.h: nadm_wld; admixdate.py) on a resident synthetic matrix, next to
nadm_ld_band at the same rows over the same SNP range in the same run.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events, the kernels alternating; median and quartiles:
  nadm_wld      `--rows` rows (default 2504), the SNPs [0, `--M`) (default 32768) as one chromosome of evenly spaced SNPs, a reach of
                `--W` SNPs (default 2048) spread over `--nbins` bins (default 400), for 1 and for `--C` curves (default 3)
  nadm_ld_band  the same rows and SNPs at its widest window (1024 neighbours, r^2 only)
    python tools/time_wld.py [--rounds 5] [--out profiles/wld.txt]
The library adds a block's pairs in LDS first; a build with -DNADM_WLD_GLOBAL_ATOMICS (tools/build_variant.sh, then NADM_LIB=) times the
plain form, every add in global memory.
Nothing is gated or promised; the numbers are recorded."""
import argparse
import ctypes as C
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd import ld  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", type=int, default=2504)
ap.add_argument("--M", type=int, default=32768)
ap.add_argument("--W", type=int, default=2048)
ap.add_argument("--nbins", type=int, default=400)
ap.add_argument("--C", type=int, default=3)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--out", default="profiles/wld.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_wld.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
xp, P, Q, kp, ldb = functools.partial(synth_model, rng=rng, dev=dev, st=st)(a.rows, a.M, a.K)
per_bin = -(-(a.W + 1) // a.nbins)                              # SNPs per grid cell: a pair W apart lands in the last bins
cell = torch.from_numpy((np.arange(a.M) // per_bin).astype(np.int32)).to(dev)
wt = (P[:, :1] - P[:, 1:a.C + 1]).T.contiguous().to(torch.float64)          # C curves: component 1 against 2 .. C + 1
s = torch.empty((a.C, a.nbins), dtype=torch.int64, device=dev)
n = torch.empty((a.nbins,), dtype=torch.int64, device=dev)
keep = {}


def wld(curves):
    check(lib.nadm_wld(ptr(xp), ldb, None, a.rows, a.M, 0, a.M, a.W, ptr(cell), ptr(wt), curves, a.nbins, 2, ptr(s), ptr(n), st), "wld")


def band():
    keep["r2"] = ld.ld_band(xp, a.M, ld.MAX_WINDOW, 0, a.M)


legs = {"nadm_wld, 1 curve": lambda: wld(1), f"nadm_wld, {a.C} curves": lambda: wld(a.C), "nadm_ld_band, W = 1024": band}
for f in legs.values():                                         # warm-up: code objects loaded, buffers touched
    f()
torch.cuda.synchronize()
t = {k: [] for k in legs}
for _ in range(a.rounds):
    for k, f in legs.items():
        t[k].append(timed(f))
wld(a.C)
torch.cuda.synchronize()
pairs = {k: int(n.sum()) for k in legs}
pairs["nadm_ld_band, W = 1024"] = sum(min(1024, a.M - 1 - j) for j in range(a.M))
lines = [f"tools/time_wld.py; {torch.cuda.get_device_name(0)}",
         f"{a.rows} rows, SNPs [0, {a.M}) (ld = {ldb}), reach W = {a.W} in {a.nbins} bins of {per_bin} SNPs; library: "
         f"{os.environ.get('NADM_LIB') or 'csrc/libnadm.so'}; device events, {a.rounds} rounds, the legs alternating; ms per call: "
         "median [quartiles]"]
for k, v in t.items():
    q = quart(v)
    lines.append(f"  {k:<24}{q[1]:10.3f}  [{q[0]:.3f}, {q[2]:.3f}]   {pairs[k]} pairs, {pairs[k] / q[1] / 1e6:.2f} G pairs/s")
text = "\n".join(lines) + "\n"
print(text, end="")
with open(a.out, "w") as fb:
    fb.write(text)
