#!/usr/bin/env python3
"""LD pruning on a resident synthetic matrix (admixture-model genotypes from nadm_synth_packed, 2 % missing; neighbouring SNPs are
independent, so the sweep removes next to nothing: the times are those of the band, the copies and an idle sweep):
  - nadm_snp_counts and nadm_ld_band over every range of --range-snps SNPs, device events, medians over --rounds;
  - the whole ld.prune (counts, band range by range, copies to the host, host sweep), wall clock.
Appends its lines to --out (default profiles/ld_prune.txt).  --band-only N: N plain launches of the first range and nothing else
(what a profiler run wraps)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_admixture_amd import ld  # noqa: E402
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd.layout import ModelLayout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2504)
ap.add_argument("--M", type=int, default=600_000)
ap.add_argument("--window", type=int, default=50)
ap.add_argument("--range-snps", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--band-only", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld_prune.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "time_ld.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
rows, M, K = a.rows, a.M, 8
ldb = ModelLayout.row_stride(M)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
Fq = torch.from_numpy(np.clip(0.5 * rng.beta(0.5, 0.5, size=(K, M)), 0.005, 0.5).astype(np.float32)).to(dev)
Qt = torch.from_numpy(rng.dirichlet(0.2 * np.ones(K), size=rows).astype(np.float32)).to(dev)
xp = torch.zeros((rows, ldb), dtype=torch.uint8, device=dev)
check(lib.nadm_synth_packed(ptr(xp), rows, 0, M, ldb, ptr(Qt), ptr(Fq), K, 0.02, 7, st), "synth_packed")
torch.cuda.synchronize()
ranges = [(m0, min(M, m0 + a.range_snps)) for m0 in range(0, M, a.range_snps)]

if a.band_only:
    for _ in range(a.band_only):
        r2 = ld.ld_band(xp, M, a.window, *ranges[0])
    torch.cuda.synchronize()
    print(f"{a.band_only} launches of nadm_ld_band: {rows} x {M}, window {a.window}, SNPs {ranges[0][0]}..{ranges[0][1]}")
    sys.exit(0)


def timed(fn):
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


ld.ld_band(xp, M, a.window, *ranges[0])
ld.snp_counts(xp, M)
torch.cuda.synchronize()
t_cnt = timed(lambda: ld.snp_counts(xp, M))
t_first = timed(lambda: ld.ld_band(xp, M, a.window, *ranges[0]))
t_all = timed(lambda: [ld.ld_band(xp, M, a.window, m0, m1) for m0, m1 in ranges])
t0 = time.time()
keep, stats = ld.prune(xp, M, a.window, 0.1, range_snps=a.range_snps)
wall = time.time() - t0
packed = rows * ((M + 3) // 4)
lines = [f"## {rows} x {M}, window {a.window} (W = {a.window - 1}), ranges of {a.range_snps} SNPs ({len(ranges)}), medians of {a.rounds} (device events)",
         f"nadm_snp_counts, all SNPs:            {t_cnt:10.3f} ms   ({packed / t_cnt / 1e6:.1f} GB/s of packed bytes)",
         f"nadm_ld_band, first range:            {t_first:10.3f} ms",
         f"nadm_ld_band, all {len(ranges):3d} ranges:         {t_all:10.3f} ms   ({rows * M * (a.window - 1) / t_all / 1e9:.2f} x 10^12 sample-pairs/s; "
         f"packed matrix {packed / 1e9:.3f} GB = the bytes one pass must move: {packed / t_all / 1e6:.1f} GB/s)",
         f"ld.prune, wall clock:                 {wall * 1e3:10.1f} ms   (band + copies {stats['seconds_band'] * 1e3:.1f} ms, host sweep "
         f"{stats['seconds_sweep'] * 1e3:.1f} ms; kept {stats['kept']} of {M})"]
print("\n".join(lines))
with open(a.out, "a") as fb:
    fb.write("\n".join(lines) + "\n\n")
