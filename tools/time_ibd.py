"""Times of the IBD-sharing sums given ancestry (include/nadm.h: nadm_ibd; relate.py) on a resident synthetic matrix, each next to
nadm_kinship (REAP) at the same shape in the same run.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events, the two kernels alternating; median and quartiles:
  one block    `--b` x `--b` rows (default 1024 x 1024, drawn out of 4 b resident rows) at `--M` SNPs (default 500000), f = uniform(-0.1, 0.1)
  all pairs    relate.ibd_pairs next to relate.kinship_pairs at `--full` (default 2504 x 600000), both with min_phi = 0: the samples
               are unrelated, and at the default threshold no block would hold a listed pair and ibd_pairs would skip them all;
               at 0 about half the pairs are listed and every block is computed
    python tools/time_ibd.py [--rounds 10] [--out profiles/ibd.txt]
Nothing is gated or promised; the numbers are recorded."""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib  # noqa: E402
from neural_admixture_amd import relate  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--b", type=int, default=1024)
ap.add_argument("--M", type=int, default=500000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--full", default="2504x600000")
ap.add_argument("--out", default="profiles/ibd.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_ibd.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)


def fmt(v):
    q = quart(v)
    return f"{q[1]:10.3f}  [{q[0]:.3f}, {q[2]:.3f}]", q[1]


def block_leg(b, M, K):
    rows = 4 * b
    xp, P, Q, kp, ld = synth(rows, M, K)
    idx = torch.from_numpy(rng.permutation(rows)[:b].astype(np.int32)).to(dev)
    idb = torch.from_numpy(rng.permutation(rows)[:b].astype(np.int32)).to(dev)
    QA, QB = Q[idx.long()].contiguous(), Q[idb.long()].contiguous()
    fA, fB = (torch.from_numpy(rng.uniform(-0.1, 0.1, size=b).astype(np.float32)).to(dev) for _ in range(2))
    xs, rs = relate.ibd_scratch(b, b, M, dev), relate.kinship_scratch(b, b, M, dev)
    keep = {}

    def hip_ibd():
        keep["i"] = relate.ibd_block(xp, M, P, K, idx, QA, fA, idb, QB, fB, 0.0, xs)

    def hip_reap():
        keep["r"] = relate.kinship_block(xp, M, P, K, idx, QA, idb, QB, 0.0, rs)

    hip_ibd(), hip_reap()                                     # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    t = {"nadm_ibd": [], "nadm_kinship": []}
    for _ in range(a.rounds):
        t["nadm_ibd"].append(timed(hip_ibd))
        t["nadm_kinship"].append(timed(hip_reap))
    lines = [f"one {b} x {b} block, M = {M} ({rows} resident rows, ld = {ld}; K = {K}, kp = {kp}); device events, "
             f"{a.rounds} rounds, the two alternating; ms per block: median [quartiles]"]
    med = {}
    for k, v in t.items():
        s, med[k] = fmt(v)
        lines.append(f"  {k:<14}{s}   {b * b * M / med[k] / 1e9:.1f} T pair-SNPs/s")
    k2num, k2den, exp0, ibs0 = keep["i"]
    lines.append(f"  nadm_ibd / nadm_kinship = {med['nadm_ibd'] / med['nadm_kinship']:.3f}; {int(lib.nadm_ibd_ranges(b, b, M))} range(s), "
                 f"partials {xs.numel() * 4 / 1e6:.1f} MB; median k2 of the unrelated pairs {float((k2num / k2den).median()):.2e}, "
                 f"median ibs0 / exp0 {float((ibs0.double() / exp0).median()):.4f}")
    return lines


def full_leg(N, M, K):
    xp, P, Q, kp, ld = synth(N, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    out = {}

    def all_ibd():
        out["i"] = relate.ibd_pairs(xp, M, Pk, Qk, min_phi=0.0)

    def all_reap():
        out["r"] = relate.kinship_pairs(xp, M, Pk, Qk, min_phi=0.0)

    all_ibd(), all_reap()
    torch.cuda.synchronize()
    t = {"relate.ibd_pairs": [], "relate.kinship_pairs": []}
    for _ in range(max(2, a.rounds // 3)):
        t["relate.ibd_pairs"].append(timed(all_ibd))
        t["relate.kinship_pairs"].append(timed(all_reap))
    nb = -(-N // relate.ROWS)
    lines = [f"all pairs of {N} x {M}, min_phi = 0 ({nb * (nb + 1) // 2} blocks of up to {relate.ROWS} x {relate.ROWS}; ibd_pairs runs "
             f"kinship_pairs first, then nadm_ibd on every block with a listed pair; the pair list and the gathers included); device "
             f"events around the whole call, {len(t['relate.ibd_pairs'])} rounds; ms: median [quartiles]"]
    med = {}
    for k, v in t.items():
        s, med[k] = fmt(v)
        lines.append(f"  {k:<22}{s}")
    k0 = out["i"][5]
    lines.append(f"  relate.ibd_pairs / relate.kinship_pairs = {med['relate.ibd_pairs'] / med['relate.kinship_pairs']:.3f}; {k0.numel()} pairs "
                 f"listed among unrelated synthetic samples, median k0 {float(k0.nanmedian()):.4f}")
    return lines


lines = [f"tools/time_ibd.py; {torch.cuda.get_device_name(0)}"]
lines += block_leg(a.b, a.M, a.K)
torch.cuda.empty_cache()
N1, M1 = (int(v) for v in a.full.split("x"))
lines += full_leg(N1, M1, a.K)
text = "\n".join(lines) + "\n"
print(text, end="")
with open(a.out, "w") as fb:
    fb.write(text)
