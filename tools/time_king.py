"""Times of KING-robust kinship (include/nadm.h: nadm_king; king.py) on a resident synthetic matrix, each next to nadm_kinship (REAP)
at the same shape in the same run.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events, the two kernels alternating; median and quartiles:
  one block    `--b` x `--b` rows (default 1024 x 1024, drawn out of 4 b resident rows) at `--M` SNPs (default 500000)
  all pairs    king.king_pairs next to relate.kinship_pairs at `--full` (default 2504 x 600000): every block with a <= b
    python tools/time_king.py [--rounds 10] [--out profiles/king.txt]
Nothing is gated or promised; the numbers are recorded."""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib  # noqa: E402
from neural_admixture_amd import king, relate  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--b", type=int, default=1024)
ap.add_argument("--M", type=int, default=500000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--full", default="2504x600000")
ap.add_argument("--out", default="profiles/king.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_king.py measures on the GPU; there is no fallback"
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
    ks, rs = king.king_scratch(b, b, M, dev), relate.kinship_scratch(b, b, M, dev)
    keep = {}

    def hip_king():
        keep["c"] = king.king_block(xp, M, idx, idb, b, b, ks)

    def hip_reap():
        keep["r"] = relate.kinship_block(xp, M, P, K, idx, QA, idb, QB, 0.0, rs)

    hip_king(), hip_reap()                                    # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    t = {"nadm_king": [], "nadm_kinship": []}
    for _ in range(a.rounds):
        t["nadm_king"].append(timed(hip_king))
        t["nadm_kinship"].append(timed(hip_reap))
    lines = [f"one {b} x {b} block, M = {M} ({rows} resident rows, ld = {ld}; nadm_kinship at K = {K}, kp = {kp}); device events, "
             f"{a.rounds} rounds, the two alternating; ms per block: median [quartiles]"]
    med = {}
    for k, v in t.items():
        s, med[k] = fmt(v)
        lines.append(f"  {k:<14}{s}   {b * b * M / med[k] / 1e9:.1f} T pair-SNPs/s")
    n = keep["c"][0]
    lines.append(f"  nadm_king / nadm_kinship = {med['nadm_king'] / med['nadm_kinship']:.3f}; {int(lib.nadm_king_ranges(b, b, M))} range(s), "
                 f"partials {ks.numel() * 4 / 1e6:.1f} MB; n equal to nadm_kinship's: {bool(torch.equal(n, keep['r'][2]))}")
    return lines


def full_leg(N, M, K):
    xp, P, Q, kp, ld = synth(N, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    out = {}

    def all_king():
        out["k"] = king.king_pairs(xp, M)

    def all_reap():
        out["r"] = relate.kinship_pairs(xp, M, Pk, Qk)

    all_king(), all_reap()
    torch.cuda.synchronize()
    t = {"king.king_pairs": [], "relate.kinship_pairs": []}
    for _ in range(max(2, a.rounds // 3)):
        t["king.king_pairs"].append(timed(all_king))
        t["relate.kinship_pairs"].append(timed(all_reap))
    nb = -(-N // king.ROWS)
    lines = [f"all pairs of {N} x {M} ({nb * (nb + 1) // 2} blocks of up to {king.ROWS} x {king.ROWS}; the pair list included); device "
             f"events around the whole call, {len(t['king.king_pairs'])} rounds; ms: median [quartiles]"]
    for k, v in t.items():
        lines.append(f"  {k:<22}{fmt(v)[0]}")
    phi = out["k"][2]
    lines.append(f"  {phi.numel()} pairs at or above {king.MIN_PHI:.4f} among unrelated synthetic samples")
    return lines


lines = [f"tools/time_king.py; {torch.cuda.get_device_name(0)}"]
lines += block_leg(a.b, a.M, a.K)
torch.cuda.empty_cache()
N1, M1 = (int(v) for v in a.full.split("x"))
lines += full_leg(N1, M1, a.K)
text = "\n".join(lines) + "\n"
print(text, end="")
with open(a.out, "w") as fb:
    fb.write(text)
