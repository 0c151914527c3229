"""Times of the Q standard errors given P (include/nadm.h: nadm_sample_info; qse.py) on a resident synthetic matrix.

Per shape (default 2504 x 600000, then a projected batch of 1024 x 600000, both at K = 8; admixture-model genotypes from
nadm_synth_packed, 2 % missing), device events, `--rounds` rounds, the legs alternating; median and quartiles:
  qse.q_info        the information of every sample: nadm_sample_info over blocks of 32768 rows
  pse.p_info        nadm_snp_info at the same shape in the same run -- the same N M K (K + 1) / 2 multiply-adds with the running sums per
                    SNP instead of per sample
  qse.se_from_info  the float64 inversion of the b blocks on the device (the drop-one form, two calls of nadm_snp_info_se)
    python tools/time_qse.py [--rounds 10] [--shapes 2504x600000x8,1024x600000x8] [--out profiles/q_se.txt]
"""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib  # noqa: E402
from neural_admixture_amd import pse, qse  # noqa: E402
from _timing import synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--shapes", default="2504x600000x8,1024x600000x8")
ap.add_argument("--out", default="profiles/q_se.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_qse.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)


def leg(b, M, K):
    xp, P, Q, kp, ld = synth(b, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    keep = {}

    def q_info():
        keep["q"] = qse.q_info(xp, M, Pk, Qk)

    def p_info():
        keep["p"] = pse.p_info(xp, M, Pk, Qk)

    def inverse():
        keep["se"] = qse.se_from_info(keep["q"][0], Qk, keep["q"][1])

    q_info(), p_info(), inverse()                             # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    t = {"qse.q_info": [], "pse.p_info": [], "qse.se_from_info": []}
    for _ in range(a.rounds):
        t["qse.q_info"].append(timed(q_info))
        t["pse.p_info"].append(timed(p_info))
        t["qse.se_from_info"].append(timed(inverse))
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items()}
    bb = min(b, qse.ROW_BLOCK)
    scr = int(lib.nadm_sample_info_scratch_floats(bb, M, kp))
    se = keep["se"].se
    lines = [f"b = {b} resident rows, M = {M}, K = {K} (kp = {kp}), ld = {ld}; device events, {a.rounds} rounds, the legs alternating; "
             "ms per call: median [quartiles]"]
    for k, v in q.items():
        rate = "" if k == "qse.se_from_info" else f"   {b * M / v[1] / 1e6:9.1f} G genotypes/s"
        lines.append(f"  {k:<18}{v[1]:10.3f}  [{v[0]:.3f}, {v[2]:.3f}]{rate}")
    lines.append(f"  qse.q_info / pse.p_info = {q['qse.q_info'][1] / q['pse.p_info'][1]:.3f}; {-(-b // qse.ROW_BLOCK)} row block(s) of at most "
                 f"{qse.ROW_BLOCK}, {int(lib.nadm_sample_info_ranges(bb, M))} range(s) x {-(-bb // 256)} tile(s), partials {scr * 4 / 1e6:.1f} MB; "
                 f"packed matrix {b * ld / 1e9:.2f} GB")
    lines.append(f"  median SE {float(se.nanmedian()):.5f}, {int(torch.isnan(se).sum())} of {se.numel()} NaN, "
                 f"{int(keep['se'].at_bound.sum())} entries at the bound")
    return lines


out = [f"tools/time_qse.py: {torch.cuda.get_device_name(0)}"]
for shape in a.shapes.split(","):
    out += leg(*(int(x) for x in shape.split("x")))
    torch.cuda.empty_cache()
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
