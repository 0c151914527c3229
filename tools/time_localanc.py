"""Times of the local-ancestry recursion (include/nadm.h: nadm_local_anc; localanc.py) on a resident synthetic matrix, next to
nadm_sample_info (the other lane-per-sample walk over the whole SNP axis) at the same shape in the same run.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; the SNPs as `--chroms` chromosomes (default 22) of equal size and
`--cm` cM each (default 150), evenly spaced; `--generations` 20; output points every `--grid` cM; device events, the legs
alternating; median and quartiles:
  forward    nadm_local_anc with dosage == NULL: the log-likelihood alone (what the scan over the generations calls)
  full       both passes, in row blocks whose checkpoints fit `--budget_gb` (default 16; localanc.block_rows)
  sample_info  qse.q_info on the same rows
    python tools/time_localanc.py [--rounds 3] [--shapes 2504x600000x3,2504x600000x8,100000x500000x8] [--out profiles/localanc.txt]
The library calls alone are timed (forward_backward on operands already on the device), not the copies of the results to the host.
Nothing is gated or promised; the numbers are recorded."""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd import localanc as la, qse  # noqa: E402
from _timing import quart, synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--shapes", default="2504x600000x3,2504x600000x8,100000x500000x8")
ap.add_argument("--chroms", type=int, default=22)
ap.add_argument("--cm", type=float, default=150.0)
ap.add_argument("--generations", type=float, default=20.0)
ap.add_argument("--grid", type=float, default=la.GRID)
ap.add_argument("--budget_gb", type=float, default=16.0)
ap.add_argument("--out", default="profiles/localanc.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_localanc.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)


def leg(b, M, K):
    xp, P, Q, kp, ld = synth(b, M, K)
    per = -(-M // a.chroms)
    chrom = np.minimum(np.arange(M) // per, a.chroms - 1)
    cm = (np.arange(M) - chrom * per) * (a.cm / per)
    rho, ranges = la.switch_prob(cm, chrom, a.generations)
    out_snp, oseg = la.output_points(cm, chrom, a.grid)
    seg, out_snp, oseg = la.check_layout(M, [m0 for m0, _ in ranges] + [M], out_snp, oseg)
    rho_d, seg_d, out_d, oseg_d = (torch.from_numpy(v).to(dev) for v in (rho, seg, out_snp, oseg))
    step = la.block_rows(len(out_snp), K, int(a.budget_gb * (1 << 30)))
    rows = torch.arange(b, dtype=torch.int32, device=dev)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    keep = {}

    def forward():
        keep["ll"] = la.forward_backward(xp, M, P, Q, K, None, b, rho_d, seg_d, None, None, full=False)[3]

    def full():
        nan = 0
        for r0 in range(0, b, step):
            r1 = min(b, r0 + step)
            d, c, p, l_ = la.forward_backward(xp, M, P, Q[r0:r1], K, rows[r0:r1], r1 - r0, rho_d, seg_d, out_d, oseg_d)
            nan = nan + torch.isnan(p).sum()
            del d, c, p
        keep["nan"] = nan

    def sample_info():
        keep["q"] = qse.q_info(xp, M, Pk, Qk)

    legs = {"forward": forward, "full": full, "sample_info": sample_info}
    for f in legs.values():                                   # warm-up: code objects loaded, buffers touched
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            t[k].append(timed(f))
    lines = [f"b = {b} resident rows, M = {M} in {a.chroms} chromosomes of {a.cm:g} cM, K = {K} (kp = {kp}), ld = {ld}; {a.generations:g} "
             f"generations, {len(out_snp)} output points every {a.grid:g} cM; {-(-b // step)} row block(s) of at most {step} rows "
             f"(checkpoints {min(step, b) * len(out_snp) * la.n_pairs(kp) * 4 / 1e9:.2f} GB); device events, {a.rounds} rounds, the legs "
             "alternating; ms per call: median [quartiles]"]
    for k, v in t.items():
        q = quart(v)
        lines.append(f"  {k:<14}{q[1]:12.3f}  [{q[0]:.3f}, {q[2]:.3f}]   {b * M / q[1] / 1e6:9.2f} G genotypes/s")
    lines.append(f"  total log-likelihood {float(keep['ll'].sum()):.6e}; {int(keep['nan'])} NaN points")
    return lines


out = [f"tools/time_localanc.py: {torch.cuda.get_device_name(0)}"]
for shape in a.shapes.split(","):
    out += leg(*(int(x) for x in shape.split("x")))
    torch.cuda.empty_cache()
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
