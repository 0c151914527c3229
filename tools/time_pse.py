"""Times of the P standard errors (include/nadm.h: nadm_snp_info; pse.py) on a resident synthetic matrix.

Per shape (default 100000 x 500000 at K = 8, then 2504 x 600000 at K = 7; admixture-model genotypes from nadm_synth_packed, 2 %
missing), device events, `--rounds` rounds, the legs alternating; median and quartiles:
  pse.p_info        the information of every SNP: nadm_snp_info over blocks of 32768 rows, the blocks added in float64
  nadm_snp_hwe      one Hardy-Weinberg call at the same shape -- it shares the SNP-owner sweep and has four running sums per SNP where
                    this pass has K (K + 1) / 2 + 1; the expectation from the instruction counts is 2 to 3 times that pass
  torch fp32        the same sums in plain torch: blocks of 8192 rows x 16384 SNPs, a matmul for pi, elementwise weights and one
                    matmul (w q_a q_b against ones is written as W^T [q_a q_b]) per block (`--torch_rounds`, it is slow)
  pse.se_from_info  the float64 inversion of the M blocks on the device
    python tools/time_pse.py [--rounds 10] [--torch_rounds 2] [--shapes 100000x500000x8,2504x600000x7] [--out profiles/p_se.txt]
"""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd import pse  # noqa: E402
from _timing import synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--torch_rounds", type=int, default=2)
ap.add_argument("--shapes", default="100000x500000x8,2504x600000x7")
ap.add_argument("--out", default="profiles/p_se.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_pse.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)
EPS = 1e-6


def leg(b, M, K):
    xp, P, Q, kp, ld = synth(b, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    U, Hexp = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    nn, Hobs = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    h_scr = torch.empty(int(lib.nadm_snp_hwe_scratch_floats(b, M)), dtype=torch.float32, device=dev)
    ia, ib = torch.triu_indices(K, K, device=dev)
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)
    keep = {}

    def info():
        keep["info"] = pse.p_info(xp, M, Pk, Qk)

    def hwe():
        check(lib.nadm_snp_hwe(ptr(xp), ld, None, b, M, ptr(Q), kp, K, kp, ptr(P), EPS, 0.0, ptr(U), ptr(Hexp), ptr(nn), ptr(Hobs),
                               ptr(h_scr), st), "snp_hwe")

    def plain():
        out = torch.zeros((M, ia.numel()), dtype=torch.float32, device=dev)
        n_ = torch.zeros(M, dtype=torch.int32, device=dev)
        for r0 in range(0, b, 8192):
            r1 = min(b, r0 + 8192)
            qq = Qk[r0:r1, ia] * Qk[r0:r1, ib]
            for j0 in range(0, M, 16384):
                j1 = min(M, j0 + 16384)
                by = xp[r0:r1, j0 // 4:(j1 + 3) // 4]
                code = ((by[:, :, None] >> shifts) & 3).reshape(by.shape[0], -1)[:, :j1 - j0]
                pi = Qk[r0:r1] @ Pk[j0:j1].T
                m = code != 3
                w = m / (torch.clamp(pi, EPS, 1.0 - EPS) * torch.clamp(1.0 - pi, EPS, 1.0 - EPS))
                out[j0:j1] += w.T @ qq
                n_[j0:j1] += m.sum(dim=0, dtype=torch.int32)
        keep["plain"] = (2.0 * out, n_)

    def inverse():
        keep["se"] = pse.se_from_info(keep["info"][0], Pk, keep["info"][1])

    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    info(), hwe(), plain(), inverse()                         # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    I, n = keep["info"]
    It, nt = keep["plain"]
    agree = float(((I - It.double()).abs() / It.double().clamp(min=1e-30))[It > 0].max())
    same_n = bool(torch.equal(n, nt))
    t = {"pse.p_info": [], "nadm_snp_hwe": [], "torch fp32": [], "pse.se_from_info": []}
    for r in range(a.rounds):
        t["pse.p_info"].append(timed(info))
        t["nadm_snp_hwe"].append(timed(hwe))
        t["pse.se_from_info"].append(timed(inverse))
        if r < a.torch_rounds:
            t["torch fp32"].append(timed(plain))
    torch.backends.cuda.matmul.allow_tf32 = prev
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items() if v}
    blocks = -(-b // pse.ROW_BLOCK)
    scr = int(lib.nadm_snp_info_scratch_floats(min(b, pse.ROW_BLOCK), M, kp))
    se = keep["se"].se
    lines = [f"b = {b} resident rows, M = {M}, K = {K} (kp = {kp}), ld = {ld}; device events, {a.rounds} rounds ({len(t['torch fp32'])} of torch), "
             "the legs alternating; ms per call: median [quartiles]"]
    for k, v in q.items():
        rate = "" if k == "pse.se_from_info" else f"   {b * M / v[1] / 1e6:9.1f} G genotypes/s"
        lines.append(f"  {k:<18}{v[1]:10.3f}  [{v[0]:.3f}, {v[2]:.3f}]{rate}")
    lines.append(f"  pse.p_info / nadm_snp_hwe = {q['pse.p_info'][1] / q['nadm_snp_hwe'][1]:.3f}"
                 + (f"; pse.p_info / torch fp32 = {q['pse.p_info'][1] / q['torch fp32'][1]:.4f}" if "torch fp32" in q else "")
                 + f"; {blocks} row block(s) of at most {pse.ROW_BLOCK}, {int(lib.nadm_snp_info_slices(min(b, pse.ROW_BLOCK), M))} sample "
                 f"slice(s) each, partials {scr * 4 / 1e6:.1f} MB; packed matrix {b * ld / 1e9:.2f} GB")
    lines.append(f"  against the torch sums: max |I - I_torch| / I_torch = {agree:.2e}, n {'equal' if same_n else 'DIFFERS'}; "
                 f"median SE {float(se.nanmedian()):.5f}, {int(torch.isnan(se).sum())} of {se.numel()} NaN")
    return lines


out = [f"tools/time_pse.py: {torch.cuda.get_device_name(0)}"]
for shape in a.shapes.split(","):
    out += leg(*(int(x) for x in shape.split("x")))
    torch.cuda.empty_cache()
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
