"""Times of the model-fit check (include/nadm.h: nadm_em_sums, nadm_resid_cor; fitcheck.py) on a resident synthetic matrix.

Admixture-model genotypes from nadm_synth_packed, 2 % missing; device events, the legs alternating; median and quartiles:
  nadm_em_sums      the EM sums B and C over all rows (`--sums` shape, default 2504 x 500000 at K = 8), beside nadm_project_p, whose
                    accumulation it shares
  nadm_resid_cor    ONE block of `--block` x `--block` ordered pairs (default 1024) at the same shape
  torch fp32        the same block in plain torch: a loop over the left-out samples b with [ba, M] temporaries (the refit of b's
                    frequencies, a matmul for pi, the residuals, four reductions).  Only `--torch_cols` columns are run and the time
                    is scaled to the block's: a whole 1024-column block takes several seconds per round
  fitcheck.resid_cor  the full statistic (`--full` shape, default 2504 x 600000 at K = 7): the sums once, every ordered block of 1024
                    rows, the symmetrisation; `--full_rounds` rounds after the block leg has loaded the code objects
    python tools/time_fitcheck.py [--rounds 5] [--torch_cols 8] [--full_rounds 2] [--out profiles/fitcheck.txt]
"""
import argparse
import ctypes as C
import functools
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd import fitcheck  # noqa: E402
from _timing import synth_model, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--torch_cols", type=int, default=8)
ap.add_argument("--full_rounds", type=int, default=2)
ap.add_argument("--sums", default="2504x500000x8")
ap.add_argument("--block", type=int, default=1024)
ap.add_argument("--full", default="2504x600000x7")
ap.add_argument("--out", default="profiles/fitcheck.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_fitcheck.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
synth = functools.partial(synth_model, rng=rng, dev=dev, st=st)
EPS = 1e-6


def quart(v):
    q = np.percentile(v, [25, 50, 75])
    return f"{q[1]:10.3f}  [{q[0]:.3f}, {q[2]:.3f}]", q[1]


def decode(xp, rows, M):
    """codes uint8 [len(rows), M] of the packed rows."""
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)
    by = xp[rows, :(M + 3) // 4]
    return ((by[:, :, None] >> shifts) & 3).reshape(by.shape[0], -1)[:, :M]


def block_leg(N, M, K, blk):
    xp, P, Q, kp, ld = synth(N, M, K)
    Pk = P[:, :K].contiguous()
    keep = {}
    p_scr = torch.empty(int(lib.nadm_project_p_scratch_floats(N, M, kp)), dtype=torch.float32, device=dev)
    Pout = torch.empty_like(P)

    def sums():
        keep["BC"] = fitcheck._em_sums_padded(xp, M, K, P, Q, None, N, EPS)

    def pstep():
        check(lib.nadm_project_p(ptr(xp), ld, None, N, M, ptr(Q), kp, K, kp, ptr(P), ptr(Pout), EPS, 1e-6, None, ptr(p_scr), st), "project_p")

    sums()
    B, Cc = keep["BC"]
    ia = torch.arange(0, blk, dtype=torch.int32, device=dev)
    ib = torch.arange(N - blk, N, dtype=torch.int32, device=dev)       # another set of rows, overlapping the first when 2 blk > N
    QA, QB = Q[ia.long()].contiguous(), Q[ib.long()].contiguous()
    scr = fitcheck.resid_cor_scratch(blk, blk, M, kp, dev)

    def block():
        keep["blk"] = fitcheck.resid_cor_block(xp, M, P, K, ia, QA, ib, QB, B, Cc, EPS, scr)

    cols = min(a.torch_cols, blk)
    gA = decode(xp, ia.long(), M)
    oA = (gA != 3).to(torch.float32)
    gA = gA.to(torch.float32) * oA
    Bk, Ck = B[:, :K], Cc[:, :K]
    den = Pk * Bk + (1.0 - Pk) * Ck

    def plain():
        S, Ta, Tb, nn = (torch.empty((blk, cols), dtype=torch.float32, device=dev) for _ in range(4))
        for c in range(cols):
            gb = decode(xp, ib[c:c + 1].long(), M)[0]
            ob = (gb != 3).to(torch.float32)
            gb = gb.to(torch.float32) * ob
            qb = QB[c, :K]
            rr = Pk @ qb
            t1 = gb / torch.clamp(rr, EPS, 1.0 - EPS)
            t0 = ob * (2.0 - gb) / torch.clamp(1.0 - rr, EPS, 1.0 - EPS)
            numn = Pk * torch.clamp(Bk - t1[:, None] * qb, min=0.0)
            denn = numn + (1.0 - Pk) * torch.clamp(Ck - t0[:, None] * qb, min=0.0)
            take = (denn >= 0.125 * den) & (den > 0) & (denn > 0)
            f = torch.where(take, numn / torch.where(take, denn, torch.ones_like(denn)), Pk)
            dA = oA * (gA - 2.0 * (QA[:, :K] @ f.T))             # [ba, M]
            db = ob * (gb - 2.0 * (f @ qb))
            S[:, c] = dA @ db
            Ta[:, c] = (dA * dA) @ ob
            Tb[:, c] = oA @ (db * db)
            nn[:, c] = oA @ ob
        keep["plain"] = (S, Ta, Tb, nn)

    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    pstep(), block(), plain()                                  # warm-up: code objects loaded, buffers touched
    torch.cuda.synchronize()
    S, Ta, Tb, nn = keep["blk"]
    St, Tat, Tbt, nt = keep["plain"]
    c_dev = (S / torch.sqrt(Ta * Tb))[:, :cols]
    c_tor = (St / torch.sqrt(Tat * Tbt)).double()
    ok = torch.isfinite(c_dev) & torch.isfinite(c_tor)
    agree = float((c_dev - c_tor)[ok].abs().max())
    same_n = bool(torch.equal(nn[:, :cols], nt.to(torch.int32)))
    t = {"nadm_em_sums": [], "nadm_project_p": [], "nadm_resid_cor": [], "torch fp32": []}
    for r in range(a.rounds):
        t["nadm_em_sums"].append(timed(sums))
        t["nadm_project_p"].append(timed(pstep))
        t["nadm_resid_cor"].append(timed(block))
        if r < 2:
            t["torch fp32"].append(timed(plain) * blk / cols)
    torch.backends.cuda.matmul.allow_tf32 = prev
    lines = [f"N = {N} resident rows, M = {M}, K = {K} (kp = {kp}), ld = {ld}; device events, {a.rounds} rounds (2 of torch), the legs "
             "alternating; ms per call: median [quartiles]"]
    med = {}
    for k, v in t.items():
        s, med[k] = quart(v)
        note = f"   ({cols} of {blk} columns run, scaled)" if k == "torch fp32" else ""
        lines.append(f"  {k:<18}{s}{note}")
    triples = blk * blk * M
    lines.append(f"  one {blk} x {blk} block: {triples / med['nadm_resid_cor'] / 1e6:.1f} G (a, b, SNP) triples/s; nadm_resid_cor / torch fp32 = "
                 f"{med['nadm_resid_cor'] / med['torch fp32']:.4f}; {int(lib.nadm_resid_cor_ranges(blk, blk, M, kp))} range(s), partials "
                 f"{scr.numel() * 4 / 1e6:.1f} MB; nadm_em_sums / nadm_project_p = {med['nadm_em_sums'] / med['nadm_project_p']:.3f}")
    lines.append(f"  against the torch block: max |c - c_torch| = {agree:.2e} over {cols} columns, n {'equal' if same_n else 'DIFFERS'}")
    return lines


def full_leg(N, M, K):
    xp, P, Q, kp, ld = synth(N, M, K)
    Pk, Qk = P[:, :K].contiguous(), Q[:, :K].contiguous()
    keep = {}

    def full():
        keep["r"] = fitcheck.resid_cor(xp, M, Pk, Qk)

    t = [timed(full) for _ in range(a.full_rounds)]
    cor, n = keep["r"]
    iu = torch.triu_indices(N, N, 1, device=dev)
    v = cor[iu[0], iu[1]]
    s, med = quart(t)
    blocks = (-(-N // fitcheck.ROWS)) ** 2
    return [f"N = {N} resident rows, M = {M}, K = {K} (kp = {kp}); {a.full_rounds} rounds; ms per call: median [quartiles]",
            f"  fitcheck.resid_cor{s}   {N * N * M / med / 1e6:.1f} G (a, b, SNP) triples/s; {blocks} ordered blocks of at most "
            f"{fitcheck.ROWS} rows a side",
            f"  the matrix: mean {float(v.nanmean()):+.5f}, sd {float(v[~torch.isnan(v)].std()):.5f} over {int((~torch.isnan(v)).sum())} pairs "
            f"(P and Q are the truth the genotypes were drawn from, not a fit); 1 / sqrt(median n) = {1.0 / float(n[iu[0], iu[1]].double().median()) ** 0.5:.5f}"]


out = [f"tools/time_fitcheck.py: {torch.cuda.get_device_name(0)}"]
out += block_leg(*(int(x) for x in a.sums.split("x")), a.block)
torch.cuda.empty_cache()
out += full_leg(*(int(x) for x in a.full.split("x")))
print("\n".join(out))
with open(a.out, "w") as fb:
    fb.write("\n".join(out) + "\n")
