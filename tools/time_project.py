"""Time one projection step (nadm_project_q, include/nadm.h) and its counterpart for P (nadm_project_p) next to pass 2 at the same shape.
    python tools/time_project.py [--b 800] [--M 500000] [--K 8] [--rounds 30] [--out profiles/project_p.txt]

Four launch groups on the same resident matrix (admixture-model genotypes from nadm_synth_packed, 2 % missing, the batch = b random
rows of 4 b resident ones), the same P and Q:
    project        nadm_project_q, loglik == NULL (an iteration of the refinement: accumulate + fold)
    project+ll     nadm_project_q with loglik (the logarithms; the first and the last pass of a refinement)
    project_p      nadm_project_p (the P step of a polish round: accumulate + fold)
    pass2          nadm_decode_bce, with_loss = 1, no Adam: the same two products Q.P^T and dR.P plus dP, the yardstick
Each is warmed up, then timed with device events over `rounds` rounds in which the four alternate (what shares the box shifts all
four alike); a timed window is 10 back-to-back calls.  Reported: the median per call and the quartiles, and the ratios to pass 2.

    python tools/time_project.py --kinship [--b 1024] [--M 500000] [--K 8] [--rounds 10] [--out profiles/kinship.txt]
The kinship leg (nadm_kinship, relate.py): one b x b block of sample pairs at M SNPs next to a plain torch formulation of the same block
on the same GPU (per slab of 16384 SNPs: unpack, pi = Q.P^T, the mask, d and s in fp32, then D.D^T, S.S^T and m.m^T as fp32 matmuls --
in this tool only), and the whole pair list of the configs[1] shape (2504 x 600k) through relate.kinship_pairs.

    python tools/time_project.py --hwe [--b 100000] [--M 500000] [--K 8] [--rounds 10] [--out profiles/snp_hwe.txt]
The Hardy-Weinberg leg (nadm_snp_hwe, hwe.py): the four per-SNP sums over b resident rows (all of them, in a permuted order) next to
a plain torch fp32 formulation of the same sums on the same GPU (per block of 8192 rows x 16384 SNPs: unpack, pi = Q.P^T, the mask, the
clips, t and 2 pi (1 - pi) elementwise, column sums -- in this tool only)."""
import argparse
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd.layout import ModelLayout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=None, help="rows of the batch / of a block side (default 800; 1024 with --kinship)")
ap.add_argument("--M", type=int, default=500_000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--kinship", action="store_true", help="the kinship leg instead of the projection groups")
ap.add_argument("--hwe", action="store_true", help="the Hardy-Weinberg leg instead of the projection groups")
a = ap.parse_args()
if a.out is None:
    a.out = "profiles/kinship.txt" if a.kinship else ("profiles/snp_hwe.txt" if a.hwe else "profiles/project_p.txt")
if a.b is None:
    a.b = 1024 if a.kinship else (100_000 if a.hwe else 800)
if a.hwe and a.rounds == 30:
    a.rounds = 10
assert torch.cuda.is_available(), "time_project.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
b, M, K = a.b, a.M, a.K
kp, ld, rows = int(lib.nadm_pad_k(K)), ModelLayout.row_stride(M), (b if a.hwe else 4 * b)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
Fq = torch.from_numpy(np.clip(0.5 * rng.beta(0.5, 0.5, size=(K, M)), 0.005, 0.5).astype(np.float32)).to(dev)
Qt = torch.from_numpy(rng.dirichlet(0.2 * np.ones(K), size=rows).astype(np.float32)).to(dev)
xp = torch.zeros((rows, ld), dtype=torch.uint8, device=dev)
check(lib.nadm_synth_packed(ptr(xp), rows, 0, M, ld, ptr(Qt), ptr(Fq), K, 0.02, 7, st), "synth_packed")
idx = torch.from_numpy(rng.permutation(rows)[:b].astype(np.int32)).to(dev)
P = torch.zeros((M, kp), dtype=torch.float32, device=dev)
P[:, :K] = Fq.T
Q = torch.zeros((b, kp), dtype=torch.float32, device=dev)
Q[:, :K] = torch.from_numpy(rng.dirichlet(np.ones(K), size=b).astype(np.float32)).to(dev)


def kinship_leg():
    from neural_admixture_amd import relate
    num = torch.empty((b, b), dtype=torch.float64, device=dev)
    den, nn = torch.empty_like(num), torch.empty((b, b), dtype=torch.int32, device=dev)
    k_scratch = relate.kinship_scratch(b, b, M, dev)
    idb = torch.from_numpy(rng.permutation(rows)[:b].astype(np.int32)).to(dev)

    def hip():
        check(lib.nadm_kinship(ptr(xp), ld, ptr(idx), b, ptr(idb), b, M, ptr(P), K, kp, ptr(Q), ptr(Q), kp, 0.0, ptr(num), ptr(den), ptr(nn),
                               ptr(k_scratch), st), "kinship")

    slab = 16384
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)

    def side(rows_idx, j0, j1):
        by = xp[rows_idx.long(), j0 // 4:(j1 + 3) // 4]
        code = ((by[:, :, None] >> shifts) & 3).reshape(by.shape[0], -1)[:, :j1 - j0]
        pi = Q[:, :K] @ P[j0:j1, :K].T
        m = (code != 3).to(torch.float32)
        return m * (code.to(torch.float32) - 2.0 * pi), m * torch.sqrt(torch.clamp(pi * (1.0 - pi), min=0.0)), m

    def plain():
        n_ = torch.zeros((b, b), dtype=torch.float32, device=dev)
        d_, s_ = torch.zeros_like(n_), torch.zeros_like(n_)
        for j0 in range(0, M, slab):
            j1 = min(M, j0 + slab)
            da, sa, ma = side(idx, j0, j1)
            db, sb, mb = side(idb, j0, j1)
            d_ += da @ db.T
            s_ += sa @ sb.T
            n_ += ma @ mb.T
        return d_, s_, n_

    for _ in range(2):
        hip()
        want = plain()
    torch.cuda.synchronize()
    agree = float(((num - want[0].double()).abs() / want[1].double()).max())
    t = {"nadm_kinship": [], "torch fp32": []}
    for _ in range(a.rounds):
        for name, f in (("nadm_kinship", hip), ("torch fp32", plain)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    q = {n: np.percentile(v, [25, 50, 75]) for n, v in t.items()}
    macs = float(b) * b * M
    lines = [f"tools/time_project.py --kinship: one {b} x {b} block, M = {M}, K = {K} (kp = {kp}), {rows} resident rows; {torch.cuda.get_device_name(0)}",
             f"device events, {a.rounds} rounds, the two alternating; ms per block: median [quartiles]"]
    for n in t:
        lines.append(f"  {n:13s} {q[n][1]:9.3f}  [{q[n][0]:.3f}, {q[n][2]:.3f}]   {macs / q[n][1] / 1e9:.1f} T pair-SNPs/s")
    lines.append(f"  nadm_kinship / torch fp32 = {q['nadm_kinship'][1] / q['torch fp32'][1]:.3f}; {int(lib.nadm_kinship_ranges(b, b, M))} ranges; "
                 f"max |num - num_torch| / den = {agree:.2e}")
    # the whole pair list of the configs[1] shape
    N1, M1 = 2504, 600_000
    ld1 = ModelLayout.row_stride(M1)
    F1 = torch.from_numpy(np.clip(0.5 * rng.beta(0.5, 0.5, size=(K, M1)), 0.005, 0.5).astype(np.float32)).to(dev)
    Q1 = torch.from_numpy(rng.dirichlet(0.2 * np.ones(K), size=N1).astype(np.float32)).to(dev)
    x1 = torch.zeros((N1, ld1), dtype=torch.uint8, device=dev)
    check(lib.nadm_synth_packed(ptr(x1), N1, 0, M1, ld1, ptr(Q1), ptr(F1), K, 0.02, 7, st), "synth_packed")
    relate.kinship_pairs(x1, M1, F1.T, Q1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    i_, j_, p_, n_, f_ = relate.kinship_pairs(x1, M1, F1.T, Q1)
    e1.record()
    e1.synchronize()
    lines.append(f"  relate.kinship_pairs at {N1} x {M1}, K = {K} (6 blocks of up to 1024 x 1024): {e0.elapsed_time(e1):.1f} ms, "
                 f"{i_.numel()} pairs at or above {relate.MIN_PHI:.4f} among unrelated synthetic samples, max |f| = {float(f_.abs().max()):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fb:
        fb.write(text)


def hwe_leg():
    eps, pimin = 1e-6, 0.0
    U, Hexp = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    nn, Hobs = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    h_scratch = torch.empty(int(lib.nadm_snp_hwe_scratch_floats(b, M)), dtype=torch.float32, device=dev)

    def hip():
        check(lib.nadm_snp_hwe(ptr(xp), ld, ptr(idx), b, M, ptr(Q), kp, K, kp, ptr(P), eps, pimin, ptr(U), ptr(Hexp), ptr(nn), ptr(Hobs),
                               ptr(h_scratch), st), "snp_hwe")

    rblock, slab = 8192, 16384
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)
    rows_l = idx.long()

    def plain(with_abs=False):
        U_, H_ = torch.zeros(M, dtype=torch.float32, device=dev), torch.zeros(M, dtype=torch.float32, device=dev)
        n_, o_ = torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
        T_ = torch.zeros(M, dtype=torch.float32, device=dev)
        for r0 in range(0, b, rblock):
            r1 = min(b, r0 + rblock)
            for j0 in range(0, M, slab):
                j1 = min(M, j0 + slab)
                by = xp[rows_l[r0:r1], j0 // 4:(j1 + 3) // 4]
                code = ((by[:, :, None] >> shifts) & 3).reshape(by.shape[0], -1)[:, :j1 - j0]
                pi = Q[r0:r1, :K] @ P[j0:j1, :K].T
                m = (code != 3) & (pi >= pimin) & (pi <= 1.0 - pimin)
                r, u = torch.clamp(pi, eps, 1.0 - eps), torch.clamp(1.0 - pi, eps, 1.0 - eps)
                t = torch.where(code == 0, r / u, torch.where(code == 2, u / r, torch.full_like(pi, -1.0))) * m
                U_[j0:j1] += t.sum(dim=0)
                H_[j0:j1] += (2.0 * pi * (1.0 - pi) * m).sum(dim=0)
                n_[j0:j1] += m.sum(dim=0, dtype=torch.int32)
                o_[j0:j1] += (m & (code == 1)).sum(dim=0, dtype=torch.int32)
                if with_abs:
                    T_[j0:j1] += t.abs().sum(dim=0)
        return U_, H_, n_, o_, T_

    hip()
    want = plain(with_abs=True)
    hip()
    plain()
    torch.cuda.synchronize()
    agree_u = float(((U - want[0].double()).abs() / want[4].double().clamp(min=1e-30)).max())
    agree_h = float(((Hexp - want[1].double()).abs() / want[1].double().clamp(min=1e-30)).max())
    same_n = bool(torch.equal(nn, want[2]) and torch.equal(Hobs, want[3]))
    t = {"nadm_snp_hwe": [], "torch fp32": []}
    for _ in range(a.rounds):
        for name, f in (("nadm_snp_hwe", hip), ("torch fp32", plain)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    q = {n: np.percentile(v, [25, 50, 75]) for n, v in t.items()}
    cells = float(b) * M
    lines = [f"tools/time_project.py --hwe: b = {b} resident rows (permuted gather list), M = {M}, K = {K} (kp = {kp}), ld = {ld}; {torch.cuda.get_device_name(0)}",
             f"device events, {a.rounds} rounds, the two alternating; ms per call: median [quartiles]"]
    for n in t:
        lines.append(f"  {n:13s} {q[n][1]:10.3f}  [{q[n][0]:.3f}, {q[n][2]:.3f}]   {cells / q[n][1] / 1e6:.1f} G genotypes/s")
    lines.append(f"  nadm_snp_hwe / torch fp32 = {q['nadm_snp_hwe'][1] / q['torch fp32'][1]:.4f}; {int(lib.nadm_snp_hwe_slices(b, M))} sample slice(s), "
                 f"partials {4 * h_scratch.numel() / 1e6:.1f} MB; packed matrix {b * ld / 1e9:.2f} GB once through HBM = "
                 f"{b * ld / q['nadm_snp_hwe'][1] / 1e9:.3f} TB/s at that time")
    lines.append(f"  against the torch sums: max |U - U_torch| / T_abs = {agree_u:.2e}, max |Hexp - Hexp_torch| / Hexp = {agree_h:.2e}, "
                 f"n and Hobs {'equal' if same_n else 'DIFFER'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fb:
        fb.write(text)


if a.kinship:
    kinship_leg()
    sys.exit(0)
if a.hwe:
    hwe_leg()
    sys.exit(0)
Qo = torch.empty_like(Q)
ll = torch.empty(b, dtype=torch.float64, device=dev)
nobs = torch.empty(b, dtype=torch.int32, device=dev)
scratch = torch.empty(int(lib.nadm_project_scratch_floats(b, M, kp)), dtype=torch.float32, device=dev)
Po = torch.empty_like(P)
nsnp = torch.empty(M, dtype=torch.int32, device=dev)
p_scratch = torch.empty(int(lib.nadm_project_p_scratch_floats(b, M, kp)), dtype=torch.float32, device=dev)
chunks = int(lib.nadm_decode_chunks(M, kp))
dP, dq, loss = torch.empty_like(P), torch.empty(chunks * b * kp, dtype=torch.float32, device=dev), torch.empty(chunks, dtype=torch.float32, device=dev)


def project(with_ll):
    check(lib.nadm_project_q(ptr(xp), ld, ptr(idx), b, M, ptr(P), K, kp, ptr(Q), ptr(Qo), kp, 1e-6, 1e-6, ptr(ll) if with_ll else None,
                             ptr(nobs), ptr(scratch), st), "project_q")


def project_p():
    check(lib.nadm_project_p(ptr(xp), ld, ptr(idx), b, M, ptr(Q), kp, K, kp, ptr(P), ptr(Po), 1e-6, 1e-6, ptr(nsnp), ptr(p_scratch), st),
          "project_p")


def pass2():
    check(lib.nadm_decode_bce(ptr(xp), ld, ptr(idx), b, M, ptr(P), kp, ptr(Q), kp, ptr(dP), ptr(dq), ptr(loss), 1, st), "decode_bce")


groups = {"project": lambda: project(False), "project+ll": lambda: project(True), "project_p": project_p, "pass2": pass2}
for f in groups.values():                                   # warm-up: code objects, caches, clocks
    for _ in range(5):
        f()
torch.cuda.synchronize()
ms = {n: [] for n in groups}
for _ in range(a.rounds):
    for n, f in groups.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            f()
        e1.record()
        e1.synchronize()
        ms[n].append(e0.elapsed_time(e1) / a.calls)
q = {n: np.percentile(v, [25, 50, 75]) for n, v in ms.items()}
lines = [f"tools/time_project.py: b = {b}, M = {M}, K = {K} (kp = {kp}), {rows} resident rows, ld = {ld}; {torch.cuda.get_device_name(0)}",
         f"device events, {a.rounds} rounds x {a.calls} calls per group, the groups alternating; ms per call: median [quartiles]"]
for n in groups:
    lines.append(f"  {n:11s} {q[n][1]:8.4f}  [{q[n][0]:.4f}, {q[n][2]:.4f}]")
lines.append(f"  project / pass2 = {q['project'][1] / q['pass2'][1]:.3f}   project+ll / pass2 = {q['project+ll'][1] / q['pass2'][1]:.3f}   "
             f"project+ll / project = {q['project+ll'][1] / q['project'][1]:.3f}   project_p / pass2 = {q['project_p'][1] / q['pass2'][1]:.3f}   "
             f"project_p / project = {q['project_p'][1] / q['project'][1]:.3f}")
pairs = b * M
lines.append(f"  (sample, SNP) pairs per call {pairs:.3e}: project {pairs / q['project'][1] / 1e6:.1f} G pairs/s, packed bytes read {b * ld / 1e6:.1f} MB, "
             f"partials written + read {2 * 4 * scratch.numel() / 1e6:.1f} MB; project_p {pairs / q['project_p'][1] / 1e6:.1f} G pairs/s, "
             f"{int(lib.nadm_project_p_slices(b, M))} sample slice(s), partials at most {2 * 4 * p_scratch.numel() / 1e6:.1f} MB")
text = "\n".join(lines) + "\n"
print(text, end="")
with open(a.out, "w") as fb:
    fb.write(text)
