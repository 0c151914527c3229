"""Time one projection step (nadm_project_q, include/nadm.h) and its counterpart for P (nadm_project_p) next to pass 2 at the same shape.
    python tools/time_project.py [--b 800] [--M 500000] [--K 8] [--rounds 30] [--out profiles/project_p.txt]

Four launch groups on the same resident matrix (admixture-model genotypes from nadm_synth_packed, 2 % missing, the batch = b random
rows of 4 b resident ones), the same P and Q:
    project        nadm_project_q, loglik == NULL (an iteration of the refinement: accumulate + fold)
    project+ll     nadm_project_q with loglik (the logarithms; the first and the last pass of a refinement)
    project_p      nadm_project_p (the P step of a polish round: accumulate + fold)
    pass2          nadm_decode_bce, with_loss = 1, no Adam: the same two products Q.P^T and dR.P plus dP, the yardstick
Each is warmed up, then timed with device events over `rounds` rounds in which the four alternate (what shares the box shifts all
four alike); a timed window is 10 back-to-back calls.  Reported: the median per call and the quartiles, and the ratios to pass 2."""
import argparse
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from neural_admixture_amd._lib import lib, check, ptr  # noqa: E402
from neural_admixture_amd.layout import ModelLayout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=800)
ap.add_argument("--M", type=int, default=500_000)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default="profiles/project_p.txt")
a = ap.parse_args()
assert torch.cuda.is_available(), "time_project.py measures on the GPU; there is no fallback"
dev = torch.device("cuda:0")
b, M, K = a.b, a.M, a.K
kp, ld, rows = int(lib.nadm_pad_k(K)), ModelLayout.row_stride(M), 4 * b
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
