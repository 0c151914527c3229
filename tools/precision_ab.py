"""A / B of the step's matmul precision (nadm_plan_set_precision): "highest" against "medium" on ONE engine, the setting switched
between blocks of steps, three interleaved rounds (highest, medium, highest, medium, ...) at the bench's workload: 800 rows per step
out of a resident synthetic matrix (default 100k x 500k, K = 8, C = 8, hidden 1024).

Per round and setting: ms / step from HIP events around --steps steps (no timing records inside), then pass 1 and pass 2 [us] from
the plan's own event records (nadm_plan_timing, Engine.time_kernels) over another --steps steps.  Prints one line per block and the
spread of the rounds; --out FILE writes the same text there.

    python tools/precision_ab.py [--rows 100000] [--snps 500000] [--k 8] [--steps 200] [--no-loss] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neural_admixture_amd as na                       # noqa: E402
from neural_admixture_amd._lib import lib, check        # noqa: E402
from neural_admixture_amd.model import init_encoder_weights  # noqa: E402
import bench                                            # noqa: E402  (make_dataset: the bench's synthetic matrix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--snps", type=int, default=500_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--batch", type=int, default=800)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-loss", action="store_true", help="steps without the loss value (the bench's headline computes it every step)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    M, K, b = a.snps, a.k, a.batch
    eng = na.Engine(M, 8, a.hidden, [K], dev, b)
    eng.set_packed(bench.make_dataset(eng, a.rows, 0, K, dev))
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, (K, M)).astype(np.float32)
    eng.load_params(V0, P0, init_encoder_weights(42, 8, a.hidden, [K]))
    perm = torch.randperm(a.rows, generator=torch.Generator().manual_seed(1000)).to(torch.int32).to(dev)
    nb = a.rows // b
    s_ = [0]

    def steps(n):
        for _ in range(n):
            o = (s_[0] % nb) * b
            eng.train_step(perm[o:o + b], b, 2e-3, not a.no_loss)
            s_[0] += 1

    lines = []

    def out(t):
        print(t, flush=True)
        lines.append(t)

    out(f"precision A/B: {a.rows} x {M} resident, K = {K}, batch {b}, hidden {a.hidden}, loss value {'never' if a.no_loss else 'every step'}; "
        f"{a.rounds} interleaved rounds, {a.steps} steps per block; "
        f"device {torch.cuda.get_device_name(dev)}")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 3.0:                   # untimed clock ramp
        steps(20)
        torch.cuda.synchronize()
    res = {"highest": [], "medium": []}
    for r in range(a.rounds):
        for name, code in (("highest", 0), ("medium", 1)):
            check(lib.nadm_plan_set_precision(eng._plan, code), "plan_set_precision")
            steps(20)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            steps(a.steps)
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / a.steps
            eng.time_kernels(["encode_fwd", "decode_bce"])
            steps(a.steps)
            km = eng.kernel_ms()
            eng.time_kernels(None)
            p1, p2 = 1e3 * km["encode_fwd"], 1e3 * km["decode_bce"]
            res[name].append((ms, p1, p2))
            out(f"round {r} {name:8s} step {ms:.4f} ms   pass 1 {p1:7.1f} us   pass 2 {p2:7.1f} us")
    out("")
    for name in res:
        v = np.asarray(res[name])
        out(f"{name:8s} step {v[:, 0].mean():.4f} ms (spread {v[:, 0].min():.4f}..{v[:, 0].max():.4f})   "
            f"pass 1 {v[:, 1].mean():.1f} us ({v[:, 1].min():.1f}..{v[:, 1].max():.1f})   pass 2 {v[:, 2].mean():.1f} us ({v[:, 2].min():.1f}..{v[:, 2].max():.1f})")
    h, m = np.asarray(res["highest"]), np.asarray(res["medium"])
    gain2 = 1.0 - m[:, 2] / h[:, 2]
    gain1 = 1.0 - m[:, 1] / h[:, 1]
    gains = 1.0 - m[:, 0] / h[:, 0]
    out("medium vs highest per round: pass 2 " + ", ".join(f"{100 * g:+.1f} %" for g in -gain2) + ";  pass 1 "
        + ", ".join(f"{100 * g:+.1f} %" for g in -gain1) + ";  step " + ", ".join(f"{100 * g:+.1f} %" for g in -gains))
    out(f"pass 2 faster by >= 8 % in every round: {bool((gain2 >= 0.08).all())};  step faster in every round: {bool((gains > 0).all())}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
