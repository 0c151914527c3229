"""A / B of two BUILDS of the library on the three launches that end in the park-and-count hand-off (csrc/nadm_common.h): the sliced
pass 2 (800 rows x 50,000 SNPs, K = 8: three slices by the library's rule), the MLP backward that builds the dZ image (the same 800
rows) and the sliced pass 3 (6400 rows x 62,500 SNPs, C = 8: two slices).  Kernel times are the plan's own HIP event records
(Engine.time_kernels) over --steps steps after --warmup.

    python tools/handoff_ab.py --parent-lib OTHER/libnadm.so [--rounds 3] [--out FILE]

runs a fresh process per build and round, the builds interleaved (parent, this tree, parent, ...), and prints per launch both means,
the parent's round-to-round spread and whether this tree's mean lies inside it.  Without --parent-lib: one round under the library
NADM_LIB names (default: this tree's), one line per launch."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8000, 50_000, 800, ("decode_bce", "mlp_bwd")), (12_800, 62_500, 6400, ("encode_bwd",)))      # resident rows, SNPs, rows per step, timed groups


def one_round(steps, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import neural_admixture_amd as na
    from neural_admixture_amd._lib import lib
    import bench                                            # make_dataset: the bench's synthetic matrix
    dev = torch.device("cuda:0")
    for rows, M, b, names in SHAPES:
        e = na.Engine(M, 8, 1024, [8], dev, b)
        e.set_packed(bench.make_dataset(e, rows, 0, 8, dev))
        rng = np.random.default_rng(0)
        e.load_params((rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32), rng.uniform(0.05, 0.95, (8, M)).astype(np.float32),
                      na.model.init_encoder_weights(42, 8, 1024, [8]))
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1000)).to(torch.int32).to(dev)
        nb = rows // b
        for s in range(warmup):
            e.train_step(perm[(s % nb) * b:(s % nb) * b + b], b, 2e-3, True)
        e.time_kernels(names)
        for s in range(steps):
            e.train_step(perm[(s % nb) * b:(s % nb) * b + b], b, 2e-3, True)
        km = e.kernel_ms()
        e.time_kernels(None)
        for n in names:
            print(f"AB {b}x{M} {n} slices_p2={lib.nadm_decode_slices(b, M, 8)} slices_p3={lib.nadm_encode_slices(b, M, 8)} {1e3 * km[n]:.2f}", flush=True)
        del e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", type=str, default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not a.parent_lib:
        return one_round(a.steps, a.warmup)
    res, lines = {}, []

    def out(t):
        print(t, flush=True)
        lines.append(t)

    out(f"hand-off A/B: parent build against this tree, {a.rounds} interleaved rounds, a fresh process each, {a.steps} steps per launch after {a.warmup}; kernel time [us] from HIP events")
    for r in range(a.rounds):
        for build, path in (("parent", os.path.abspath(a.parent_lib)), ("new", "")):
            env = dict(os.environ)
            env.pop("NADM_LIB", None)
            if path:
                env["NADM_LIB"] = path
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env,
                               capture_output=True, text=True, timeout=240)
            if p.returncode != 0:                           # nothing more is started on the GPU after a failure
                out(p.stdout + p.stderr)
                sys.exit(f"round {r} {build}: exit status {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("AB "):
                    f = line.split()
                    res.setdefault((f[1], f[2], f[3], f[4]), {"parent": [], "new": []})[build].append(float(f[5]))
                    out(f"round {r} {build:6s} {' '.join(f[1:5])}  {f[5]} us")
    out("")
    for (shape, name, s2, s3), v in res.items():
        p, n = v["parent"], v["new"]
        pm, nm = sum(p) / len(p), sum(n) / len(n)
        out(f"{shape:12s} {name:10s} parent {pm:7.2f} us (rounds {min(p):.2f}..{max(p):.2f})   new {nm:7.2f} us (rounds {min(n):.2f}..{max(n):.2f})   "
            f"new mean inside the parent's spread: {min(p) <= nm <= max(p)}   new mean <= parent's slowest round: {nm <= max(p)}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
