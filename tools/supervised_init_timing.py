#!/usr/bin/env python3
"""What the supervised decoder init (train.supervised_init) costs on the host path and on the device path (nadm_class_sums), with 30 %
of the samples unlabelled: both paths at a shape the host loop finishes in reasonable time (default 20000 x 200000, K = 8), then the
device path alone on a GPU-resident matrix of the bench's shape (100000 x 500000) against the bytes it has to read, N * M / 4.
Usage: supervised_init_timing.py [N_small M_small [N_big M_big]]  -> stdout"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_admixture_amd._lib import lib, check, ptr                  # noqa: E402
from neural_admixture_amd.io import PackedGenotypes                    # noqa: E402
from neural_admixture_amd.layout import ModelLayout                    # noqa: E402
from neural_admixture_amd.train import supervised_init                 # noqa: E402

K = 8
dev = torch.device("cuda:0")


def synth(N, M):
    ld = ModelLayout.row_stride(M)
    torch.manual_seed(1234)
    Fq = (0.5 * torch.distributions.Beta(torch.tensor(0.5), torch.tensor(0.5)).sample((K, M))).clamp(0.005, 0.5).float().to(dev)
    Qt = torch.distributions.Dirichlet(torch.full((K,), 0.2)).sample((N,)).float().to(dev)
    xp = torch.empty((N, ld), dtype=torch.uint8, device=dev)
    check(lib.nadm_synth_packed(ptr(xp), N, 0, M, ld, ptr(Qt), ptr(Fq), K, 0.01, 1234, None))
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    pops = np.asarray([f"pop{c}" for c in Qt.argmax(dim=1).cpu().numpy()], dtype=object)
    pops[rng.random(N) < 0.3] = "-"
    return xp, ld, [str(a) for a in pops]


def timed(fn):
    torch.cuda.synchronize()
    t = time.time()
    r = fn()
    torch.cuda.synchronize()
    return r, time.time() - t


def main():
    a = [int(v) for v in sys.argv[1:]]
    Ns, Ms = (a[0], a[1]) if len(a) >= 2 else (20_000, 200_000)
    Nb, Mb = (a[2], a[3]) if len(a) >= 4 else (100_000, 500_000)
    print(f"host threads {torch.get_num_threads()}, device {torch.cuda.get_device_name(0)}")
    xp, ld, pops = synth(Ns, Ms)
    n_unl = sum(p == "-" for p in pops)
    host_data = PackedGenotypes(xp.cpu(), Ns, Ms)
    print(f"{Ns} x {Ms}, K = {K}, {n_unl} samples unlabelled; packed matrix {Ns * ld / 1e9:.2f} GB")
    (yh, Ph), t_host = timed(lambda: supervised_init(host_data, pops, K, unlabelled=("-",)))
    print(f"  host path (unpack_rows + numpy sums)                      {t_host:8.3f} s")
    supervised_init(PackedGenotypes(xp[:64], 64, Ms), pops[:64], len(set(pops[:64]) - {"-"}), unlabelled=("-",), device=dev)   # first-use costs
    (yd, Pd), t_stream = timed(lambda: supervised_init(host_data, pops, K, unlabelled=("-",), device=dev))
    print(f"  device path, matrix on the host (streamed in 4096 rows)   {t_stream:8.3f} s   same bits as the host path: "
          f"{bool(np.array_equal(yd, yh) and np.array_equal(Pd, Ph))}")
    (yr, Pr), t_res = timed(lambda: supervised_init(PackedGenotypes(xp, Ns, Ms), pops, K, unlabelled=("-",), device=dev))
    print(f"  device path, matrix resident on the GPU                   {t_res:8.3f} s   same bits as the host path: "
          f"{bool(np.array_equal(yr, yh) and np.array_equal(Pr, Ph))}")
    del xp, host_data
    torch.cuda.empty_cache()

    xp, ld, pops = synth(Nb, Mb)
    n_unl = sum(p == "-" for p in pops)
    print(f"{Nb} x {Mb}, K = {K}, {n_unl} samples unlabelled; packed matrix resident on the GPU, N * M / 4 = {Nb * Mb / 4 / 1e9:.2f} GB "
          f"({(Nb - n_unl) * Mb / 4 / 1e9:.2f} GB in labelled rows)")
    (y, P), t_all = timed(lambda: supervised_init(PackedGenotypes(xp, Nb, Mb), pops, K, unlabelled=("-",), device=dev))
    print(f"  supervised_init, device path (label mapping, argsort, kernel, read-back, float64 division)   {t_all:8.3f} s")
    order = np.argsort(y, kind="stable")
    start = np.searchsorted(y[order], np.arange(K + 1)).astype(np.int64)
    idx = torch.from_numpy(order.astype(np.int32)).to(dev)
    sums = torch.zeros((K, Mb), dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(5):
        sums.zero_()
        ev[0].record()
        check(lib.nadm_class_sums(ptr(xp), ld, Nb, Mb, ptr(idx), start.ctypes.data_as(C.POINTER(C.c_int64)), K, ptr(sums), None), "class_sums")
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    read = (Nb - n_unl) * ((Mb + 15) // 16) * 4
    print(f"  nadm_class_sums alone, 5 launches: {', '.join(f'{v:.2f}' for v in ms)} ms; median {np.median(ms):.2f} ms = "
          f"{read / np.median(ms) / 1e6:.0f} GB/s over the {read / 1e9:.2f} GB of the labelled rows it reads")
    cnt = np.bincount(y[y >= 0], minlength=K)
    print(f"  check: P == sums / counts {bool(np.array_equal(P, (sums.cpu().numpy().view(np.uint32).astype(np.float64) / cnt[:, None]).astype(np.float32)))}")


if __name__ == "__main__":
    main()
