"""What the time_*.py scripts of the analysis modes share (time_cv, time_bootstrap, time_pse, time_qse, time_residpca, time_fitcheck, time_pca, time_king, time_ibd, time_wld): a resident synthetic
matrix drawn from a model, the quartiles of a leg's times and the device-event clock.  Imported as a sibling module: the scripts run as
``python tools/time_x.py``."""
import numpy as np
import torch

from neural_admixture_amd._lib import lib, check, ptr
from neural_admixture_amd.layout import ModelLayout


def synth_model(rows, M, K, rng, dev, st):
    """(xp [rows, ld], P [M, kp], Q [rows, kp], kp, ld): genotypes drawn from the model (P, Q), 2 % missing.  ``rng``: the script's
    numpy generator (P and Q come from it, in this order); ``dev`` / ``st``: its device and stream."""
    kp, ld = int(lib.nadm_pad_k(K)), ModelLayout.row_stride(M)
    Fq = torch.from_numpy(np.clip(0.5 * rng.beta(0.5, 0.5, size=(K, M)), 0.005, 0.5).astype(np.float32)).to(dev)
    Qt = torch.from_numpy(rng.dirichlet(0.2 * np.ones(K), size=rows).astype(np.float32)).to(dev)
    xp = torch.zeros((rows, ld), dtype=torch.uint8, device=dev)
    check(lib.nadm_synth_packed(ptr(xp), rows, 0, M, ld, ptr(Qt), ptr(Fq), K, 0.02, 7, st), "synth_packed")
    P = torch.zeros((M, kp), dtype=torch.float32, device=dev)
    P[:, :K] = Fq.T
    Q = torch.zeros((rows, kp), dtype=torch.float32, device=dev)
    Q[:, :K] = Qt
    return xp, P, Q, kp, ld


def quart(v):
    return np.percentile(np.asarray(v), [25, 50, 75])


def timed(f):
    """Milliseconds of ``f()`` on the current stream, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)
