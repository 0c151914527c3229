"""Projection: fit Q to a FIXED P by maximum likelihood over the OBSERVED calls only (what ADMIXTURE calls -P).

``project_q`` needs no encoder: a packed genotype matrix in HBM and a host ``P [M, K]`` (a ``.P`` file) are enough.  Every
iteration is one call of ``nadm_project_q`` (include/nadm.h: one masked EM step of the binomial admixture model, two launches,
reproducible bit for bit); ``Engine.project_q`` runs the same loop on the engine's own P with the encoder's Q as the start.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr

EPS = 1e-6           # clip of the reconstruction: the log-likelihood report's (report.py)
QMIN = 1e-6          # floor of an ancestry fraction before the renormalisation


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pad_P(P, device: torch.device) -> torch.Tensor:
    """Host or device ``P [M, K]`` -> contiguous float32 ``[M, nadm_pad_k(K)]`` on ``device``, pad columns 0."""
    Pt = torch.as_tensor(np.asarray(P) if not isinstance(P, torch.Tensor) else P).to(torch.float32)
    if Pt.dim() != 2:
        raise RuntimeError("P must be a matrix [M, K]")
    M, K = Pt.shape
    kp = int(lib.nadm_pad_k(K))
    if kp <= 0:
        raise RuntimeError("K must be in 1..64")
    out = torch.zeros((M, kp), dtype=torch.float32, device=device)
    out[:, :K] = Pt.to(device)
    return out


def pad_Q(q, b: int, k: int, kp: int, device: torch.device) -> torch.Tensor:
    """``q [b, k]`` (None: the uniform 1/k) -> contiguous float32 ``[b, kp]`` on ``device``, pad columns 0."""
    out = torch.zeros((b, kp), dtype=torch.float32, device=device)
    if q is None:
        out[:, :k] = 1.0 / k
        return out
    qt = torch.as_tensor(np.asarray(q) if not isinstance(q, torch.Tensor) else q).to(torch.float32)
    if tuple(qt.shape) != (b, k):
        raise RuntimeError(f"q0 must be [{b}, {k}]")
    out[:, :k] = qt.to(device)
    return out


def em_step(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], b: int, Pp: torch.Tensor, k: int, qin: torch.Tensor,
            qout: torch.Tensor, scratch: torch.Tensor, eps: float = EPS, qmin: float = QMIN,
            loglik: Optional[torch.Tensor] = None, nobs: Optional[torch.Tensor] = None) -> None:
    """One ``nadm_project_q`` call on the current stream: ``Pp [M, kp]``, ``qin`` / ``qout [b, kp]`` (may be the same tensor)."""
    kp = Pp.shape[1]
    check(lib.nadm_project_q(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Pp), k, kp, ptr(qin), ptr(qout), qin.stride(0),
                             eps, qmin, ptr(loglik), ptr(nobs), ptr(scratch), _stream()), "project_q")


def refine_heads(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], b: int, Pps: Sequence[torch.Tensor], ks: Sequence[int],
                 q0s: Sequence[torch.Tensor], iters: int, tol: float, eps: float = EPS, qmin: float = QMIN, with_loglik: bool = False):
    """The iteration both public forms share.  ``Pps[h] [M, kp_h]``, ``q0s[h] [b, kp_h]`` (not modified).  Stops after ``iters``
    steps, or earlier once ``max |q_out - q_in| < tol`` over the batch and ALL heads (one device reduction and one host read per
    iteration).  Returns ``(Qs [b, kp_h], lls, nobs, iterations run)``; ``lls`` (float64 [b], at the returned Q) and ``nobs``
    (int32 [b]) per head, or None without ``with_loglik``."""
    if xp.dtype != torch.uint8 or xp.dim() != 2 or not xp.is_contiguous():
        raise RuntimeError("packed genotypes must be a contiguous uint8 [rows, ld] matrix")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < b):
        raise RuntimeError("idx must be an int32 tensor of at least b rows")
    dev = xp.device
    n_scr = max(int(lib.nadm_project_scratch_floats(b, M, Pp.shape[1])) for Pp in Pps)
    scratch = torch.empty(max(n_scr, 4), dtype=torch.float32, device=dev)
    cur = [q.clone() for q in q0s]
    nxt = [torch.empty_like(q) for q in q0s]
    done = 0
    for _ in range(int(iters)):
        delta = None
        for h, Pp in enumerate(Pps):
            em_step(xp, M, idx, b, Pp, ks[h], cur[h], nxt[h], scratch, eps, qmin)
            d = (nxt[h] - cur[h]).abs().max()
            delta = d if delta is None else torch.maximum(delta, d)
        cur, nxt = nxt, cur
        done += 1
        if float(delta) < tol:
            break
    lls = nobs = None
    if with_loglik:                                          # ll is reported at the step's INPUT: one more pass at the final Q
        lls, nobs = [], []
        for h, Pp in enumerate(Pps):
            ll = torch.empty(b, dtype=torch.float64, device=dev)
            no = torch.empty(b, dtype=torch.int32, device=dev)
            em_step(xp, M, idx, b, Pp, ks[h], cur[h], nxt[h], scratch, eps, qmin, ll, no)
            lls.append(ll)
            nobs.append(no)
    return cur, lls, nobs, done


def project_q(xp: torch.Tensor, M: int, P, q0=None, iters: int = 20, tol: float = 1e-4, idx: Optional[torch.Tensor] = None,
              b: Optional[int] = None, eps: float = EPS, qmin: float = QMIN, with_loglik: bool = False):
    """Ancestry fractions of the rows ``idx[0..b)`` (default: every row) of the packed device matrix ``xp [rows, ld]`` against the
    fixed allele frequencies ``P [M, K]`` (host or device): ``iters`` masked EM steps from ``q0 [b, K]`` (None: the uniform 1/K),
    stopping early once no entry moves by ``tol``.  Returns ``Q [b, K]`` (float32, on xp's device); with ``with_loglik`` also the
    per-sample log-likelihood at that Q (float64 [b]) and the number of observed calls (int32 [b])."""
    if xp.device.type != "cuda":
        raise RuntimeError("project_q needs the packed matrix on a ROCm GPU (no CPU fallback)")
    if b is None:
        b = int(idx.numel()) if idx is not None else int(xp.shape[0])
    Pp = pad_P(P, xp.device)
    if Pp.shape[0] != M:
        raise RuntimeError(f"P has {Pp.shape[0]} rows, the genotypes {M} SNPs")
    K = int(np.shape(P)[1])
    q = pad_Q(q0, b, K, Pp.shape[1], xp.device)
    Qs, lls, nobs, _ = refine_heads(xp, M, idx, b, [Pp], [K], [q], iters, tol, eps, qmin, with_loglik)
    Q = Qs[0][:, :K].clone()
    return (Q, lls[0], nobs[0]) if with_loglik else Q


def find_P_files(save_dir: str, name: str, ks: Sequence[int]) -> List[str]:
    """The paths ``{save_dir}/{name}.{k}.P`` for every k; a missing file ends the run, naming it."""
    import os
    paths = [os.path.join(save_dir, f"{name}.{k}.P") for k in ks]
    for p in paths:
        if not os.path.isfile(p):
            raise SystemExit(f"    --refine needs the allele frequencies the training run wrote: {p} not found.")
    return paths


def read_P_files(paths: Sequence[str], ks: Sequence[int], num_snps: int) -> List[np.ndarray]:
    """One ``.P`` file per k -> float32 [M, k]; a row count other than the model's number of SNPs ``num_snps`` (the rows of the
    checkpoint's V: the config's ``num_features`` is the width of the encoder's input, not M) ends the run, naming the file."""
    out = []
    for p, k in zip(paths, ks):
        a = np.loadtxt(p, dtype=np.float32, ndmin=2)
        if a.shape[0] != int(num_snps) or a.shape[1] != int(k):
            raise SystemExit(f"    {p} holds a {a.shape[0]} x {a.shape[1]} matrix, the model needs {int(num_snps)} x {int(k)}.")
        out.append(a)
    return out
