"""What every caller of a library function that reads the packed genotype matrix does first (engine, project, relate, hwe, ld): the
current stream's handle, the checks of the matrix and its gather list, and the padded ``P`` / ``Q`` operands of the model
``pi = Q P^T`` (include/nadm.h: K padded to ``nadm_pad_k(K)`` columns, pad columns 0)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._lib import lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def n_rows(xp: torch.Tensor, idx: Optional[torch.Tensor]) -> int:
    """The rows a call works on: those the gather list ``idx`` names, without one every row of ``xp``."""
    return int(idx.numel()) if idx is not None else int(xp.shape[0])


def check_packed(xp: torch.Tensor, idx: Optional[torch.Tensor], b: int, what: Optional[str] = None) -> None:
    """``xp``: contiguous uint8 ``[rows, ld]`` on a GPU; ``idx``: None or int32 with at least ``b`` entries.  A caller that hands the
    whole of ``idx`` to the library names itself (``what``): the list must then be a contiguous vector on xp's device."""
    if xp.device.type != "cuda":
        raise RuntimeError("the packed matrix must be on a ROCm GPU (no CPU fallback)")
    if xp.dtype != torch.uint8 or xp.dim() != 2 or not xp.is_contiguous():
        raise RuntimeError("packed genotypes must be a contiguous uint8 [rows, ld] matrix")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < b):
        raise RuntimeError("idx must be an int32 tensor of at least b rows")
    if what is not None and idx is not None and (idx.device != xp.device or idx.dim() != 1 or not idx.is_contiguous()):
        raise RuntimeError(f"{what}: idx must be a contiguous int32 vector on the packed matrix's device")


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


def model_operands(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], P, Q, b: Optional[int] = None, what: Optional[str] = None):
    """The checks and operands of a call on ``b`` rows of ``xp`` (default: ``n_rows``) with the allele frequencies ``P [M, K]`` and
    the ancestry fractions ``Q [b, K]`` (host or device; None: uniform): ``(b, K, Pp [M, kp], Qp [b, kp])``."""
    if b is None:
        b = n_rows(xp, idx)
    check_packed(xp, idx, b, what)
    Pp = pad_P(P, xp.device)
    if Pp.shape[0] != int(M):
        raise RuntimeError(f"P has {Pp.shape[0]} rows, the genotypes {int(M)} SNPs")
    K = int(np.shape(P)[1])
    return b, K, Pp, pad_Q(Q, b, K, Pp.shape[1], xp.device)
