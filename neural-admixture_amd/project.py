"""Projection: fit Q to a FIXED P by maximum likelihood over the OBSERVED calls only (what ADMIXTURE calls -P), its counterpart for P
against a fixed Q, and the two alternated (``polish``): the FRAPPE / ADMIXTURE block EM over observed calls.

``project_q`` needs no encoder: a packed genotype matrix in HBM and a host ``P [M, K]`` (a ``.P`` file) are enough.  Every
iteration is one call of ``nadm_project_q`` (include/nadm.h: one masked EM step of the binomial admixture model, two launches,
reproducible bit for bit); ``Engine.project_q`` runs the same loop on the engine's own P with the encoder's Q as the start.

``project_p`` is the other half: allele frequencies for given ancestry fractions (a ``.Q`` file, say) and any genotype matrix, one
``nadm_project_p`` call per iteration.  ``polish`` alternates the two from a trained model's answer; ``Engine.polish`` and
``train(..., polish=N)`` run it on the resident matrix.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr

EPS = 1e-6           # clip of the reconstruction: the log-likelihood report's (report.py)
QMIN = 1e-6          # floor of an ancestry fraction before the renormalisation
PMIN = 1e-6          # clip of a refitted allele frequency: [PMIN, 1 - PMIN]
POLISH_ROWS = 1024   # rows per Q step of polish(): bounds nadm_project_scratch_floats whatever N is


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


def p_step(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], b: int, Qp: torch.Tensor, k: int, pin: torch.Tensor,
           pout: torch.Tensor, scratch: torch.Tensor, eps: float = EPS, pmin: float = PMIN, nobs_snp: Optional[torch.Tensor] = None) -> None:
    """One ``nadm_project_p`` call on the current stream: ``Qp [b, >= kp]`` (row s belongs to ``idx[s]``), ``pin`` / ``pout [M, kp]``
    (may be the same tensor), ``nobs_snp`` int32 [M] or None."""
    kp = pin.shape[1]
    check(lib.nadm_project_p(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Qp), Qp.stride(0), k, kp, ptr(pin), ptr(pout), eps, pmin,
                             ptr(nobs_snp), ptr(scratch), _stream()), "project_p")


def _p_scratch(b: int, M: int, kps: Sequence[int], dev) -> torch.Tensor:
    return torch.empty(max(max(int(lib.nadm_project_p_scratch_floats(b, M, kp)) for kp in kps), 4), dtype=torch.float32, device=dev)


def _check_packed(xp: torch.Tensor, idx: Optional[torch.Tensor], b: int) -> None:
    if xp.device.type != "cuda":
        raise RuntimeError("the packed matrix must be on a ROCm GPU (no CPU fallback)")
    if xp.dtype != torch.uint8 or xp.dim() != 2 or not xp.is_contiguous():
        raise RuntimeError("packed genotypes must be a contiguous uint8 [rows, ld] matrix")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < b):
        raise RuntimeError("idx must be an int32 tensor of at least b rows")


def project_p(xp: torch.Tensor, M: int, Q, p0=None, iters: int = 20, tol: float = 1e-5, idx: Optional[torch.Tensor] = None,
              b: Optional[int] = None, eps: float = EPS, pmin: float = PMIN) -> torch.Tensor:
    """Allele frequencies ``P [M, K]`` (float32, on xp's device) of the packed device matrix ``xp [rows, ld]`` for the FIXED ancestry
    fractions ``Q [b, K]`` of its rows ``idx[0..b)`` (default: every row): ``iters`` masked EM steps from ``p0 [M, K]``, stopping
    early once no entry moves by ``tol``.  ``p0 = None`` starts every entry at 0.5; the first step then yields the ancestry-weighted
    allele frequencies.  The SNPs need not be ones a model was trained on."""
    if b is None:
        b = int(idx.numel()) if idx is not None else int(xp.shape[0])
    _check_packed(xp, idx, b)
    K = int(np.shape(Q)[1])
    kp = int(lib.nadm_pad_k(K))
    if kp <= 0:
        raise RuntimeError("K must be in 1..64")
    Qp = pad_Q(Q, b, K, kp, xp.device)
    cur = pad_P(np.full((M, K), 0.5, dtype=np.float32) if p0 is None else p0, xp.device)
    if tuple(cur.shape) != (M, kp):
        raise RuntimeError(f"p0 must be [{M}, {K}]")
    nxt = torch.empty_like(cur)
    scratch = _p_scratch(b, M, [kp], xp.device)
    for _ in range(int(iters)):
        p_step(xp, M, idx, b, Qp, K, cur, nxt, scratch, eps, pmin)
        delta = float((nxt - cur).abs().max())
        cur, nxt = nxt, cur
        if delta < tol:
            break
    return cur[:, :K].clone()


def _summed_loglik(xp: torch.Tensor, M: int, N: int, Pps, ks, Qps, rows: int, eps: float, qmin: float) -> float:
    """Log-likelihood of the observed calls summed over the rows 0..N and the heads, in float64: the ``ll`` of a Q step that moves
    nothing (``refine_heads`` with ``iters = 0``), in row batches."""
    total = 0.0
    for s in range(0, N, rows):
        bb = min(rows, N - s)
        _, lls, _, _ = refine_heads(xp[s:s + bb], M, None, bb, Pps, ks, [q[s:s + bb] for q in Qps], 0, 0.0, eps, qmin, with_loglik=True)
        total += float(sum(ll.sum() for ll in lls))
    return total


def polish(xp: torch.Tensor, M: int, Ps: Sequence, Qs: Sequence, rounds: int, tol: float = 1e-5, eps: float = EPS, qmin: float = QMIN,
           pmin: float = PMIN):
    """Block EM over the observed calls from a given answer: per head ``h``, ``Ps[h] [M, k_h]`` and ``Qs[h] [N, k_h]`` (host or device;
    N = the rows of ``xp``) are alternately refitted -- one round is a Q step over all rows with P fixed (in batches of POLISH_ROWS
    rows), then a P step over all rows with the new Q -- for ``rounds`` rounds, or until max |dQ| and max |dP| of a round are both
    below ``tol`` over all heads.  Returns ``(Ps, Qs, ll_before, ll_after, rounds_run)``: float32 device matrices ``[M, k_h]`` /
    ``[N, k_h]`` and the log-likelihood of the observed calls summed over samples and heads (float64) at the start and at the end."""
    N = int(xp.shape[0])
    _check_packed(xp, None, N)
    dev = xp.device
    ks = [int(np.shape(P)[1]) for P in Ps]
    Pc = [pad_P(P, dev) for P in Ps]
    Qc = [pad_Q(Q, N, k, Pp.shape[1], dev) for Q, k, Pp in zip(Qs, ks, Pc)]
    if any(Pp.shape[0] != M for Pp in Pc):
        raise RuntimeError(f"every P must have {M} rows, one per SNP")
    rows = min(POLISH_ROWS, N)
    q_scratch = torch.empty(max(max(int(lib.nadm_project_scratch_floats(rows, M, Pp.shape[1])) for Pp in Pc), 4), dtype=torch.float32, device=dev)
    p_scratch = _p_scratch(N, M, [Pp.shape[1] for Pp in Pc], dev)
    ll_before = _summed_loglik(xp, M, N, Pc, ks, Qc, rows, eps, qmin)
    done = 0
    for _ in range(int(rounds)):
        delta = torch.zeros((), dtype=torch.float32, device=dev)
        for h, k in enumerate(ks):
            qn, pn = torch.empty_like(Qc[h]), torch.empty_like(Pc[h])
            for s in range(0, N, rows):
                bb = min(rows, N - s)
                em_step(xp[s:s + bb], M, None, bb, Pc[h], k, Qc[h][s:s + bb], qn[s:s + bb], q_scratch, eps, qmin)
            p_step(xp, M, None, N, qn, k, Pc[h], pn, p_scratch, eps, pmin)
            delta = torch.maximum(delta, torch.maximum((qn - Qc[h]).abs().max(), (pn - Pc[h]).abs().max()))
            Qc[h], Pc[h] = qn, pn
        done += 1
        if float(delta) < tol:
            break
    ll_after = _summed_loglik(xp, M, N, Pc, ks, Qc, rows, eps, qmin) if done else ll_before
    return [P[:, :k].clone() for P, k in zip(Pc, ks)], [Q[:, :k].clone() for Q, k in zip(Qc, ks)], ll_before, ll_after, done


def find_P_files(save_dir: str, name: str, ks: Sequence[int], what: str = "--refine") -> List[str]:
    """The paths ``{save_dir}/{name}.{k}.P`` for every k; a missing file ends the run, naming it (``what``: who asks)."""
    import os
    paths = [os.path.join(save_dir, f"{name}.{k}.P") for k in ks]
    for p in paths:
        if not os.path.isfile(p):
            raise SystemExit(f"    {what} needs the allele frequencies the training run wrote: {p} not found.")
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
