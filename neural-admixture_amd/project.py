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

from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, model_operands, n_rows, pad_P, pad_Q, stream as _stream    # noqa: F401  (pad_P, pad_Q: also for callers that pad operands themselves)

EPS = 1e-6           # clip of the reconstruction: the log-likelihood report's (report.py)
QMIN = 1e-6          # floor of an ancestry fraction before the renormalisation
PMIN = 1e-6          # clip of a refitted allele frequency: [PMIN, 1 - PMIN]
POLISH_ROWS = 1024   # rows per Q step of polish(): bounds nadm_project_scratch_floats whatever N is


def em_step(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], b: int, Pp: torch.Tensor, k: int, qin: torch.Tensor,
            qout: torch.Tensor, scratch: torch.Tensor, eps: float = EPS, qmin: float = QMIN,
            loglik: Optional[torch.Tensor] = None, nobs: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None) -> None:
    """One ``nadm_project_q`` call on the current stream: ``Pp [M, kp]``, ``qin`` / ``qout [b, kp]`` (may be the same tensor).
    ``weights``: a uint8 device vector of M SNP weights (``check_weights``) makes it one ``nadm_project_q_w`` call instead."""
    kp = Pp.shape[1]
    if weights is not None:
        if weights.dtype != torch.uint8 or weights.device != xp.device or weights.dim() != 1 or weights.shape[0] != M or not weights.is_contiguous():
            raise RuntimeError(f"weights must be a contiguous uint8 vector of {M} entries on the matrix's device")
        check(lib.nadm_project_q_w(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Pp), k, kp, ptr(qin), ptr(qout), qin.stride(0),
                                   eps, qmin, ptr(loglik), ptr(nobs), ptr(scratch), ptr(weights), _stream()), "project_q_w")
        return
    check(lib.nadm_project_q(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Pp), k, kp, ptr(qin), ptr(qout), qin.stride(0),
                             eps, qmin, ptr(loglik), ptr(nobs), ptr(scratch), _stream()), "project_q")


def check_weights(weights: torch.Tensor, M: int) -> None:
    """The refusal the weighted Q step leaves to this layer: a sample's count of observed calls is an int32 sum of weights, so the
    weights of all M SNPs together must stay below 2^31 (one device reduction and one host read: once per fit, not per step)."""
    if int(weights.sum(dtype=torch.int64)) > 0x7FFFFFFF:
        raise RuntimeError("the SNP weights sum to more than 2^31 - 1")


def refine_heads(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], b: int, Pps: Sequence[torch.Tensor], ks: Sequence[int],
                 q0s: Sequence[torch.Tensor], iters: int, tol: float, eps: float = EPS, qmin: float = QMIN, with_loglik: bool = False,
                 weights: Optional[torch.Tensor] = None):
    """The iteration both public forms share.  ``Pps[h] [M, kp_h]``, ``q0s[h] [b, kp_h]`` (not modified).  Stops after ``iters``
    steps, or earlier once ``max |q_out - q_in| < tol`` over the batch and ALL heads (one device reduction and one host read per
    iteration).  ``weights``: SNP weights for every step (``em_step``).  Returns ``(Qs [b, kp_h], lls, nobs, iterations run)``; ``lls`` (float64 [b], at the returned Q) and ``nobs``
    (int32 [b]) per head, or None without ``with_loglik``."""
    check_packed(xp, idx, b)
    dev = xp.device
    n_scr = max(int(lib.nadm_project_scratch_floats(b, M, Pp.shape[1])) for Pp in Pps)
    scratch = torch.empty(max(n_scr, 4), dtype=torch.float32, device=dev)
    cur = [q.clone() for q in q0s]
    nxt = [torch.empty_like(q) for q in q0s]
    done = 0
    for _ in range(int(iters)):
        delta = None
        for h, Pp in enumerate(Pps):
            em_step(xp, M, idx, b, Pp, ks[h], cur[h], nxt[h], scratch, eps, qmin, weights=weights)
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
            em_step(xp, M, idx, b, Pp, ks[h], cur[h], nxt[h], scratch, eps, qmin, ll, no, weights=weights)
            lls.append(ll)
            nobs.append(no)
    return cur, lls, nobs, done


def project_q(xp: torch.Tensor, M: int, P, q0=None, iters: int = 20, tol: float = 1e-4, idx: Optional[torch.Tensor] = None,
              b: Optional[int] = None, eps: float = EPS, qmin: float = QMIN, with_loglik: bool = False):
    """Ancestry fractions of the rows ``idx[0..b)`` (default: every row) of the packed device matrix ``xp [rows, ld]`` against the
    fixed allele frequencies ``P [M, K]`` (host or device): ``iters`` masked EM steps from ``q0 [b, K]`` (None: the uniform 1/K),
    stopping early once no entry moves by ``tol``.  Returns ``Q [b, K]`` (float32, on xp's device); with ``with_loglik`` also the
    per-sample log-likelihood at that Q (float64 [b]) and the number of observed calls (int32 [b])."""
    b, K, Pp, q = model_operands(xp, M, idx, P, q0, b)
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


def project_p(xp: torch.Tensor, M: int, Q, p0=None, iters: int = 20, tol: float = 1e-5, idx: Optional[torch.Tensor] = None,
              b: Optional[int] = None, eps: float = EPS, pmin: float = PMIN) -> torch.Tensor:
    """Allele frequencies ``P [M, K]`` (float32, on xp's device) of the packed device matrix ``xp [rows, ld]`` for the FIXED ancestry
    fractions ``Q [b, K]`` of its rows ``idx[0..b)`` (default: every row): ``iters`` masked EM steps from ``p0 [M, K]``, stopping
    early once no entry moves by ``tol``.  ``p0 = None`` starts every entry at 0.5; the first step then yields the ancestry-weighted
    allele frequencies.  The SNPs need not be ones a model was trained on."""
    K = int(np.shape(Q)[1])
    if p0 is not None and tuple(np.shape(p0)) != (M, K):
        raise RuntimeError(f"p0 must be [{M}, {K}]")
    b, _, cur, Qp = model_operands(xp, M, idx, np.full((M, K), 0.5, dtype=np.float32) if p0 is None else p0, Q, b)
    nxt = torch.empty_like(cur)
    scratch = _p_scratch(b, M, [cur.shape[1]], xp.device)
    for _ in range(int(iters)):
        p_step(xp, M, idx, b, Qp, K, cur, nxt, scratch, eps, pmin)
        delta = float((nxt - cur).abs().max())
        cur, nxt = nxt, cur
        if delta < tol:
            break
    return cur[:, :K].clone()


def _summed_loglik(xp: torch.Tensor, M: int, N: int, Pps, ks, Qps, rows: int, eps: float, qmin: float, weights=None) -> float:
    """Log-likelihood of the observed calls summed over the rows 0..N and the heads, in float64: the ``ll`` of a Q step that moves
    nothing (``refine_heads`` with ``iters = 0``), in row batches."""
    total = 0.0
    for s in range(0, N, rows):
        bb = min(rows, N - s)
        _, lls, _, _ = refine_heads(xp[s:s + bb], M, None, bb, Pps, ks, [q[s:s + bb] for q in Qps], 0, 0.0, eps, qmin, with_loglik=True,
                                     weights=weights)
        total += float(sum(ll.sum() for ll in lls))
    return total


def polish(xp: torch.Tensor, M: int, Ps: Sequence, Qs: Sequence, rounds: int, tol: float = 1e-5, eps: float = EPS, qmin: float = QMIN,
           pmin: float = PMIN, weights: Optional[torch.Tensor] = None):
    """Block EM over the observed calls from a given answer: per head ``h``, ``Ps[h] [M, k_h]`` and ``Qs[h] [N, k_h]`` (host or device;
    N = the rows of ``xp``) are alternately refitted -- one round is a Q step over all rows with P fixed (in batches of POLISH_ROWS
    rows), then a P step over all rows with the new Q -- for ``rounds`` rounds, or until max |dQ| and max |dP| of a round are both
    below ``tol`` over all heads.  Returns ``(Ps, Qs, ll_before, ll_after, rounds_run)``: float32 device matrices ``[M, k_h]`` /
    ``[N, k_h]`` and the log-likelihood of the observed calls summed over samples and heads (float64) at the start and at the end.
    ``weights`` (a uint8 device vector of M entries, e.g. a bootstrap replicate's ``bootstrap.block_weights``) makes it the block EM of
    the weighted likelihood sum_j w_j l_j: every Q step and both log-likelihoods carry the weights; the P step needs none (a SNP's
    weight multiplies its numerator and denominator alike).  ``None`` is the unweighted call path as it always was."""
    if weights is not None:
        check_weights(weights, M)
    N, dev = n_rows(xp, None), xp.device
    if any(np.shape(P)[0] != M for P in Ps):
        raise RuntimeError(f"every P must have {M} rows, one per SNP")
    _, ks, Pc, Qc = (list(t) for t in zip(*(model_operands(xp, M, None, P, Q) for P, Q in zip(Ps, Qs))))
    rows = min(POLISH_ROWS, N)
    q_scratch = torch.empty(max(max(int(lib.nadm_project_scratch_floats(rows, M, Pp.shape[1])) for Pp in Pc), 4), dtype=torch.float32, device=dev)
    p_scratch = _p_scratch(N, M, [Pp.shape[1] for Pp in Pc], dev)
    ll_before = _summed_loglik(xp, M, N, Pc, ks, Qc, rows, eps, qmin, weights)
    done = 0
    for _ in range(int(rounds)):
        delta = torch.zeros((), dtype=torch.float32, device=dev)
        for h, k in enumerate(ks):
            qn, pn = torch.empty_like(Qc[h]), torch.empty_like(Pc[h])
            for s in range(0, N, rows):
                bb = min(rows, N - s)
                em_step(xp[s:s + bb], M, None, bb, Pc[h], k, Qc[h][s:s + bb], qn[s:s + bb], q_scratch, eps, qmin, weights=weights)
            p_step(xp, M, None, N, qn, k, Pc[h], pn, p_scratch, eps, pmin)
            delta = torch.maximum(delta, torch.maximum((qn - Qc[h]).abs().max(), (pn - Pc[h]).abs().max()))
            Qc[h], Pc[h] = qn, pn
        done += 1
        if float(delta) < tol:
            break
    ll_after = _summed_loglik(xp, M, N, Pc, ks, Qc, rows, eps, qmin, weights) if done else ll_before
    return [P[:, :k].clone() for P, k in zip(Pc, ks)], [Q[:, :k].clone() for Q, k in zip(Qc, ks)], ll_before, ll_after, done
