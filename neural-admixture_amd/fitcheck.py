"""Model fit along the sample axis: the pairwise correlation of leave-one-out residuals (evalAdmix, Garcia-Erill & Albrechtsen 2020)
from the packed genotype matrix, ``Q`` and one head's ``P``.

A clean-looking ``.Q`` does not say that the model describes the samples: a ghost population, a bottlenecked group that gets a
component of its own, or two populations that K forces into one all give tidy bar plots.  Under a good fit the residuals
``g - 2 pi`` of two samples are uncorrelated; where the model is wrong the correlation is positive inside the groups it merged or
mis-modelled and negative between them.  The plain residual correlation is biased -- a sample's own genotype sits in the frequencies
its residual is taken against, about ``-1/n`` for a pair inside a group of ``n`` unadmixed samples -- so for an ordered pair (a, b) the
frequencies are refitted WITHOUT sample b (one EM step of P from the sums ``B`` and ``C`` that ``nadm_project_p`` forms) and BOTH
residuals are taken against that refit:

    c_ab = sum_j d_aj d_bj / sqrt(sum_j d_aj^2 o_bj  sum_j d_bj^2 o_aj),    d_ij = o_ij (g_ij - 2 sum_k q_ik f^{-b}_jk)

over the SNPs b was called at (include/nadm.h, nadm_resid_cor, has the refit and its fallback).  ``c_ab`` and ``c_ba`` are different
computations; the reported value is ``(c_ab + c_ba) / 2``.  This is evalAdmix's statistic as this project understands it; the
numbers of that tool are not promised.

``em_sums`` is ``nadm_em_sums``, ``resid_cor_block`` one ``nadm_resid_cor`` call, ``resid_cor`` the sums once over all rows and then
every ORDERED block of pairs, symmetrised; ``group_means`` / ``sample_means`` summarise the matrix, ``fit_check`` puts them together
for one head, ``Engine.resid_cor`` runs on the resident matrix with the engine's own P and the encoder's final Q.  K <= 16, and
O(S^2 M K) work for S samples: at most 4096 samples' pairs here (the sums always run over every row of the fit).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, model_operands, n_rows, stream
from ._pairs import block_rows, walk

EPS = 1e-6           # clip of pi and of 1 - pi: the projection's (project.EPS)
ROWS = 1024          # rows per block side
MAX_ROWS = 4096      # NADM_RESID_COR_MAX_ROWS: rows per block side at most, and samples whose pairs the command line takes
MAX_K = 16
WARN = 0.02          # |group mean| above which the log warns: a convention, not a calibration
EM_GAP_WARN = 1e-3   # an EM step of P from the given P that moves a frequency by more than this: P is not at its own fixed point
TOO_WIDE = "K must be <= 16 for the fit check (a sample's Q row and a chunk's refitted frequencies live in registers and LDS)"


class FitResult(NamedTuple):
    """One head's fit check: ``cor`` float64 ``[S, S]`` (NaN diagonal) and ``n`` int32 ``[S, S]`` on the device; on the host
    ``groups`` (names), ``labels`` (group index per sample, int64 ``[S]``), ``means`` / ``counts`` ``[G, G]``, ``sample_mean`` /
    ``sample_n`` ``[S]`` and ``em_gap``, the largest move of a frequency under one EM step of P from the given P."""
    K: int
    cor: torch.Tensor
    n: torch.Tensor
    groups: list
    labels: np.ndarray
    means: np.ndarray
    counts: np.ndarray
    sample_mean: np.ndarray
    sample_n: np.ndarray
    em_gap: float


def _check_width(P, what: str) -> None:
    if np.ndim(P) == 2 and int(np.shape(P)[1]) > MAX_K:
        raise RuntimeError(f"{what}: {TOO_WIDE}")


def _em_sums_padded(xp, M, K, Pp, Qp, idx, b, eps):
    kp, dev = int(Pp.shape[1]), xp.device
    n_scr = int(lib.nadm_em_sums_scratch_floats(b, M, kp))
    if n_scr <= 0:
        raise RuntimeError(f"em_sums: {b} rows over {M} SNPs with K = {K} are not supported")
    scratch = torch.empty(n_scr, dtype=torch.float32, device=dev)
    B = torch.empty((M, kp), dtype=torch.float32, device=dev)
    C = torch.empty((M, kp), dtype=torch.float32, device=dev)
    check(lib.nadm_em_sums(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Qp), Qp.stride(0), K, kp, ptr(Pp), float(eps), ptr(B), ptr(C), None,
                           ptr(scratch), stream()), "em_sums")
    return B, C


def em_sums(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, eps: float = EPS):
    """The EM sums ``B_jk = sum_i q_ik g_ij / r_ij`` and ``C_jk = sum_i q_ik (2 - g_ij) / u_ij`` over the observed calls of the rows
    ``idx`` (int32, default: every row) of the packed device matrix ``xp [rows, ld]`` for ``P [M, K]`` and ``Q [b, K]`` (host or
    device; row s of Q belongs to ``idx[s]``): ``(B, C)`` float32 ``[M, kp]`` on xp's device, pad columns 0 -- the sums
    ``nadm_project_p`` forms, with its bits (``nadm_em_sums``)."""
    M = int(M)
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="em_sums")
    return _em_sums_padded(xp, M, K, Pp, Qp, idx, b, eps)


def resid_cor_scratch(ba: int, bb: int, M: int, kp: int, device) -> torch.Tensor:
    n = int(lib.nadm_resid_cor_scratch_floats(ba, bb, M, kp))
    if n <= 0:
        raise RuntimeError(f"resid_cor: a block of {ba} x {bb} rows over {M} SNPs is not supported (1..4096 rows a side, K <= 16)")
    return torch.empty(n, dtype=torch.float32, device=device)


def resid_cor_block(xp: torch.Tensor, M: int, Pp: torch.Tensor, k: int, idxA: Optional[torch.Tensor], QA: torch.Tensor,
                    idxB: Optional[torch.Tensor], QB: torch.Tensor, B: torch.Tensor, C: torch.Tensor, eps: float = EPS,
                    scratch: Optional[torch.Tensor] = None):
    """One ``nadm_resid_cor`` call on the current stream: the rows ``idxA`` (int32, None: rows 0..ba) against the LEFT-OUT rows
    ``idxB`` of the packed device matrix ``xp [rows, ld]``; ``Pp [M, kp]`` padded (``pad_P``), ``QA [ba, >= kp]`` / ``QB [bb, >= kp]``
    padded (``pad_Q``; row s belongs to ``idx[s]``), ``B`` / ``C`` ``[M, kp]`` as ``em_sums`` returns them over ALL rows of the fit.
    Returns ``(S, Ta, Tb)`` float64 ``[ba, bb]`` and ``n`` int32 ``[ba, bb]``: ``c_ab = S / sqrt(Ta Tb)``."""
    ba, bb = int(QA.shape[0]), int(QB.shape[0])
    check_packed(xp, idxA, ba)
    check_packed(xp, idxB, bb)
    for t in (Pp, QA, QB, B, C):
        if t.dtype != torch.float32 or t.dim() != 2 or t.device != xp.device or t.stride(1) != 1:
            raise RuntimeError("resid_cor_block: P, Q, B and C must be float32 matrices on the packed matrix's device")
    for t in (Pp, B, C):
        if not t.is_contiguous() or tuple(t.shape) != (int(M), int(Pp.shape[1])):
            raise RuntimeError(f"resid_cor_block: P, B and C must be contiguous [{M}, kp] matrices")
    if QA.stride(0) != QB.stride(0):
        raise RuntimeError("resid_cor_block: QA and QB must have the same row stride")
    dev, kp = xp.device, int(Pp.shape[1])
    if kp > MAX_K:
        raise RuntimeError(f"resid_cor_block: {TOO_WIDE}")
    if scratch is None:
        scratch = resid_cor_scratch(ba, bb, M, kp, dev)
    S, Ta, Tb = (torch.empty((ba, bb), dtype=torch.float64, device=dev) for _ in range(3))
    n = torch.empty((ba, bb), dtype=torch.int32, device=dev)
    check(lib.nadm_resid_cor(ptr(xp), xp.shape[1], ptr(idxA), ba, ptr(idxB), bb, M, ptr(Pp), k, kp, ptr(QA), ptr(QB), QA.stride(0),
                             ptr(B), ptr(C), float(eps), ptr(S), ptr(Ta), ptr(Tb), ptr(n), ptr(scratch), stream()), "resid_cor")
    return S, Ta, Tb, n


def _cor(S: torch.Tensor, Ta: torch.Tensor, Tb: torch.Tensor) -> torch.Tensor:
    """S / sqrt(Ta Tb), NaN where Ta Tb == 0 (no SNP both samples were called at, or a residual that is 0 throughout)."""
    den = Ta * Tb
    return torch.where(den != 0, S / torch.sqrt(den), torch.full_like(S, float("nan")))


def em_gap(Pp: torch.Tensor, B: torch.Tensor, C: torch.Tensor, K: int) -> float:
    """max |p B / (p B + (1 - p) C) - p| over the real columns with a positive denominator: how far the given P is from the fixed
    point of its own EM step (0 for a P polished to convergence against this Q)."""
    p, b, c = (t[:, :K].to(torch.float64) for t in (Pp, B, C))
    num = p * b
    den = num + (1.0 - p) * c
    gap = torch.where(den > 0, (num / den - p).abs(), torch.zeros_like(p))
    return float(gap.max()) if gap.numel() else 0.0


def _resid_cor(xp, M, P, Q, idx, pairs_idx, rows, eps):
    _check_width(P, "resid_cor")
    M, rows = int(M), block_rows(rows)                          # (refused before the matrix is looked at)
    N, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="resid_cor")
    dev = xp.device
    if pairs_idx is None:
        pos = torch.arange(N, dtype=torch.int64, device=dev)
    else:
        pos = torch.as_tensor(np.asarray(pairs_idx) if not isinstance(pairs_idx, torch.Tensor) else pairs_idx).to(device=dev, dtype=torch.int64)
        if pos.dim() != 1 or pos.numel() < 1 or int(pos.min()) < 0 or int(pos.max()) >= N:
            raise RuntimeError(f"resid_cor: pairs_idx must name rows 0..{N - 1} of the fit")
    S_ = int(pos.numel())
    B, C = _em_sums_padded(xp, M, K, Pp, Qp, idx, N, eps)       # once, over ALL rows of the fit
    mrows = (idx.to(torch.int64)[pos] if idx is not None else pos).to(torch.int32).contiguous()     # matrix rows of the pairs' samples
    Qs = Qp[pos].contiguous()
    rows, blocks = walk(S_, rows, mrows, dev, ordered=True)     # ALL ordered blocks: c_ab and c_ba are different computations
    scratch = resid_cor_scratch(rows, rows, M, int(Pp.shape[1]), dev)
    c = torch.empty((S_, S_), dtype=torch.float64, device=dev)
    n = torch.empty((S_, S_), dtype=torch.int32, device=dev)
    for a, ba, ia, b, bb, ib in blocks:
        Sab, Ta, Tb, nn = resid_cor_block(xp, M, Pp, K, ia, Qs[a:a + ba], ib, Qs[b:b + bb], B, C, eps, scratch)
        c[a:a + ba, b:b + bb] = _cor(Sab, Ta, Tb)
        n[a:a + ba, b:b + bb] = nn
    cor = (c + c.T) * 0.5                                       # symmetric bit for bit: x + y == y + x
    cor.fill_diagonal_(float("nan"))
    return cor, n, em_gap(Pp, B, C, K)


def resid_cor(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, pairs_idx=None, rows: int = ROWS, eps: float = EPS):
    """The symmetrised correlation of leave-one-out residuals among the samples ``pairs_idx`` (positions 0..N-1 into the rows of
    the fit; default: all of them) for ``P [M, K]`` and ``Q [N, K]`` (host or device; row s of Q belongs to ``idx[s]``, default:
    row s of ``xp``).  The EM sums are computed once over ALL N rows; every ordered ``rows`` x ``rows`` block of pairs is one
    ``nadm_resid_cor`` call and one block of sums is held at a time.  Returns ``(cor float64 [S, S]`` with a NaN diagonal, ``n int32
    [S, S])`` on xp's device; ``cor`` is symmetric bit for bit, NaN where a pair shares no call."""
    cor, n, _ = _resid_cor(xp, M, P, Q, idx, pairs_idx, rows, eps)
    return cor, n


def group_means(cor, labels, groups: Optional[Sequence] = None):
    """The G x G matrix of mean correlations between the groups of ``labels`` (one per sample; ``groups``: their order, default the
    sorted distinct labels): within a group over the pairs a < b, between two groups over every pair; NaN pairs are skipped and a
    cell without a pair is NaN.  Returns ``(means float64 [G, G], counts int64 [G, G], groups)``."""
    c = np.asarray(cor.cpu() if torch.is_tensor(cor) else cor, dtype=np.float64)
    labels = np.asarray(labels)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or labels.shape != (c.shape[0],):
        raise RuntimeError("group_means: cor must be [S, S] and labels [S]")
    groups = list(np.unique(labels)) if groups is None else list(groups)
    G = len(groups)
    means = np.full((G, G), np.nan)
    counts = np.zeros((G, G), dtype=np.int64)
    members = [np.flatnonzero(labels == g) for g in groups]
    for x in range(G):
        for y in range(x, G):
            blk = c[np.ix_(members[x], members[y])]
            if x == y:
                blk = blk[np.triu_indices(len(members[x]), 1)]
            ok = ~np.isnan(blk)
            counts[x, y] = counts[y, x] = int(ok.sum())
            if ok.any():
                means[x, y] = means[y, x] = float(blk[ok].mean())
    return means, counts, groups


def sample_means(cor):
    """Per sample, the mean correlation with every other sample (NaN pairs and the diagonal skipped) and the number of pairs behind
    it: ``(mean float64 [S], n_pairs int64 [S])``; NaN for a sample without a pair."""
    c = np.asarray(cor.cpu() if torch.is_tensor(cor) else cor, dtype=np.float64).copy()
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise RuntimeError("sample_means: cor must be [S, S]")
    np.fill_diagonal(c, np.nan)
    ok = ~np.isnan(c)
    n = ok.sum(axis=1).astype(np.int64)
    s = np.where(ok, c, 0.0).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, np.nan), n


def default_labels(Q):
    """Without population labels every sample goes to its largest component: ``(labels '1'..'K' per sample, the K group names)``."""
    q = np.asarray(Q.cpu() if torch.is_tensor(Q) else Q)
    names = [str(k + 1) for k in range(q.shape[1])]
    return np.asarray(names)[np.argmax(q, axis=1)], names


def fit_check(xp: torch.Tensor, M: int, P, Q, labels=None, pairs_idx=None, rows: int = ROWS, eps: float = EPS) -> FitResult:
    """``resid_cor`` and its summaries for one head: ``labels`` one group name per row of the fit (default: the largest component,
    named 1..K); ``pairs_idx`` as in ``resid_cor``."""
    K = int(np.shape(P)[1])
    if labels is None:
        labels, names = default_labels(Q)
    else:
        labels = np.asarray([str(x) for x in labels])
        names = sorted(set(labels.tolist()))
    if labels.shape[0] != n_rows(xp, None):
        raise RuntimeError(f"fit_check: {labels.shape[0]} labels for {n_rows(xp, None)} samples")
    cor, n, gap = _resid_cor(xp, M, P, Q, None, pairs_idx, rows, eps)
    if pairs_idx is not None:
        labels = labels[np.asarray(pairs_idx.cpu() if torch.is_tensor(pairs_idx) else pairs_idx, dtype=np.int64)]
    names = [g for g in names if (labels == g).any()]
    means, counts, names = group_means(cor, labels, names)
    sm, sn = sample_means(cor)
    code = {g: i for i, g in enumerate(names)}
    return FitResult(K, cor, n, names, np.asarray([code[x] for x in labels.tolist()], dtype=np.int64), means, counts, sm, sn, gap)


def _within_between(r: FitResult):
    """Pair-weighted mean correlation within groups and between groups, and the largest |group mean| (NaN cells skipped)."""
    G = len(r.groups)
    d = np.eye(G, dtype=bool)
    up = np.triu(np.ones((G, G), dtype=bool), 1)
    out = []
    for sel in (d, up):
        ok = sel & ~np.isnan(r.means) & (r.counts > 0)
        out.append(float((r.means[ok] * r.counts[ok]).sum() / r.counts[ok].sum()) if ok.any() else float("nan"))
    have = ~np.isnan(r.means)
    return out[0], out[1], (float(np.abs(r.means[have]).max()) if have.any() else float("nan"))


def write_results(save_dir, name: str, results: Sequence[FitResult], matrix: bool = False) -> None:
    """Per head ``{save_dir}/{name}.{K}.cor_pop`` (a header line of group names, then the G rows of mean correlations),
    ``.cor_sample`` (``mean_cor n_pairs`` per sample) and, with ``matrix``, ``.cor`` (S x S in the ``.Q`` text format, ``nan`` on the
    diagonal and where a pair shares no call)."""
    from .io import savetxt
    os.makedirs(save_dir, exist_ok=True)
    for r in results:
        stem = os.path.join(save_dir, f"{name}.{r.K}")
        with open(stem + ".cor_pop", "w") as fb:
            fb.write(" ".join(str(g) for g in r.groups) + "\n")
            for row in r.means:
                fb.write(" ".join(f"{v:.8f}" for v in row.tolist()) + "\n")
        with open(stem + ".cor_sample", "w") as fb:
            for m, c in zip(r.sample_mean.tolist(), r.sample_n.tolist()):
                fb.write(f"{m:.8f} {c:d}\n")
        if matrix:
            a = r.cor.cpu().numpy().astype(np.float32)
            a[np.isnan(a)] = np.float32("nan")                  # one NaN: the positive quiet one, printed as `nan`
            savetxt(stem + ".cor", a)


def log_results(results: Sequence[FitResult], log, warn: float = WARN) -> None:
    """Per K one line (the mean within-group and between-group correlation, the largest |group mean|), a warning line for every
    group pair whose mean exceeds ``warn`` in magnitude, with the way to read it, and a warning when P is not at the fixed point of
    its own EM step (the leave-one-out refit is an EM step from the given P: it then moves every frequency, not only by b's share)."""
    for r in results:
        w, b, top = _within_between(r)
        log.info(f"Fit check (K={r.K}): mean residual correlation within groups {w:.4f}, between groups {b:.4f}; largest |group mean| "
                 f"{top:.4f} over {len(r.groups)} groups, {len(r.sample_mean)} samples (a good fit gives 0 everywhere).")
        for x, gx in enumerate(r.groups):
            for y in range(x, len(r.groups)):
                v = r.means[x, y]
                if np.isnan(v) or abs(v) <= warn:
                    continue
                if x == y:
                    how = ("positive within a group: unmodelled structure or relatedness there" if v > 0 else
                           "negative within a group: the group is split over components it should not be")
                    log.info(f"    Warning (K={r.K}): group {gx}: mean correlation {v:+.4f} over {int(r.counts[x, y])} pairs ({how}).")
                else:
                    how = ("negative between groups: they share a component they should not" if v < 0 else
                           "positive between groups: they share structure the model does not carry")
                    log.info(f"    Warning (K={r.K}): groups {gx} and {r.groups[y]}: mean correlation {v:+.4f} over {int(r.counts[x, y])} pairs ({how}).")
        log.info(f"    Largest move of a frequency under one EM step of P from the given P (K={r.K}): {r.em_gap:.2e}.")
        if r.em_gap > EM_GAP_WARN:
            log.info(f"    Warning (K={r.K}): P is not at the fixed point of its own EM step (above {EM_GAP_WARN:g}): the leave-one-out refit then "
                     "moves every frequency, not only by the left-out sample's share, and the correlations carry that.  The network's P "
                     "reads a missing call as genotype 0: run train --polish first.")
