"""Residual PCA given ``Q`` and ``P``: the principal components of the model's standardised (Pearson) residuals, straight from the
packed matrix in HBM.  What structure is left in the data after the K components have been taken out, and which samples carry it?

With ``pi_ij = sum_k q_ik p_jk`` the standardised residual of a call is

    a_ij = m_ij (g_ij - 2 pi_ij) / sqrt(2 pi_ij (1 - pi_ij))          (m: observed and pimin <= pi <= 1 - pimin)

Under a good fit every entry has mean 0 and variance 1, so the spectrum of ``A A^T / M_eff`` is a Marchenko-Pastur bulk with a known
upper edge; a ghost population, two populations that K forced into one or a batch effect stick out as eigenvalues above the edge, and
their eigenvectors name the samples.  PC-Relate and PCAngsd standardise by the individual-specific frequency for the same reason.
``fitcheck`` (evalAdmix's pairwise residual correlation) answers the same question for pairs at O(N^2 M K) and has to subsample above
4096 samples; this is O(N M (K + columns)) per product.  ``pca`` looks at the genotypes, whose top PCs are the structure the model
has already explained.

``A`` is never formed: ``resid_project`` / ``resid_project_t`` are ``nadm_resid_project`` / ``nadm_resid_project_t`` (include/nadm.h:
reproducible bit for bit), and the subspace iteration is ``pca.subspace_pcs``, the one ``pca.pca`` runs.  Definitions: ``M_eff`` the
SNPs with an included call, ``N_eff`` the rows with one, ``total = sum_i ss_i / M_eff`` the trace of ``A A^T / M_eff``, and

    edge = (total / N_eff) (1 + sqrt(N_eff / M_eff))^2

the Marchenko-Pastur upper edge at the MEASURED mean variance ``total / N_eff`` (1 under the model; trace-normalised, so that a fit
whose residual variance is off by a common factor does not move every ratio).  ``ratio = eigenvalue / edge``; above about 1.5 (a
convention: DESIGN.md section 4.19 has the simulated panels behind it) a PC is structure the K components do not describe.  LD
between SNPs inflates the whole spectrum -- the edge assumes independent columns -- so use LD-pruned data.  K <= 16."""
from __future__ import annotations

import logging
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import model_operands, stream
from . import pca as _pca

log = logging.getLogger(__name__)

EPS = 1e-6           # clip of pi and of 1 - pi: the projection's (project.EPS)
PIMIN = 0.01         # calls whose pi is outside [PIMIN, 1 - PIMIN] are left out: their residual is heavy-tailed
WARN = 1.5           # eigenvalue / edge above which the log warns: a convention, not a calibration
ROW_BLOCK = 32768    # rows per call of either product: bounds the scratch whatever b is
MAX_K = 16
TOO_WIDE = "K must be <= 16 for the residual PCA (a row of q or p lives in one thread's registers beside the column sums)"


class ResidPcaResult(NamedTuple):
    K: int
    eigenvalues: np.ndarray      # float64 [pcs], descending: of A A^T / M_eff
    eigenvectors: np.ndarray     # float64 [N, pcs], unit norm, the entry of largest magnitude positive; 0 for a row without a call
    M_eff: int                   # SNPs with an included call
    N_eff: int                   # rows with an included call
    total: float                 # sum_ij a_ij^2 / M_eff
    edge: float                  # (total / N_eff) (1 + sqrt(N_eff / M_eff))^2
    ratio: np.ndarray            # eigenvalues / edge


def check_args(pcs: int, oversample: int, iters: int, pimin: float) -> int:
    """The refusals that need neither data nor a GPU; returns ``L = pcs + oversample``."""
    try:
        L = _pca.check_args(pcs, oversample, iters, 0.0)
    except RuntimeError as e:
        raise RuntimeError("resid_" + str(e)) from None
    if not 0.0 <= float(pimin) < 0.5:
        raise RuntimeError("resid_pca: pimin must be in [0, 0.5)")
    return L


def _check_width(P, what: str) -> None:
    if np.ndim(P) == 2 and int(np.shape(P)[1]) > MAX_K:
        raise RuntimeError(f"{what}: {TOO_WIDE}")


def _project(xp, M, K, Pp, Qp, idx, b, W, C, pimin, eps, scratch=None):
    """``nadm_resid_project`` over blocks of at most ROW_BLOCK rows (a row is its own output: the blocks are independent)."""
    CP, kp, ld, dev = int(W.shape[1]), int(Pp.shape[1]), int(xp.shape[1]), xp.device
    need = int(lib.nadm_resid_project_scratch_floats(min(b, ROW_BLOCK), M, CP))
    if need <= 0:
        raise RuntimeError(f"resid_project: a block of {b} rows over {M} SNPs with {CP} columns is not supported")
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    Y = torch.empty((b, CP), dtype=torch.float32, device=dev)
    ss = torch.empty(b, dtype=torch.float64, device=dev)
    n = torch.empty(b, dtype=torch.int32, device=dev)
    for s in range(0, b, ROW_BLOCK):
        bb = min(ROW_BLOCK, b - s)
        rows, xb = (idx[s:s + bb], xp) if idx is not None else (None, xp[s:s + bb])
        check(lib.nadm_resid_project(ptr(xb), ld, ptr(rows), bb, M, ptr(Pp), K, kp, ptr(Qp[s:s + bb]), Qp.stride(0), float(eps),
                                     float(pimin), ptr(W), int(C), CP, ptr(Y[s:s + bb]), ptr(ss[s:s + bb]), ptr(n[s:s + bb]),
                                     ptr(scratch), stream()), "resid_project")
    return Y, ss, n


def _project_t(xp, M, K, Pp, Qp, idx, b, Yin, C, pimin, eps, scratch=None):
    """``nadm_resid_project_t`` over blocks of at most ROW_BLOCK rows; more than one block: the blocks' fp32 results are added in
    float64 in block order and rounded once, the counts as integers (a fixed function of the shape)."""
    CP, kp, ld, dev = int(Yin.shape[1]), int(Pp.shape[1]), int(xp.shape[1]), xp.device
    need = int(lib.nadm_resid_project_t_scratch_floats(min(b, ROW_BLOCK), M, kp, CP))
    if need <= 0:
        raise RuntimeError(f"resid_project_t: a block of {b} rows over {M} SNPs with {CP} columns is not supported")
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    O = n = None
    for s in range(0, b, ROW_BLOCK):
        bb = min(ROW_BLOCK, b - s)
        rows, xb = (idx[s:s + bb], xp) if idx is not None else (None, xp[s:s + bb])
        blk_O = torch.empty((M, CP), dtype=torch.float32, device=dev)
        blk_n = torch.empty(M, dtype=torch.int32, device=dev)
        check(lib.nadm_resid_project_t(ptr(xb), ld, ptr(rows), bb, M, ptr(Pp), K, kp, ptr(Qp[s:s + bb]), Qp.stride(0), float(eps),
                                       float(pimin), ptr(Yin[s:s + bb]), int(C), CP, ptr(blk_O), ptr(blk_n), ptr(scratch), stream()),
              "resid_project_t")
        if b <= ROW_BLOCK:                                   # one block: its result as it is
            return blk_O, blk_n
        O = blk_O.to(torch.float64) if O is None else O + blk_O.to(torch.float64)
        n = blk_n if n is None else n + blk_n
    return O.to(torch.float32), n


def resid_project(xp: torch.Tensor, M: int, P, Q, W: torch.Tensor, C: int, idx: Optional[torch.Tensor] = None, pimin: float = PIMIN,
                  scratch: Optional[torch.Tensor] = None, eps: float = EPS):
    """``Y[i, c] = sum_j a_ij W[j, c]`` with the standardised residuals ``a`` of the module docstring, over the rows ``idx`` (int32,
    default: every row) of the packed device matrix ``xp [rows, ld]``, the allele frequencies ``P [M, K]`` and the ancestry fractions
    ``Q [b, K]`` (host or device; row s of Q belongs to ``idx[s]``).  ``W`` float32 ``[M, CP]`` on xp's device, CP 16 or 32, ``C``
    columns in use.  Returns ``(Y float32 [b, CP]`` with pad columns zero, ``ss float64 [b]`` the rows' sums of squares of ``a``,
    ``nobs int32 [b]`` their included calls)."""
    M = int(M)
    _check_width(P, "resid_project")
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="resid_project")
    CP = int(W.shape[1]) if torch.is_tensor(W) and W.dim() == 2 else 0
    _pca._operand(W, M, CP, "resid_project: W")
    with torch.cuda.device(xp.device):
        return _project(xp, M, K, Pp, Qp, idx, b, W, C, pimin, eps, scratch)


def resid_project_t(xp: torch.Tensor, M: int, P, Q, Yin: torch.Tensor, C: int, idx: Optional[torch.Tensor] = None,
                    pimin: float = PIMIN, scratch: Optional[torch.Tensor] = None, eps: float = EPS):
    """``O[j, c] = sum_i a_ij Yin[i, c]`` (arguments as ``resid_project``; ``Yin`` float32 ``[b, CP]``, row s belongs to ``idx[s]``).
    Returns ``(O float32 [M, CP]`` with pad columns zero, ``nobs_snp int32 [M]`` the SNPs' included calls)."""
    M = int(M)
    _check_width(P, "resid_project_t")
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="resid_project_t")
    CP = int(Yin.shape[1]) if torch.is_tensor(Yin) and Yin.dim() == 2 else 0
    _pca._operand(Yin, b, CP, "resid_project_t: Yin")
    with torch.cuda.device(xp.device):
        return _project_t(xp, M, K, Pp, Qp, idx, b, Yin, C, pimin, eps, scratch)


def mp_edge(total: float, n_eff: int, m_eff: int) -> float:
    """The Marchenko-Pastur upper edge of ``A A^T / M_eff`` for ``A [N_eff, M_eff]`` of independent entries whose mean variance is
    ``total / N_eff``."""
    return (total / n_eff) * (1.0 + np.sqrt(n_eff / m_eff)) ** 2


def resid_pca(xp: torch.Tensor, M: int, P, Q, pcs: int = 10, oversample: int = 10, iters: int = 10, pimin: float = PIMIN,
              seed: int = 42, idx=None) -> ResidPcaResult:
    """The top ``pcs`` principal components of the standardised residuals of the samples ``idx`` (default: every row) of the packed
    device matrix given ``P [M, K]`` and ``Q [b, K]``: eigenvalues and eigenvectors of ``A A^T / M_eff`` (module docstring) by
    ``pca.subspace_pcs`` on ``L = pcs + oversample <= 32`` columns, with the Marchenko-Pastur edge they are to be read against."""
    L = check_args(pcs, oversample, iters, pimin)
    _check_width(P, "resid_pca")
    pcs, iters, M = int(pcs), int(iters), int(M)
    if idx is not None and not torch.is_tensor(idx):
        idx = torch.from_numpy(np.ascontiguousarray(np.asarray(idx), dtype=np.int32)).to(xp.device)
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="resid_pca")
    if pcs > b:
        raise RuntimeError(f"resid_pca: {pcs} components were asked of {b} samples")
    dev, CP, kp = xp.device, _pca.pad_columns(L), int(Pp.shape[1])
    seen = {}
    with torch.cuda.device(dev):
        bb = min(b, ROW_BLOCK)
        fwd_scratch = torch.empty(max(int(lib.nadm_resid_project_scratch_floats(bb, M, CP)), 4), dtype=torch.float32, device=dev)
        t_scratch = torch.empty(max(int(lib.nadm_resid_project_t_scratch_floats(bb, M, kp, CP)), 4), dtype=torch.float32, device=dev)

        def a_times(Wd):                                     # A W: W float64 [M, CP] on the device, pad columns 0 -> host float64 [b, L]
            Y, ss, n = _project(xp, M, K, Pp, Qp, idx, b, Wd.to(torch.float32), L, pimin, EPS, fwd_scratch)
            seen["ss"], seen["n"] = ss, n
            return Y[:, :L].cpu().numpy().astype(np.float64)

        def at_times(Qh):                                    # A^T Q: Q host float64 [b, <= L] -> float64 [M, CP] on the device, pad columns 0
            Yp = np.zeros((b, CP), dtype=np.float32)
            Yp[:, :Qh.shape[1]] = Qh
            O, n_snp = _project_t(xp, M, K, Pp, Qp, idx, b, torch.from_numpy(Yp).to(dev), L, pimin, EPS, t_scratch)
            seen["n_snp"] = n_snp
            return O.to(torch.float64)

        def m_eff():
            m = int((seen["n_snp"] > 0).sum())
            if m == 0:
                raise RuntimeError(f"resid_pca: no call is left: every call is missing or has its frequency outside [{float(pimin):g}, "
                                   f"{1.0 - float(pimin):g}]")
            return m

        values, vectors = _pca.subspace_pcs(a_times, at_times, M, L, CP, pcs, iters, seed, dev, m_eff)
        have = (seen["n"] > 0).cpu().numpy()
        vectors[~have] = 0.0                                 # (its row of A is zero: Householder QR leaves it at 1e-17, not at 0)
        m, n_eff = m_eff(), int(have.sum())
        total = float(seen["ss"].sum()) / m
    edge = float(mp_edge(total, n_eff, m))
    return ResidPcaResult(K, values, vectors, m, n_eff, total, edge, values / edge)


def _groups(res: ResidPcaResult, labels, pc: int):
    """The mean score of PC ``pc`` per group of ``labels``: ``[(name, mean, members)]`` by descending mean."""
    labels = np.asarray([str(x) for x in labels])
    v = res.eigenvectors[:, pc]
    out = [(g, float(v[labels == g].mean()), int((labels == g).sum())) for g in sorted(set(labels.tolist()))]
    return sorted(out, key=lambda t: -t[1])


def log_results(results: Sequence[ResidPcaResult], labels: Sequence, logger=log, warn: float = WARN) -> None:
    """Per K the summary line and one line per PC (eigenvalue, ratio to the edge); for every PC whose ratio exceeds ``warn`` a warning
    with the way to read it, the two groups with the most positive and the most negative mean score (``labels[h]``: one group name
    per sample for result h) and the five samples with the largest |entry|."""
    for res, lab in zip(results, labels):
        K = res.K
        logger.info(f"Residual PCA (K={K}): {res.N_eff} samples x {res.M_eff} SNPs with an included call, mean residual variance "
                    f"{res.total / res.N_eff:.4f} (the model expects 1), Marchenko-Pastur edge {res.edge:.6g}.")
        for k, (v, r) in enumerate(zip(res.eigenvalues, res.ratio), start=1):
            logger.info(f"      PC{k}: eigenvalue {v:.6g}, {r:.3f} x the edge")
        for k, r in enumerate(res.ratio):
            if not r > warn:
                continue
            logger.info(f"    Warning (K={K}): residual PC{k + 1} is {r:.2f} x the edge (above {warn:g}): structure the {K} components do not "
                        f"describe.  Try K = {K + 1}, and look at the 'fit' mode for the samples below.")
            g = _groups(res, lab, k)
            hi, lo = g[0], g[-1]
            logger.info(f"      groups at the two ends of PC{k + 1}: {hi[0]} (mean score {hi[1]:+.4f}, {hi[2]} samples) and {lo[0]} "
                        f"(mean score {lo[1]:+.4f}, {lo[2]} samples)")
            v = res.eigenvectors[:, k]
            top = np.argsort(-np.abs(v), kind="stable")[:5]
            logger.info(f"      samples with the largest |score| on PC{k + 1} (0-based index: score): " +
                        ", ".join(f"{int(i)}: {v[i]:+.4f}" for i in top))


def write_results(save_dir, name: str, results: Sequence[ResidPcaResult]) -> None:
    """Per head ``{save_dir}/{name}.{K}.resid.eigenval`` and ``.resid.eigenvec`` in ``pca.write_result``'s layout (17 digits)."""
    import os
    os.makedirs(save_dir, exist_ok=True)
    for r in results:
        _pca.write_result(os.path.join(save_dir, f"{name}.{r.K}.resid"), r)
