"""Cross-validation error for choosing K, over held-out genotype CALLS (what ADMIXTURE's ``--cv`` does): hide a random fold of the
observed calls, refit on the rest, score how well the refit predicts the hidden calls by the binomial deviance; the K with the
lowest error per held-out call is the one to take.  The in-sample log-likelihood cannot choose K: it improves with every K.

The fold of a call is a fixed function of (seed, matrix row, SNP) that include/nadm.h states.  ``mask_fold`` is one ``nadm_cv_mask``
call: a copy of the packed matrix with one fold's observed calls turned into missing ones, on which the masked EM of project.py runs
unchanged.  ``heldout_deviance`` is one ``nadm_cv_deviance`` call on the ORIGINAL matrix (reproducible bit for bit).  ``cv_error``
is the driver: per fold one masked copy (the one extra matrix-sized buffer, reused), one ``project.polish`` of all heads from the
given answer, one deviance pass per head.

The refit starts from the full-data answer, which has seen the held-out calls: stopped early it LEAKS, and the error of a K that
is too large comes out too low.  So the round limit defaults high, ``tol`` stops a refit that has converged, and
``CvResult.hit_limit`` says when the limit and not ``tol`` ended a refit: that K's error is then optimistic.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, model_operands, stream
from . import project

MAX_FOLDS = 64       # NADM_CV_MAX_FOLDS
COUNT_ROWS = 1 << 24  # rows per nadm_snp_counts call at most


class CvResult(NamedTuple):
    """One head's cross-validation error: ``error`` = the held-out deviance summed over folds and SNPs / the number of held-out
    calls; ``se`` = the standard deviation of the per-fold errors (n - 1 in the denominator) / sqrt(folds); ``per_fold`` the folds'
    own errors; ``n_held`` the held-out calls over all folds (= the observed calls of the matrix); ``rounds_run`` the refit's rounds
    per fold; ``hit_limit``: a fold's refit ran all its ``rounds`` (a refit that met ``tol`` in its very last round counts too: the
    two cannot be told apart, and the warning is the safe side)."""
    k: int
    error: float
    se: float
    per_fold: List[float]
    n_held: int
    rounds_run: List[int]
    hit_limit: bool


def _fold_args(fold: int, folds: int, seed: int, row0: int):
    fold, folds, seed, row0 = int(fold), int(folds), int(seed), int(row0)
    if not 2 <= folds <= MAX_FOLDS:
        raise RuntimeError(f"folds must be in 2..{MAX_FOLDS}")
    if not 0 <= fold < folds:
        raise RuntimeError(f"fold must be in 0..{folds - 1}")
    if not 0 <= seed < 1 << 64:
        raise RuntimeError("seed must be in 0..2^64-1")
    if row0 < 0:
        raise RuntimeError("row0 must be >= 0")
    return fold, folds, seed, row0


def mask_fold(xp: torch.Tensor, M: int, fold: int, folds: int, seed: int, out: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """One ``nadm_cv_mask`` call on the current stream: the packed device matrix ``xp [rows, ld]`` with every OBSERVED call of fold
    ``fold`` (of ``folds``, drawn with ``seed``) turned into a missing one, every other bit as it is.  ``out``: where to write
    (same shape; ``xp`` itself: in place; default: a new matrix); ``row0``: the index of xp's first row in the whole matrix."""
    fold, folds, seed, row0 = _fold_args(fold, folds, seed, row0)
    check_packed(xp, None, int(xp.shape[0]))
    if out is None:
        out = torch.empty_like(xp)
    elif out.shape != xp.shape or out.dtype != torch.uint8 or out.device != xp.device or not out.is_contiguous():
        raise RuntimeError("mask_fold: out must be a contiguous uint8 matrix of xp's shape on xp's device")
    check(lib.nadm_cv_mask(ptr(xp), xp.shape[1], xp.shape[0], row0, int(M), seed, folds, fold, ptr(out), stream()), "cv_mask")
    return out


def heldout_deviance(xp: torch.Tensor, M: int, P, Q, fold: int, folds: int, seed: int, eps: float = project.EPS, row0: int = 0):
    """One ``nadm_cv_deviance`` call on the current stream: the binomial deviance of the observed calls of fold ``fold`` in the
    ORIGINAL packed device matrix ``xp [rows, ld]`` under ``pi = Q P^T`` (``P [M, K]``, ``Q [rows, K]``, host or device), per SNP.
    Returns ``(dev float64 [M], nheld int32 [M])`` on xp's device.  ``row0``: the index of xp's first row in the whole matrix."""
    fold, folds, seed, row0 = _fold_args(fold, folds, seed, row0)
    M = int(M)
    b, K, Pp, Qp = model_operands(xp, M, None, P, Q)
    n_scr = int(lib.nadm_cv_deviance_scratch_floats(b, M))
    if n_scr <= 0:
        raise RuntimeError(f"heldout_deviance: a block of {b} rows over {M} SNPs is not supported")
    dev_ = xp.device
    scratch = torch.empty(n_scr, dtype=torch.float32, device=dev_)
    dev = torch.empty(M, dtype=torch.float64, device=dev_)
    nheld = torch.empty(M, dtype=torch.int32, device=dev_)
    check(lib.nadm_cv_deviance(ptr(xp), xp.shape[1], b, row0, M, ptr(Qp), Qp.stride(0), K, Pp.shape[1], ptr(Pp), float(eps), seed, folds,
                               fold, ptr(dev), ptr(nheld), ptr(scratch), stream()), "cv_deviance")
    return dev, nheld


def _observed_calls(xp: torch.Tensor, M: int) -> int:
    from .ld import snp_counts
    N = int(xp.shape[0])
    return sum(int(snp_counts(xp[s:s + COUNT_ROWS], M)[:, 0].sum(dtype=torch.int64)) for s in range(0, N, COUNT_ROWS))


def cv_error(xp: torch.Tensor, M: int, Ps: Sequence, Qs: Sequence, folds: int = 5, rounds: int = 50, tol: float = 1e-5,
             seed: int = 0) -> List[CvResult]:
    """The cross-validation error of every head ``(Ps[h] [M, k_h], Qs[h] [N, k_h])`` (host or device, not modified) on the packed
    device matrix ``xp [N, ld]``: per fold ``f`` the fold's observed calls are hidden (``mask_fold``), all heads are refitted on
    the rest from the GIVEN answer (``project.polish(xo, M, Ps, Qs, rounds, tol)``), and the hidden calls of ``xp`` are scored at
    each head's refit (``heldout_deviance``).  Every observed call is held out exactly once.  One ``CvResult`` per head."""
    folds, rounds, M = int(folds), int(rounds), int(M)
    _fold_args(0, folds, seed, 0)
    if rounds < 1:
        raise RuntimeError("rounds must be >= 1")
    if len(Ps) != len(Qs) or not Ps:
        raise RuntimeError("cv_error needs one P and one Q per head")
    H = len(Ps)
    dev = np.zeros((H, folds))
    held = np.zeros((H, folds), dtype=np.int64)
    ran: List[int] = []
    xo = None
    for f in range(folds):
        xo = mask_fold(xp, M, f, folds, seed, out=xo)
        Pf, Qf, _, _, done = project.polish(xo, M, Ps, Qs, rounds, tol)
        ran.append(int(done))
        for h in range(H):
            d, n = heldout_deviance(xp, M, Pf[h], Qf[h], f, folds, seed)
            dev[h, f], held[h, f] = float(d.sum()), int(n.sum(dtype=torch.int64))
    del xo
    n_obs = _observed_calls(xp, M)
    out = []
    for h in range(H):
        assert int(held[h].sum()) == n_obs, f"cv_error: {int(held[h].sum())} calls were held out, the matrix has {n_obs} observed ones"
        with np.errstate(divide="ignore", invalid="ignore"):
            per = dev[h] / held[h]
            err = float(dev[h].sum() / held[h].sum())
        se = float(np.std(per, ddof=1) / math.sqrt(folds))
        out.append(CvResult(int(np.shape(Ps[h])[1]), err, se, [float(x) for x in per], int(held[h].sum()), list(ran),
                            any(r >= rounds for r in ran)))
    return out


def best_k(results: Sequence[CvResult]) -> int:
    """The K with the lowest cross-validation error (the smaller K on a tie)."""
    return min(results, key=lambda r: (r.error, r.k)).k


def log_results(results: Sequence[CvResult], log) -> None:
    """One line per K in ADMIXTURE's own wording (``CV error (K=3): 1.10931``: a ``grep "CV error"`` keeps working), the K with the
    lowest error, and a warning that names --cv_rounds for every K whose refit ran into the round limit."""
    for r in results:
        log.info(f"CV error (K={r.k}): {r.error:.5f}")
    if len(results) > 1:
        log.info(f"    Lowest cross-validation error: K = {best_k(results)}.")
    late = [r for r in results if r.hit_limit]
    if late:
        log.info(f"    Warning: the refit for K = {', '.join(str(r.k) for r in late)} stopped at the limit of {max(late[0].rounds_run)} "
                 "rounds, not at the tolerance; such a CV error is optimistic (the start has seen the held-out calls): raise --cv_rounds.")


def write_table(path, results: Sequence[CvResult]) -> None:
    """One line ``K cv_error se n_heldout rounds`` per head in the order given: floats with the 17 digits that read back to the same
    float64, ``rounds`` the largest count over the folds."""
    with open(path, "w") as fb:
        for r in results:
            fb.write("{:d} {:.17g} {:.17g} {:d} {:d}\n".format(r.k, r.error, r.se, r.n_held, max(r.rounds_run)))
