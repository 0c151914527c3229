"""Admixture dating: the decay of weighted admixture LD with genetic distance, fitted for the number of generations since admixture.

The covariance of the genotypes at two SNPs, weighted at each SNP by the allele-frequency difference of the two sources, decays as
``exp(-n d)`` with the genetic distance ``d`` (in Morgans) for an admixture ``n`` generations ago (ROLLOFF, Moorjani et al. 2011;
ALDER, Loh et al. 2013).  The run's own ``.P`` columns are the source frequencies: the curve of the components ``(a, b)`` weights
SNP ``j`` with ``P[j, a] - P[j, b]``.

``nadm_wld`` (include/nadm.h) sums the statistic over EVERY pair of SNPs within reach on the matrix pipe, exactly and with missing
calls handled pair by pair (the CPU tools approximate the sum with an FFT, which cannot do that): per pair the unbiased covariance
over the jointly observed samples, times the two weights, rounded to a 2^-32 fixed-point integer and added into the bin of the pair's
distance.  Integer sums: the same inputs give the same bits.

    grid_cells         genetic map -> the grid position of every SNP (with a gap between chromosomes) and the chromosome ranges
    component_weights  P, component pairs -> the weights, one curve per pair
    wld_curves         the sums and pair counts per chromosome, curve and bin (``nadm_wld``, one call per chromosome)
    fit_decay          y = A exp(-n d / 100) + c over dmin <= d < dmax, least squares weighted with the pair counts
    date_from_curves   the fit on all chromosomes and the leave-one-chromosome-out weighted block jackknife (ALDER's scheme: a
                       chromosome weighs its pair count) of n, A and c; z = A / se(A)
    admix_date         all of it for one sample group

A pair of SNPs goes to the bin ``cell[b] - cell[a]`` where ``cell = floor(position / binsize)`` counted from the chromosome's first
SNP: bin ``k`` holds distances in ``((k - 1) binsize, (k + 1) binsize)`` and is given the distance ``k binsize`` (ALDER grids the
map the same way).  The defaults -- ``binsize`` 0.05 cM, ``dmin`` 0.5 cM (background LD inside the sources sits below that),
``maxdist`` 20 cM -- are ALDER's conventions, not calibrations.  Calibration of the procedure on simulated panels: DESIGN.md
section 4.21.  The fit is numpy float64 on the host throughout.

Not built: multi-GPU, ALDER's one-reference and two-reference tests and its bounds on the mixture fraction, multiple-pulse fits.
"""
from __future__ import annotations

import logging
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, n_rows, stream

MAX_CURVES = 32              # NADM_WLD_MAX_CURVES
MAX_BINS = 4096              # NADM_WLD_MAX_BINS
MAX_SPAN = 65536             # NADM_WLD_MAX_SPAN
MAX_PAIRS_PER_BIN = 1 << 29  # what one nadm_wld call may add to a bin (include/nadm.h: |q| <= 2^33)
SCALE = 4294967296.0         # 2^32: a sum is in units of 2^-32
BINSIZE, DMIN, MAXDIST, MIN_SHARE = 0.05, 0.5, 20.0, 0.05
N_GRID = np.exp(np.linspace(0.0, math.log(1000.0), 241))     # the fixed log grid of the search over n: 1 .. 1000 generations
GOLDEN_STEPS = 100

log = logging.getLogger(__name__)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def chrom_ranges_of(chrom) -> list:
    """The runs of equal labels of ``chrom [M]`` as ``[(m0, m1), ...]``."""
    ch = np.asarray(chrom)
    if ch.ndim != 1 or len(ch) < 1:
        raise RuntimeError("chrom must hold one label per SNP")
    cuts = np.nonzero(ch[1:] != ch[:-1])[0] + 1
    edges = [0, *cuts.tolist(), len(ch)]
    return list(zip(edges[:-1], edges[1:]))


def grid_cells(cm, chrom, binsize: float, nbins: int):
    """``cm [M]`` (genetic positions in cM) and ``chrom [M]`` (one label per SNP, a chromosome's SNPs in one run) -> ``(cell, ranges)``:
    ``cell`` int32 ``[M]``, ``floor((cm - cm[first SNP of the chromosome]) / binsize)`` plus an offset that leaves more than ``nbins``
    cells between one chromosome's last SNP and the next one's first, and the chromosome ranges ``[(m0, m1), ...]``.  A map that
    decreases within a chromosome is refused, naming the first SNP that does."""
    cm = np.asarray(cm, dtype=np.float64)
    binsize, nbins = float(binsize), int(nbins)
    if cm.ndim != 1 or len(cm) != len(np.asarray(chrom)):
        raise RuntimeError("grid_cells: cm and chrom must hold one entry per SNP")
    if not binsize > 0.0 or nbins < 1:
        raise RuntimeError("grid_cells: binsize must be > 0 and nbins >= 1")
    if not np.all(np.isfinite(cm)):
        raise RuntimeError("grid_cells: the genetic map holds a value that is not a number")
    ranges = chrom_ranges_of(chrom)
    cell = np.empty(len(cm), dtype=np.int64)
    offset = 0
    for m0, m1 in ranges:
        seg = cm[m0:m1]
        down = np.nonzero(seg[1:] < seg[:-1])[0]
        if len(down):
            j = m0 + int(down[0]) + 1
            raise RuntimeError(f"grid_cells: the genetic map decreases within a chromosome at SNP {j} ({seg[j - m0]:g} cM after "
                               f"{seg[j - m0 - 1]:g} cM); sort the map or fix it")
        c = np.floor((seg - seg[0]) / binsize).astype(np.int64) + offset
        cell[m0:m1] = c
        offset = int(c[-1]) + nbins + 1
    if offset >= (1 << 31):
        raise RuntimeError("grid_cells: the map needs more than 2^31 grid cells; use a larger bin")
    return cell.astype(np.int32), ranges


def reach(cell, nbins: int, ranges) -> int:
    """The smallest ``W`` such that every pair ``a < b`` of one range with ``cell[b] - cell[a] < nbins`` has ``b - a <= W`` (at least 1)."""
    cell = np.asarray(cell, dtype=np.int64)
    W = 1
    for m0, m1 in ranges:
        seg = cell[m0:m1]
        last = np.searchsorted(seg, seg + int(nbins), side="left") - 1          # the last SNP fewer than nbins cells on
        W = max(W, int((last - np.arange(len(seg))).max()))
    return W


def component_weights(P, pairs) -> np.ndarray:
    """``P [M, K]`` and the component pairs ``[(a, b), ...]`` (0-based) -> float64 ``[len(pairs), M]``: row i is ``P[:, a] - P[:, b]``
    of pair i, the difference taken in float64."""
    Pn = np.asarray(P.detach().cpu() if torch.is_tensor(P) else P, dtype=np.float64)
    if Pn.ndim != 2:
        raise RuntimeError("component_weights: P must be a matrix [M, K]")
    K = Pn.shape[1]
    out = np.empty((len(pairs), Pn.shape[0]), dtype=np.float64)
    for i, (a, b) in enumerate(pairs):
        if not (0 <= int(a) < K and 0 <= int(b) < K) or int(a) == int(b):
            raise RuntimeError(f"component_weights: a pair must name two different components in 0..{K - 1}, got {a}-{b}")
        out[i] = Pn[:, int(a)] - Pn[:, int(b)]
    return out


# ---- the curves -------------------------------------------------------------------------------------------------------------------
def wld_curves(xp: torch.Tensor, M: int, cell, wt, nbins: int, idx: Optional[torch.Tensor] = None, chrom_ranges=None, nmin: int = 2):
    """The weighted-LD sums of the packed device matrix ``xp [rows, ld]`` over the rows ``idx`` (int32, default: every row):
    ``(sum, cnt)`` on the host, int64 ``[chrom, C, nbins]`` and ``[chrom, nbins]`` -- per chromosome range of ``chrom_ranges``
    (default: one range, all SNPs), curve of ``wt [C, M]`` (float64, |wt| <= 1) and bin ``cell[b] - cell[a] < nbins``, the sum of
    ``llrint(cov(a, b) wt[a] wt[b] 2^32)`` over the pairs with at least ``nmin`` jointly observed samples, and the number of those
    pairs (include/nadm.h, nadm_wld: exact integers, the same bits every time).  ``cell``: int32 ``[M]``, nondecreasing
    (``grid_cells``).  One call per chromosome and group of 32 curves."""
    rows = n_rows(xp, idx)
    check_packed(xp, idx, rows, "wld_curves")
    M, nbins, nmin = int(M), int(nbins), int(nmin)
    if M < 1 or M > 4 * int(xp.shape[1]):
        raise RuntimeError(f"wld_curves: M must be in 1..{4 * int(xp.shape[1])} for rows of {int(xp.shape[1])} bytes")
    if rows < 2:
        raise RuntimeError("wld_curves: a covariance needs at least 2 samples")
    if not 1 <= nbins <= MAX_BINS:
        raise RuntimeError(f"wld_curves: nbins must be in 1..{MAX_BINS}; use a larger bin or a smaller --maxdist")
    if nmin < 2:
        raise RuntimeError("wld_curves: nmin must be >= 2")
    if idx is not None and rows > 0 and (int(idx.min()) < 0 or int(idx.max()) >= int(xp.shape[0])):
        raise RuntimeError("wld_curves: idx names a row the packed matrix does not have")
    cell_h = np.ascontiguousarray(np.asarray(cell.cpu() if torch.is_tensor(cell) else cell))
    if cell_h.shape != (M,) or not np.issubdtype(cell_h.dtype, np.integer):
        raise RuntimeError(f"wld_curves: cell must hold one integer per SNP ({M})")
    if int(cell_h.min()) < 0 or int(cell_h.max()) >= (1 << 31) or np.any(cell_h[1:] < cell_h[:-1]):
        raise RuntimeError("wld_curves: cell must be nondecreasing with values in 0..2^31 - 1")
    wt_h = np.asarray(wt.detach().cpu() if torch.is_tensor(wt) else wt, dtype=np.float64)
    if wt_h.ndim != 2 or wt_h.shape[1] != M or wt_h.shape[0] < 1:
        raise RuntimeError(f"wld_curves: wt must be [C, {M}] with C >= 1")
    if not np.all(np.abs(wt_h) <= 1.0):                     # (a NaN fails this too)
        raise RuntimeError("wld_curves: every weight must be in [-1, 1] (the overflow bound of the integer sums rests on it)")
    ranges = [(0, M)] if chrom_ranges is None else [(int(a), int(b)) for a, b in chrom_ranges]
    for m0, m1 in ranges:
        if not 0 <= m0 < m1 <= M:
            raise RuntimeError(f"wld_curves: a chromosome range must satisfy 0 <= m0 < m1 <= M, got ({m0}, {m1})")
    W = reach(cell_h, nbins, ranges)
    if W > MAX_SPAN:
        raise RuntimeError(f"wld_curves: {nbins} bins reach {W} SNPs ahead, more than {MAX_SPAN}: use a larger bin or a smaller --maxdist")
    C_all, dev = wt_h.shape[0], xp.device
    out_sum = np.zeros((len(ranges), C_all, nbins), dtype=np.int64)
    out_cnt = np.zeros((len(ranges), nbins), dtype=np.int64)
    with torch.cuda.device(dev):
        cell_d = torch.from_numpy(cell_h.astype(np.int32)).to(dev)
        for c0 in range(0, C_all, MAX_CURVES):
            C = min(MAX_CURVES, C_all - c0)
            wt_d = torch.from_numpy(np.ascontiguousarray(wt_h[c0:c0 + C])).to(dev)
            s_d = torch.empty((len(ranges), C, nbins), dtype=torch.int64, device=dev)
            n_d = torch.empty((len(ranges), nbins), dtype=torch.int64, device=dev)
            for r, (m0, m1) in enumerate(ranges):
                check(lib.nadm_wld(ptr(xp), xp.shape[1], ptr(idx), rows, M, m0, m1, W, ptr(cell_d), ptr(wt_d), C, nbins, nmin,
                                   ptr(s_d[r]), ptr(n_d[r]), stream()), "wld")
            out_sum[:, c0:c0 + C] = s_d.cpu().numpy()        # (the copy waits for the stream: the operands above may go after it)
            out_cnt[:] = n_d.cpu().numpy()
    if int(out_cnt.max()) > MAX_PAIRS_PER_BIN:
        raise RuntimeError(f"wld_curves: a bin of one chromosome holds {int(out_cnt.max())} pairs, more than the {MAX_PAIRS_PER_BIN} the "
                           "64-bit sums are safe for; use a smaller bin")
    return out_sum, out_cnt


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def _linear_fit(n: float, d: np.ndarray, y: np.ndarray, w: np.ndarray):
    """For a fixed n: (sse, A, c) of y = A exp(-n d / 100) + c, least squares with the weights w (centred form)."""
    x = np.exp(-n * d / 100.0)
    sw = w.sum()
    xm, ym = (w * x).sum() / sw, (w * y).sum() / sw
    xc, yc = x - xm, y - ym
    sxx = (w * xc * xc).sum()
    A = (w * xc * yc).sum() / sxx if sxx > 0.0 else 0.0
    r = yc - A * xc
    return float((w * r * r).sum()), float(A), float(ym - A * xm)


def fit_decay(d, y, cnt, dmin: float, dmax: float):
    """``(n, A, c)`` of ``y = A exp(-n d / 100) + c`` (``d`` in cM, ``n`` in generations) over the bins with ``dmin <= d < dmax`` and a
    pair in them, by least squares weighted with ``cnt``.  For a fixed ``n`` the fit is linear in ``(A, c)``; ``n`` is searched on a
    fixed log grid over 1..1000 generations and refined by golden section between the grid neighbours of the best point.  numpy
    float64.  Fewer than 3 usable bins: ``(nan, nan, nan)``."""
    d, y, w = (np.asarray(v, dtype=np.float64) for v in (d, y, cnt))
    use = (d >= float(dmin)) & (d < float(dmax)) & (w > 0) & np.isfinite(y)
    d, y, w = d[use], y[use], w[use]
    if len(d) < 3:
        return float("nan"), float("nan"), float("nan")
    sse = np.array([_linear_fit(n, d, y, w)[0] for n in N_GRID])
    i = int(np.argmin(sse))
    lo, hi = math.log(N_GRID[max(i - 1, 0)]), math.log(N_GRID[min(i + 1, len(N_GRID) - 1)])
    g = (math.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = _linear_fit(math.exp(x1), d, y, w)[0], _linear_fit(math.exp(x2), d, y, w)[0]
    for _ in range(GOLDEN_STEPS):
        if f1 <= f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo)
            f1 = _linear_fit(math.exp(x1), d, y, w)[0]
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo)
            f2 = _linear_fit(math.exp(x2), d, y, w)[0]
    n = math.exp(0.5 * (lo + hi))
    _, A, c = _linear_fit(n, d, y, w)
    return n, A, c


def jackknife(full, leave_out, weights):
    """The weighted block jackknife (Busing et al. 1999) of an estimate: ``full`` the estimate from all blocks, ``leave_out[j]`` the one
    without block j, ``weights[j]`` block j's weight.  Returns the standard error; NaN with fewer than 2 blocks."""
    th, m = np.asarray(leave_out, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    g = len(th)
    if g < 2 or not np.all(m > 0) or not np.all(np.isfinite(th)):
        return float("nan")
    h = m.sum() / m
    tj = g * full - ((1.0 - m / m.sum()) * th).sum()
    tau = h * full - (h - 1.0) * th
    return float(math.sqrt(((tau - tj) ** 2 / (h - 1.0)).sum() / g))


class DateResult(NamedTuple):
    """One curve: the components ``a, b`` (0-based), ``generations`` and its jackknife ``se``, the amplitude ``A`` with ``se_A``, the
    offset ``c`` with ``se_c``, and ``z = A / se_A`` (NaN standard errors with fewer than 2 chromosomes)."""
    a: int
    b: int
    generations: float
    se: float
    A: float
    se_A: float
    c: float
    se_c: float
    z: float


class DateCurves(NamedTuple):
    """What ``admix_date`` returns: ``results`` one ``DateResult`` per curve, ``d`` float64 ``[nbins]`` the bins' distances in cM,
    ``pairs`` int64 ``[nbins]`` the pairs per bin over all chromosomes, ``y`` float64 ``[C, nbins]`` the mean weighted covariance per
    bin (NaN for an empty bin), and the integer ``sum [chrom, C, nbins]`` / ``cnt [chrom, nbins]`` they come from."""
    results: list
    d: np.ndarray
    pairs: np.ndarray
    y: np.ndarray
    sum: np.ndarray
    cnt: np.ndarray


def _mean_curve(s: np.ndarray, n: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s.astype(np.float64) / n.astype(np.float64) / SCALE, np.nan)


def date_from_curves(sum_, cnt, binsize: float, dmin: float, dmax: float, pairs=None) -> DateCurves:
    """The fit of every curve of ``wld_curves``' ``(sum [chrom, C, nbins], cnt [chrom, nbins])`` on all chromosomes together, and the
    leave-one-chromosome-out weighted block jackknife of n, A and c, a chromosome weighing its pairs in the fitted bins."""
    sum_, cnt = np.asarray(sum_, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    G, C, nbins = sum_.shape
    d = np.arange(nbins, dtype=np.float64) * float(binsize)
    s_all, n_all = sum_.sum(axis=0), cnt.sum(axis=0)
    fitted = (d >= float(dmin)) & (d < float(dmax))
    weights = cnt[:, fitted].sum(axis=1)
    ok = weights > 0
    y = np.stack([_mean_curve(s_all[c], n_all) for c in range(C)])
    results = []
    for c in range(C):
        full = fit_decay(d, y[c], n_all, dmin, dmax)
        ses = [float("nan")] * 3
        if int(ok.sum()) >= 2:
            loo = [fit_decay(d, _mean_curve(s_all[c] - sum_[j, c], n_all - cnt[j]), n_all - cnt[j], dmin, dmax)
                   for j in range(G) if ok[j]]
            ses = [jackknife(full[k], [v[k] for v in loo], weights[ok]) for k in range(3)]
        a, b = pairs[c] if pairs is not None else (-1, -1)
        z = full[1] / ses[1] if ses[1] == ses[1] and ses[1] > 0.0 else float("nan")
        results.append(DateResult(int(a), int(b), full[0], ses[0], full[1], ses[1], full[2], ses[2], z))
    return DateCurves(results, d, n_all, y, sum_, cnt)


def choose_pairs(Q, min_share: float = MIN_SHARE) -> list:
    """The component pairs ``a < b`` whose two mean shares over the rows of ``Q [b, K]`` are both at least ``min_share``."""
    Qn = np.asarray(Q.detach().cpu() if torch.is_tensor(Q) else Q, dtype=np.float64)
    share = Qn.mean(axis=0)
    K = len(share)
    return [(a, b) for a in range(K) for b in range(a + 1, K) if share[a] >= min_share and share[b] >= min_share]


def check_args(binsize: float, dmin: float, maxdist: float, min_share: float = MIN_SHARE) -> int:
    """Refuses, in words, what no run can use; returns ``nbins = ceil(maxdist / binsize)``."""
    if not binsize > 0.0:
        raise RuntimeError("--binsize must be > 0 (cM)")
    if not 0.0 <= dmin < maxdist:
        raise RuntimeError("--mindist must be >= 0 and below --maxdist (cM)")
    if not 0.0 <= min_share <= 0.5:
        raise RuntimeError("--min_share must be in [0, 0.5]")
    nbins = int(math.ceil(maxdist / binsize - 1e-9))
    if nbins > MAX_BINS:
        raise RuntimeError(f"--maxdist / --binsize gives {nbins} bins, more than {MAX_BINS}: use a larger bin or a smaller --maxdist")
    if nbins < 3:
        raise RuntimeError("--maxdist / --binsize gives fewer than 3 bins: nothing to fit")
    return nbins


def admix_date(xp: torch.Tensor, M: int, P, Q, cm, chrom, idx: Optional[torch.Tensor] = None, pairs: Optional[Sequence] = None,
               binsize: float = BINSIZE, dmin: float = DMIN, maxdist: float = MAXDIST, min_share: float = MIN_SHARE,
               nmin: int = 2) -> DateCurves:
    """Dates the admixture of ONE sample group -- the rows ``idx`` (int32, default: every row) of the packed device matrix
    ``xp [rows, ld]`` -- from the decay of its weighted LD: the curves of the component pairs ``pairs`` (default: ``choose_pairs`` on
    the group's rows of ``Q``, which are ``Q``'s rows in the order of ``idx``) weighted with the columns of ``P [M, K]``, binned
    on the genetic map ``cm [M]`` (cM) per chromosome ``chrom [M]``, fitted over ``dmin <= d < maxdist`` and jackknifed over the
    chromosomes (``date_from_curves``).  Fewer than 2 chromosomes: NaN standard errors and a warning."""
    nbins = check_args(binsize, dmin, maxdist, min_share)
    M = int(M)
    if np.ndim(P) != 2 or int(np.shape(P)[0]) != M:
        raise RuntimeError(f"admix_date: P must be [M, K] with M = {M}")
    if np.ndim(Q) != 2 or int(np.shape(Q)[0]) != n_rows(xp, idx) or int(np.shape(Q)[1]) != int(np.shape(P)[1]):
        raise RuntimeError(f"admix_date: Q must hold one row of {int(np.shape(P)[1])} fractions per sample of the group ({n_rows(xp, idx)})")
    pairs = choose_pairs(Q, min_share) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise RuntimeError(f"admix_date: no two components have a mean share of at least {min_share:g} in the group: nothing to date "
                           "(name the pairs, or lower --min_share)")
    wt = component_weights(P, pairs)
    cell, ranges = grid_cells(cm, chrom, binsize, nbins)
    if len(ranges) < 2:
        log.warning("    Warning: the panel holds fewer than 2 chromosomes; the jackknife needs 2: the standard errors are nan.")
    s, n = wld_curves(xp, M, cell, wt, nbins, idx=idx, chrom_ranges=ranges, nmin=nmin)
    return date_from_curves(s, n, binsize, dmin, maxdist, pairs)


# ---- the command line's side ------------------------------------------------------------------------------------------------------
def log_results(res: DateCurves, k: int, logger) -> None:
    for r in res.results:
        logger.info(f"    Admixture date (K={k}, components {r.a + 1}-{r.b + 1}): {r.generations:.2f} +- {r.se:.2f} generations; "
                    f"amplitude {r.A:.3e} +- {r.se_A:.3e} (z = {r.z:.2f}), offset {r.c:.3e}.")
        if not abs(r.z) >= 2.0:
            logger.info(f"    Warning: the components {r.a + 1}-{r.b + 1} show no admixture LD (|z| < 2, or no standard error): "
                        "their date means nothing.")


def write_results(save_dir: str, name: str, k: int, res: DateCurves) -> None:
    """``{name}.{k}.wld``: a header, then one row per bin, ``d_cM pairs`` and one column per curve; ``{name}.{k}.date``: a header, then
    one row per curve, ``a b generations se A se_A c z`` (components 1-based)."""
    import os
    stem = os.path.join(save_dir, f"{name}.{k}")
    with open(f"{stem}.wld", "w") as fb:
        fb.write(" ".join(["d_cM", "pairs"] + [f"{r.a + 1}-{r.b + 1}" for r in res.results]) + "\n")
        for i in range(len(res.d)):
            fb.write(" ".join([f"{res.d[i]:.6g}", str(int(res.pairs[i]))] + [f"{res.y[c, i]:.9e}" for c in range(len(res.results))]) + "\n")
    with open(f"{stem}.date", "w") as fb:
        fb.write("a b generations se A se_A c z\n")
        for r in res.results:
            fb.write(f"{r.a + 1} {r.b + 1} {r.generations:.6g} {r.se:.6g} {r.A:.9e} {r.se_A:.9e} {r.c:.9e} {r.z:.6g}\n")
