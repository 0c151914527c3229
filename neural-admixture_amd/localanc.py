"""Local ancestry: which stretches of each genome come from which component.

The linkage model of STRUCTURE (Falush, Stephens & Pritchard 2003), unphased as in ancestry_HMM (Corbett-Detig & Nielsen 2017): each
of a sample's two haplotypes carries an ancestry that is redrawn from the sample's row of ``Q`` at rate ``n`` per Morgan (``n``
generations since a single pulse, ONE rate for all components), and the unphased call is emitted from the two ancestries' columns
of ``P``.  ``nadm_local_anc`` (include/nadm.h) runs the forward-backward recursion over the K (K + 1) / 2 unordered ancestry pairs on
the packed matrix already in HBM, a lane per sample, and returns the posterior at the output points.

    switch_prob        genetic map, generations -> rho [M], the redraw probability between neighbouring SNPs, and the segments
    output_points      genetic map, grid -> the SNPs at which the posterior is written, per chromosome
    check_layout       the host-side checks of seg / out_snp / oseg that the library cannot make on the device
    local_ancestry     dosage, call, posterior and log-likelihood for the rows of one group, in row blocks of bounded scratch
    loglik             the forward pass alone
    scan_generations   the number of generations that maximises the log-likelihood: a fixed log grid, then golden section
    tracts             switches and mean tract length per sample from the calls

The output grid (``GRID`` = 0.5 cM: about ten points per mean tract of 100 / n cM at 20 generations) is a convention, not a
calibration.  The model has NO description of LD inside a source: strongly linked SNPs are counted as independent evidence and make
the posterior over-confident -- ``prune`` first and pass the list with ``--extract``.  Calibration on simulated panels: DESIGN.md
section 4.22.

Not built: phased input, per-component rates, multiple pulses, Viterbi paths, a ``train`` option, multi-GPU.
"""
from __future__ import annotations

import logging
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import model_operands, n_rows, stream
from .admixdate import chrom_ranges_of

MAX_K = 16
TOO_WIDE = "local ancestry is available for K <= 16 (the K (K + 1) / 2 states of a sample live in one thread's registers)"
EPS = 1e-6
GRID = 0.5                    # cM between output points
SCRATCH_BUDGET = 1 << 30      # bytes of checkpoints per row block
SCAN_SAMPLES = 512
N_GRID = np.exp(np.linspace(0.0, math.log(1000.0), 61))      # the fixed log grid of the search over n: 1 .. 1000 generations
GOLDEN_STEPS = 40
WARN_SPREAD = 4.0

log = logging.getLogger(__name__)


def n_pairs(k: int) -> int:
    return k * (k + 1) // 2


def pair_table(k: int) -> list:
    """The unordered ancestry pairs in the order of ``call``: a-major over a <= b < k."""
    return [(a, b) for a in range(k) for b in range(a, k)]


# ---- the map's side ---------------------------------------------------------------------------------------------------------------
def _map_ranges(cm, chrom, who: str):
    cm = np.asarray(cm, dtype=np.float64)
    if cm.ndim != 1 or len(cm) != len(np.asarray(chrom)):
        raise RuntimeError(f"{who}: cm and chrom must hold one entry per SNP")
    if not np.all(np.isfinite(cm)):
        raise RuntimeError(f"{who}: the genetic map holds a value that is not a number")
    ranges = chrom_ranges_of(chrom)
    for m0, m1 in ranges:
        seg = cm[m0:m1]
        down = np.nonzero(seg[1:] < seg[:-1])[0]
        if len(down):
            j = m0 + int(down[0]) + 1
            raise RuntimeError(f"{who}: the genetic map decreases within a chromosome at SNP {j} ({seg[j - m0]:g} cM after "
                               f"{seg[j - m0 - 1]:g} cM); sort the map or fix it")
    return cm, ranges


def switch_prob(cm, chrom, generations: float):
    """``cm [M]`` (cM), ``chrom [M]`` (a chromosome's SNPs in one run) and the number of generations ``n`` -> ``(rho, ranges)``: ``rho``
    float32 ``[M]``, ``1 - exp(-n d / 100)`` of the distance ``d`` to the SNP before in float64, rounded to fp32 once, and exactly 1 at
    every chromosome's first SNP; ``ranges`` the chromosomes ``[(m0, m1), ...]``.  A map that decreases within a chromosome is refused,
    naming the first SNP that does."""
    n = float(generations)
    if not (n > 0.0 and math.isfinite(n)):
        raise RuntimeError("switch_prob: generations must be > 0")
    cm, ranges = _map_ranges(cm, chrom, "switch_prob")
    rho = np.ones(len(cm), dtype=np.float64)
    for m0, m1 in ranges:
        rho[m0 + 1:m1] = -np.expm1(-n * np.diff(cm[m0:m1]) / 100.0)
    return rho.astype(np.float32), ranges


def output_points(cm, chrom, grid: float = GRID):
    """Per chromosome the first SNP at or after each multiple of ``grid`` cM counted from the chromosome's first SNP (a SNP is listed
    once): ``(out_snp int32 [n_out]`` ascending, ``oseg int32 [chromosomes + 1])``, chromosome s owning ``out_snp[oseg[s]:oseg[s + 1]]``."""
    if not float(grid) > 0.0:
        raise RuntimeError("output_points: grid must be > 0 (cM)")
    cm, ranges = _map_ranges(cm, chrom, "output_points")
    out, oseg = [], [0]
    for m0, m1 in ranges:
        rel = cm[m0:m1] - cm[m0]
        marks = np.arange(0.0, rel[-1] + 0.5 * grid, float(grid))
        at = np.unique(np.searchsorted(rel, marks, side="left"))
        out.append(m0 + at[at < m1 - m0])
        oseg.append(oseg[-1] + len(out[-1]))
    return np.concatenate(out).astype(np.int32), np.asarray(oseg, dtype=np.int32)


def check_layout(M: int, seg, out_snp=None, oseg=None):
    """What ``nadm_local_anc`` cannot check on the device, checked before the upload: ``seg`` ascending within 0..M, ``out_snp``
    strictly ascending, ``oseg`` ascending from 0 to ``len(out_snp)`` with one entry per bound of ``seg``, and every segment's slice of
    ``out_snp`` inside that segment.  Returns the three as contiguous int32 arrays (``out_snp`` / ``oseg`` None: no output points)."""
    seg = np.ascontiguousarray(np.asarray(seg, dtype=np.int64))
    if seg.ndim != 1 or len(seg) < 2:
        raise RuntimeError("local_ancestry: seg must hold the bounds of at least one segment")
    if seg[0] < 0 or seg[-1] > int(M) or np.any(seg[1:] < seg[:-1]):
        raise RuntimeError(f"local_ancestry: seg must be ascending within 0..{int(M)}")
    if out_snp is None and oseg is None:
        return seg.astype(np.int32), None, None
    if out_snp is None or oseg is None:
        raise RuntimeError("local_ancestry: out_snp and oseg go together")
    out_snp = np.ascontiguousarray(np.asarray(out_snp, dtype=np.int64))
    oseg = np.ascontiguousarray(np.asarray(oseg, dtype=np.int64))
    if out_snp.ndim != 1 or np.any(out_snp[1:] <= out_snp[:-1]):
        raise RuntimeError("local_ancestry: out_snp must be strictly ascending")
    if oseg.shape != seg.shape or oseg[0] != 0 or oseg[-1] != len(out_snp) or np.any(oseg[1:] < oseg[:-1]):
        raise RuntimeError(f"local_ancestry: oseg must ascend from 0 to {len(out_snp)} with one entry per bound of seg")
    for s in range(len(seg) - 1):
        sl = out_snp[oseg[s]:oseg[s + 1]]
        if len(sl) and (sl[0] < seg[s] or sl[-1] >= seg[s + 1]):
            raise RuntimeError(f"local_ancestry: segment {s} is [{int(seg[s])}, {int(seg[s + 1])}) but its output points run from "
                               f"{int(sl[0])} to {int(sl[-1])}")
    return seg.astype(np.int32), out_snp.astype(np.int32), oseg.astype(np.int32)


# ---- the library's side -----------------------------------------------------------------------------------------------------------
class LocalAncestry(NamedTuple):
    """What ``local_ancestry`` returns, on the host: ``call`` uint8 ``[N, points]`` (index into ``pair_table(K)``, 255 where the
    posterior is NaN), ``post`` float32 ``[N, points]`` the called pair's posterior mass, ``ll`` float64 ``[N, chromosomes]``,
    ``share`` float64 ``[N, K]`` a sample's mean local share over its finite points, ``point_share`` float64 ``[points, K]`` the mean
    share over the samples with a finite posterior there, ``nan_points`` the number of NaN (sample, point) entries, ``dosage`` float32
    ``[N, points, K]`` or None, ``out_snp`` / ``oseg`` the points, ``ranges`` the chromosomes, ``generations``."""
    call: np.ndarray
    post: np.ndarray
    ll: np.ndarray
    share: np.ndarray
    point_share: np.ndarray
    nan_points: int
    dosage: Optional[np.ndarray]
    out_snp: np.ndarray
    oseg: np.ndarray
    ranges: list
    generations: float


def _operands(xp, M, P, Q, idx, what):
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what=what)
    if K > MAX_K:
        raise RuntimeError(f"{what}: {TOO_WIDE}")
    if idx is not None and b > 0 and (int(idx.min()) < 0 or int(idx.max()) >= int(xp.shape[0])):
        raise RuntimeError(f"{what}: idx names a row the packed matrix does not have")
    if int(M) < 1 or int(M) > 4 * int(xp.shape[1]):
        raise RuntimeError(f"{what}: M must be in 1..{4 * int(xp.shape[1])} for rows of {int(xp.shape[1])} bytes")
    return b, K, Pp, Qp


def _rho_operand(rho, M, dev):
    rho = np.ascontiguousarray(np.asarray(rho, dtype=np.float32))
    if rho.shape != (int(M),) or not np.all((rho >= 0.0) & (rho <= 1.0)):          # (a NaN fails this too)
        raise RuntimeError(f"local_ancestry: rho must hold one probability in [0, 1] per SNP ({int(M)})")
    return torch.from_numpy(rho).to(dev)


def forward_backward(xp: torch.Tensor, M: int, Pp: torch.Tensor, Qp: torch.Tensor, K: int, idx: Optional[torch.Tensor], b: int,
                     rho_d: torch.Tensor, seg_d: torch.Tensor, out_d: Optional[torch.Tensor], oseg_d: Optional[torch.Tensor],
                     eps: float = EPS, full: bool = True):
    """One ``nadm_local_anc`` call on device operands that the caller has checked (``check_layout``): ``(dosage [b, n_out, kp], call,
    post, ll [b, n_seg])`` on the device; ``full`` False or no output points: the forward pass alone, ``(None, None, None, ll)``."""
    dev, kp = xp.device, int(Pp.shape[1])
    n_seg = int(seg_d.numel()) - 1
    n_out = int(out_d.numel()) if (full and out_d is not None) else 0
    with torch.cuda.device(dev):
        ll = torch.empty((b, n_seg), dtype=torch.float64, device=dev)
        if n_out == 0:
            check(lib.nadm_local_anc(ptr(xp), xp.shape[1], ptr(idx), b, int(M), ptr(Pp), K, kp, ptr(Qp), Qp.stride(0), float(eps),
                                     ptr(rho_d), ptr(seg_d), n_seg, None, None, 0, None, None, None, ptr(ll), None, stream()),
                  "local_anc")
            return None, None, None, ll
        nf = int(lib.nadm_local_anc_scratch_floats(b, n_out, kp))
        if nf <= 0:
            raise RuntimeError(f"local_ancestry: {TOO_WIDE}")
        scratch = torch.empty(nf, dtype=torch.float32, device=dev)
        dosage = torch.empty((b, n_out, kp), dtype=torch.float32, device=dev)
        call = torch.empty((b, n_out), dtype=torch.uint8, device=dev)
        post = torch.empty((b, n_out), dtype=torch.float32, device=dev)
        check(lib.nadm_local_anc(ptr(xp), xp.shape[1], ptr(idx), b, int(M), ptr(Pp), K, kp, ptr(Qp), Qp.stride(0), float(eps),
                                 ptr(rho_d), ptr(seg_d), n_seg, ptr(out_d), ptr(oseg_d), n_out, ptr(dosage), ptr(call), ptr(post),
                                 ptr(ll), ptr(scratch), stream()), "local_anc")
    return dosage, call, post, ll


def block_rows(n_out: int, K: int, budget: int = SCRATCH_BUDGET) -> int:
    """The rows of one block: the largest multiple of 256 whose checkpoints -- 4 kp (kp + 1) / 2 bytes per sample and point (144 at
    K = 8) -- fit ``budget`` bytes, at least 256."""
    kp = int(lib.nadm_pad_k(K))
    per_row = 4 * n_pairs(kp) * max(int(n_out), 1)
    return max(256, (int(budget) // per_row) // 256 * 256)


def local_ancestry(xp: torch.Tensor, M: int, P, Q, cm, chrom, generations: float, idx: Optional[torch.Tensor] = None,
                   grid: float = GRID, eps: float = EPS, dosage: bool = False, budget: int = SCRATCH_BUDGET) -> LocalAncestry:
    """The posterior local ancestry of ONE sample group -- the rows ``idx`` (int32, default: every row) of the packed device matrix
    ``xp [rows, ld]`` -- given ``P [M, K]``, the group's rows of ``Q`` (in the order of ``idx``), the genetic map ``cm [M]`` (cM) per
    chromosome ``chrom [M]`` and the number of ``generations``, at the output points of ``output_points(cm, chrom, grid)``.  The rows
    are worked off in blocks of ``block_rows`` so that the checkpoints stay under ``budget`` bytes; a sample's result does not depend on
    the blocking (the library's contract).  ``dosage``: also keep float32 ``[N, points, K]`` on the host."""
    b, K, Pp, Qp = _operands(xp, M, P, Q, idx, "local_ancestry")
    rho, ranges = switch_prob(cm, chrom, generations)
    if len(rho) != int(M):
        raise RuntimeError(f"local_ancestry: the map holds {len(rho)} SNPs, the genotypes {int(M)}")
    out_snp, oseg = output_points(cm, chrom, grid)
    if 100.0 / float(generations) < 4.0 * float(grid):
        log.warning(f"    Warning: the mean tract at {float(generations):g} generations is {100.0 / float(generations):.3g} cM, fewer than 4 "
                    f"output points of {float(grid):g} cM: tracts will be missed between the points; use a finer --grid.")
    seg, out_snp, oseg = check_layout(M, [m0 for m0, _ in ranges] + [ranges[-1][1]], out_snp, oseg)
    dev = xp.device
    rho_d, seg_d = _rho_operand(rho, M, dev), torch.from_numpy(seg).to(dev)
    out_d, oseg_d = torch.from_numpy(out_snp).to(dev), torch.from_numpy(oseg).to(dev)
    n_out, step = len(out_snp), block_rows(len(out_snp), K, budget)
    call = np.empty((b, n_out), dtype=np.uint8)
    post = np.empty((b, n_out), dtype=np.float32)
    ll = np.empty((b, len(ranges)), dtype=np.float64)
    share = np.empty((b, K), dtype=np.float64)
    psum = torch.zeros((n_out, K), dtype=torch.float64, device=dev)
    pcnt = torch.zeros(n_out, dtype=torch.float64, device=dev)
    dos = np.empty((b, n_out, K), dtype=np.float32) if dosage else None
    rows = idx if idx is not None else torch.arange(b, dtype=torch.int32, device=dev)
    nan_points = 0
    for r0 in range(0, b, step):
        r1 = min(b, r0 + step)
        sub = None if (idx is None and step >= b) else rows[r0:r1].contiguous()
        d, c, p, l_ = forward_backward(xp, M, Pp, Qp[r0:r1], K, sub, r1 - r0, rho_d, seg_d, out_d, oseg_d, eps)
        d = d[:, :, :K]
        ok = ~torch.isnan(p)
        half = torch.where(ok[:, :, None], d.to(torch.float64) * 0.5, torch.zeros((), dtype=torch.float64, device=dev))
        cnt = ok.sum(dim=1).to(torch.float64)
        share[r0:r1] = (half.sum(dim=1) / cnt[:, None]).cpu().numpy()
        psum += half.sum(dim=0)
        pcnt += ok.sum(dim=0).to(torch.float64)
        nan_points += int((~ok).sum())
        call[r0:r1], post[r0:r1], ll[r0:r1] = c.cpu().numpy(), p.cpu().numpy(), l_.cpu().numpy()
        if dosage:
            dos[r0:r1] = d.cpu().numpy()
    point_share = (psum / pcnt[:, None]).cpu().numpy()
    return LocalAncestry(call, post, ll, share, point_share, nan_points, dos, out_snp, oseg, ranges, float(generations))


def loglik(xp: torch.Tensor, M: int, P, Q, cm, chrom, generations: float, idx: Optional[torch.Tensor] = None, eps: float = EPS) -> np.ndarray:
    """The forward pass alone: float64 ``[N, chromosomes]``, the log-likelihood of every sample's calls on every chromosome at that
    number of generations."""
    b, K, Pp, Qp = _operands(xp, M, P, Q, idx, "loglik")
    rho, ranges = switch_prob(cm, chrom, generations)
    seg, _, _ = check_layout(M, [m0 for m0, _ in ranges] + [ranges[-1][1]])
    dev = xp.device
    return forward_backward(xp, M, Pp, Qp, K, idx, b, _rho_operand(rho, M, dev), torch.from_numpy(seg).to(dev), None, None, eps,
                            full=False)[3].cpu().numpy()


def scan_generations(xp: torch.Tensor, M: int, P, Q, cm, chrom, idx: Optional[torch.Tensor] = None, scan_samples: int = SCAN_SAMPLES,
                     eps: float = EPS, n_grid=None):
    """The number of generations that maximises the total log-likelihood of at most ``scan_samples`` rows of the group (taken by
    stride): the fixed log grid ``N_GRID`` over 1..1000, then golden section in log n between the grid neighbours of the best point.
    Returns ``(n, grid, ll_grid)``: the estimate and the total log-likelihood at every grid point.  A maximum at an end of the grid is
    returned as that end, with a warning."""
    b, K, Pp, Qp = _operands(xp, M, P, Q, idx, "scan_generations")
    if int(scan_samples) < 1:
        raise RuntimeError("scan_generations: scan_samples must be >= 1")
    dev = xp.device
    take = np.arange(0, b, max(1, -(-b // int(scan_samples))))
    take_d = torch.from_numpy(take.astype(np.int64)).to(dev)
    rows = (idx if idx is not None else torch.arange(b, dtype=torch.int32, device=dev))[take_d].contiguous()
    Qs = Qp[take_d].contiguous()
    _, ranges = switch_prob(cm, chrom, 1.0)
    seg, _, _ = check_layout(M, [m0 for m0, _ in ranges] + [ranges[-1][1]])
    seg_d = torch.from_numpy(seg).to(dev)

    def total(n: float) -> float:
        rho, _ = switch_prob(cm, chrom, n)
        ll = forward_backward(xp, M, Pp, Qs, K, rows, len(take), _rho_operand(rho, M, dev), seg_d, None, None, eps, full=False)[3]
        return float(ll.sum())

    grid = np.asarray(N_GRID if n_grid is None else n_grid, dtype=np.float64)
    lls = np.array([total(n) for n in grid])
    if not np.all(np.isfinite(lls)):
        raise RuntimeError("scan_generations: the log-likelihood is not finite; check P, Q and the map")
    i = int(np.argmax(lls))
    if i == 0 or i == len(grid) - 1:
        log.warning(f"    Warning: the log-likelihood is largest at the end of the grid ({grid[i]:g} generations); the panel does not date "
                    "its admixture through this model.")
        return float(grid[i]), grid, lls
    lo, hi = math.log(grid[i - 1]), math.log(grid[i + 1])
    g = (math.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = total(math.exp(x1)), total(math.exp(x2))
    for _ in range(GOLDEN_STEPS):
        if hi - lo < 1e-3:
            break
        if f1 >= f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo)
            f1 = total(math.exp(x1))
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo)
            f2 = total(math.exp(x2))
    return math.exp(0.5 * (lo + hi)), grid, lls


# ---- what is read off the calls ---------------------------------------------------------------------------------------------------
def tracts(call: np.ndarray, out_snp, oseg, cm):
    """``(switches int64 [N], mean_tract_cM float64 [N])`` from the calls: a switch is a change of the called pair between two
    neighbouring output points of one chromosome (a point without a call, 255, is skipped); the mean tract is twice the map length
    covered by the points over (switches + 2 chromosomes with points): two haplotypes share the switches.  Calls on a grid miss the
    tracts shorter than the grid."""
    call, cm = np.asarray(call), np.asarray(cm, dtype=np.float64)
    N = call.shape[0]
    sw = np.zeros(N, dtype=np.int64)
    length, pieces = 0.0, 0
    for s in range(len(oseg) - 1):
        a, b = int(oseg[s]), int(oseg[s + 1])
        if b - a < 1:
            continue
        pieces += 1
        length += float(cm[out_snp[b - 1]] - cm[out_snp[a]])
        for i in range(N):
            c = call[i, a:b]
            c = c[c != 255]
            sw[i] += int(np.count_nonzero(c[1:] != c[:-1]))
    return sw, 2.0 * length / (sw + 2.0 * pieces)


def far_from_q(share: np.ndarray, Q: np.ndarray, spread: float = WARN_SPREAD) -> np.ndarray:
    """The samples whose mean local share is further from their ``Q`` row (largest absolute difference over the components) than
    ``spread`` times the root mean square of that distance over the OTHER samples: a convention, not a test."""
    d = np.abs(np.asarray(share, dtype=np.float64) - np.asarray(Q, dtype=np.float64)).max(axis=1)
    d = np.where(np.isnan(d), np.inf, d)
    fin = np.isfinite(d)
    n = int(fin.sum())
    if n < 2:
        return np.flatnonzero(~fin)
    tot = float((d[fin] ** 2).sum())
    others = np.sqrt(np.maximum(tot - np.where(fin, d, 0.0) ** 2, 0.0) / np.maximum(n - fin.astype(int), 1))
    return np.flatnonzero(d > float(spread) * np.maximum(others, 1e-6))


def point_deviation(point_share: np.ndarray) -> np.ndarray:
    """The local-ancestry-deviation scan: per point and component ``(share - mean over points) / standard deviation over points``
    (NaN where a component's share does not vary)."""
    ps = np.asarray(point_share, dtype=np.float64)
    mu, sd = np.nanmean(ps, axis=0), np.nanstd(ps, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sd > 0.0, (ps - mu) / sd, np.nan)


# ---- the command line's side ------------------------------------------------------------------------------------------------------
def log_results(res: LocalAncestry, Q, cm, k: int, logger, spread: float = WARN_SPREAD) -> None:
    N, pts = res.call.shape
    sw, tract = tracts(res.call, res.out_snp, res.oseg, cm)
    logger.info(f"    Local ancestry (K={k}, {res.generations:.4g} generations): {N} samples at {pts} points on {len(res.ranges)} chromosomes; "
                f"total log-likelihood {res.ll.sum():.6e}; median called posterior {float(np.nanmedian(res.post)) if pts else float('nan'):.3f}; "
                f"median switches per sample {float(np.median(sw)):.0f}, median tract {float(np.median(tract)):.3g} cM; "
                f"{res.nan_points} of {N * pts} points are NaN.")
    far = far_from_q(res.share, Q, spread)
    if len(far):
        logger.info(f"    Warning: the mean local share of {len(far)} samples is further from their Q than {spread:g} times the other samples' "
                    "spread (0-based index): " + " ".join(str(int(i)) for i in far[:10]) + (" ..." if len(far) > 10 else ""))


def write_results(save_dir: str, name: str, k: int, res: LocalAncestry, Q, cm, chrom_labels=None, snp_ids=None, bp=None) -> None:
    """``{name}.{k}.lanc``: a row per output point, ``chrom snp_id bp cM`` then per sample the called pair ``a/b`` (1-based, ``./.``
    without a call); ``{name}.{k}.lanc.sample``: a header, then per sample the log-likelihood, per component the mean local share next
    to its Q, the switches and the mean tract length in cM; ``{name}.{k}.lanc.mean``: a header, then per point ``chrom snp_id bp cM``,
    the mean share per component over the samples and its deviation from the mean over the points in units of the spread over the
    points; ``{name}.{k}.lanc.dosage.npy`` (float32 ``[N, points, K]``) where the dosage was kept."""
    os.makedirs(save_dir, exist_ok=True)
    stem = os.path.join(save_dir, f"{name}.{k}.lanc")
    cm = np.asarray(cm, dtype=np.float64)
    Qn = np.asarray(Q.detach().cpu() if torch.is_tensor(Q) else Q, dtype=np.float64)
    names = np.asarray(["./."] * 256, dtype=object)
    for i, (a, b) in enumerate(pair_table(k)):
        names[i] = f"{a + 1}/{b + 1}"

    def where(j):
        return (f"{chrom_labels[j] if chrom_labels is not None else 0} {snp_ids[j] if snp_ids is not None else j} "
                f"{int(bp[j]) if bp is not None else 0} {cm[j]:.6g}")
    with open(stem, "w") as fb:
        for o, j in enumerate(res.out_snp):
            fb.write(where(int(j)) + " " + " ".join(names[res.call[:, o]]) + "\n")
    sw, tract = tracts(res.call, res.out_snp, res.oseg, cm)
    with open(f"{stem}.sample", "w") as fb:
        fb.write(" ".join(["loglik"] + [f"{h}{c + 1}" for c in range(k) for h in ("local", "Q")] + ["switches", "tract_cM"]) + "\n")
        for i in range(res.call.shape[0]):
            cols = [f"{v:.6g}" for c in range(k) for v in (res.share[i, c], Qn[i, c])]
            fb.write(" ".join([f"{res.ll[i].sum():.9e}"] + cols + [str(int(sw[i])), f"{tract[i]:.6g}"]) + "\n")
    dev = point_deviation(res.point_share)
    with open(f"{stem}.mean", "w") as fb:
        fb.write(" ".join(["chrom", "snp_id", "bp", "cM"] + [f"{h}{c + 1}" for c in range(k) for h in ("share", "dev")]) + "\n")
        for o, j in enumerate(res.out_snp):
            fb.write(where(int(j)) + " " + " ".join(f"{v:.6g}" for c in range(k) for v in (res.point_share[o, c], dev[o, c])) + "\n")
    if res.dosage is not None:
        np.save(f"{stem}.dosage.npy", res.dosage)
