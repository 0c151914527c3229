"""LD pruning: windowed r^2 of neighbouring SNPs from the packed genotype matrix, the greedy keep-list, and the selection of SNPs.

ADMIXTURE-type models assume SNPs in linkage equilibrium; the usual preparation is ``plink --indep-pairwise 50 10 0.1``.  Here the
r^2 of every SNP with its next ``window - 1`` neighbours is a banded Gram product over the sample axis of the packed matrix
(``nadm_ld_band``, include/nadm.h: int8 operands on the matrix pipe, int32 sums, exact), a host sweep turns the band into a
keep-list (``nadm_ld_sweep``: plink's rule with a step of 1 and without its window bookkeeping -- plink's own list is not
promised), and ``select_snps`` gives the kept SNPs as an ordinary :class:`~.io.PackedGenotypes`.

``snp_counts`` and ``ld_band`` are the two kernels, ``prune`` runs the band range by range and sweeps each range on the host,
``select_snps`` is what ``--extract`` of the command line applies right after the read.
"""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, n_rows, stream
from .io import read_bim, chrom_codes, read_id_list, write_id_list, resolve_ids    # noqa: F401  (their callers' old home)

MAX_WINDOW = 1025            # NADM_LD_MAX_WINDOW + 1: a SNP and its next 1024


def _rows(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], what: str) -> int:
    rows = n_rows(xp, idx)
    check_packed(xp, idx, rows, what)
    if int(M) < 1 or int(M) > 4 * int(xp.shape[1]):
        raise RuntimeError(f"{what}: M must be in 1..{4 * int(xp.shape[1])} for rows of {int(xp.shape[1])} bytes")
    return rows


def snp_counts(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per SNP of the packed device matrix ``xp [rows, ld]`` over the rows ``idx`` (int32, default: every row): int32 ``[M, 3]`` on
    xp's device with the number of observed calls, their sum and their sum of squares."""
    rows = _rows(xp, M, idx, "snp_counts")
    cnt = torch.empty((int(M), 3), dtype=torch.int32, device=xp.device)
    check(lib.nadm_snp_counts(ptr(xp), xp.shape[1], ptr(idx), rows, int(M), ptr(cnt), stream()), "snp_counts")
    return cnt


def ld_band(xp: torch.Tensor, M: int, window: int, m0: int = 0, m1: Optional[int] = None, idx: Optional[torch.Tensor] = None,
            with_moments: bool = False):
    """r^2 of every SNP ``j`` in ``[m0, m1)`` (default: all) with its next ``window - 1`` neighbours over the rows ``idx`` (default:
    every row) where both calls are observed: float64 ``[m1 - m0, window - 1]`` on xp's device, entry ``(j - m0, d)`` the pair
    ``(j, j + 1 + d)``; exactly 0 where a SNP does not vary among those rows or ``j + 1 + d >= M``.  ``with_moments``: also the six
    integer sums ``(n, Sa, Sb, Sab, Saa, Sbb)`` as int32 ``[m1 - m0, window - 1, 6]``."""
    rows = _rows(xp, M, idx, "ld_band")
    window, m0 = int(window), int(m0)
    m1 = int(M) if m1 is None else int(m1)
    if window < 2 or window > MAX_WINDOW:
        raise RuntimeError(f"ld_band: window must be in 2..{MAX_WINDOW} (a SNP and its next window - 1)")
    W = window - 1
    if not 0 <= m0 < m1 <= int(M):
        raise RuntimeError(f"ld_band: need 0 <= m0 < m1 <= M, got m0 = {m0}, m1 = {m1}, M = {int(M)}")
    r2 = torch.empty((m1 - m0, W), dtype=torch.float64, device=xp.device)
    mom = torch.empty((m1 - m0, W, 6), dtype=torch.int32, device=xp.device) if with_moments else None
    check(lib.nadm_ld_band(ptr(xp), xp.shape[1], ptr(idx), rows, int(M), m0, m1, W, ptr(r2), ptr(mom), stream()), "ld_band")
    return (r2, mom) if with_moments else r2


def maf_from_counts(cnt) -> np.ndarray:
    """Minor-allele frequency per SNP from ``snp_counts``: ``min(S, 2 n - S) / (2.0 n)`` in float64, 0 where no call is observed."""
    c = np.asarray(cnt.cpu() if torch.is_tensor(cnt) else cnt, dtype=np.int64)
    n, S = c[:, 0], c[:, 1]
    out = np.zeros(len(n), dtype=np.float64)
    ok = n > 0
    out[ok] = np.minimum(S[ok], 2 * n[ok] - S[ok]).astype(np.float64) / (2.0 * n[ok].astype(np.float64))
    return out


def sweep(r2: np.ndarray, m0: int, m1: int, M: int, maf: np.ndarray, chrom: Optional[np.ndarray], thr: float, kept: np.ndarray) -> None:
    """One ``nadm_ld_sweep`` call (host): the band ``r2 [m1 - m0, W]`` of the SNPs ``[m0, m1)`` removes SNPs from ``kept`` (uint8
    ``[M]``, in place)."""
    for a, dt, name in ((r2, np.float64, "r2"), (maf, np.float64, "maf"), (kept, np.uint8, "kept")):
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags["C_CONTIGUOUS"]:
            raise RuntimeError(f"sweep: {name} must be a contiguous {np.dtype(dt).name} array")
    if r2.ndim != 2 or r2.shape[0] != int(m1) - int(m0) or maf.shape != (int(M),) or kept.shape != (int(M),):
        raise RuntimeError("sweep: r2 must be [m1 - m0, W], maf and kept [M]")
    cp = None
    if chrom is not None:
        if not isinstance(chrom, np.ndarray) or chrom.dtype != np.int32 or chrom.shape != (int(M),) or not chrom.flags["C_CONTIGUOUS"]:
            raise RuntimeError("sweep: chrom must be a contiguous int32 array [M]")
        cp = chrom.ctypes.data
    check(lib.nadm_ld_sweep(r2.ctypes.data, int(m0), int(m1), int(r2.shape[1]), int(M), maf.ctypes.data, cp, float(thr),
                            kept.ctypes.data), "ld_sweep")


def prune(xp: torch.Tensor, M: int, window: int = 50, r2: float = 0.1, chrom=None, idx: Optional[torch.Tensor] = None,
          range_snps: int = 65536):
    """The keep-list of LD pruning for the packed device matrix ``xp [rows, ld]``: of every pair of SNPs less than ``window`` apart
    (and on the same chromosome: ``chrom``, one integer label per SNP, None = one chromosome) whose r^2 over the rows ``idx``
    exceeds ``r2``, the one with the smaller minor-allele frequency goes (the later one on a tie), in one ascending pass
    (include/nadm.h, nadm_ld_sweep).  The band is computed ``range_snps`` SNPs at a time; each range comes to the host and is swept
    there.  Returns ``(keep, stats)``: ``keep`` bool ``[M]`` on the host, ``stats`` a dict with the counts and the seconds spent."""
    rows = _rows(xp, M, idx, "prune")
    M, window, range_snps = int(M), int(window), int(range_snps)
    if window < 2 or window > MAX_WINDOW:
        raise RuntimeError(f"prune: window must be in 2..{MAX_WINDOW} (a SNP and its next window - 1)")
    if not 0.0 <= float(r2) <= 1.0:
        raise RuntimeError("prune: r2 must be in [0, 1]")
    if range_snps < 1:
        raise RuntimeError("prune: range_snps must be >= 1")
    ch = None
    if chrom is not None:
        ch = np.ascontiguousarray(np.asarray(chrom), dtype=np.int32)
        if ch.shape != (M,):
            raise RuntimeError(f"prune: chrom must hold one label per SNP ({M}), got {ch.shape}")
    t0 = time.time()
    maf = maf_from_counts(snp_counts(xp, M, idx))
    kept = np.ones(M, dtype=np.uint8)
    t_band = t_sweep = 0.0
    n_ranges = 0
    for m0 in range(0, M, range_snps):
        m1 = min(M, m0 + range_snps)
        t1 = time.time()
        band = ld_band(xp, M, window, m0, m1, idx).cpu().numpy()
        t2 = time.time()
        sweep(band, m0, m1, M, maf, ch, float(r2), kept)
        t_band, t_sweep, n_ranges = t_band + (t2 - t1), t_sweep + (time.time() - t2), n_ranges + 1
    keep = kept.astype(bool)
    stats = {"M": M, "rows": rows, "window": window, "r2": float(r2), "kept": int(keep.sum()), "removed": int(M - keep.sum()),
             "ranges": n_ranges, "seconds_band": t_band, "seconds_sweep": t_sweep, "seconds": time.time() - t0}
    return keep, stats


def select_snps(data, keep):
    """The SNPs ``keep`` (bool ``[M]``) of ``data`` (:class:`~.io.PackedGenotypes`) as a PackedGenotypes of ``keep.sum()`` SNPs with
    the row stride ``ModelLayout.row_stride`` gives them, on the device the input is on.  The orientation is decided again on the
    subset by the reader's rule (flip 0 <-> 2 when the mean code of the file's own genotypes, 3s included, is >= 1), so the result
    is byte for byte what ``read_bed_packed`` returns for a BED that holds only those SNPs; ``flipped`` says whether the result is
    flipped against the file."""
    from .io import PackedGenotypes
    from .layout import ModelLayout
    if not hasattr(data, "packed") or not torch.is_tensor(data.packed):
        raise RuntimeError("select_snps: data must be a PackedGenotypes")
    keep = np.asarray(keep.cpu() if torch.is_tensor(keep) else keep)
    if keep.dtype != np.bool_ or keep.shape != (data.M,):
        raise RuntimeError(f"select_snps: keep must be a bool vector with one entry per SNP ({data.M})")
    M_out = int(keep.sum())
    if M_out < 1:
        raise RuntimeError("select_snps: keep selects no SNP")
    home = data.packed.device
    if home.type != "cuda" and not torch.cuda.is_available():
        raise RuntimeError("select_snps: the selection runs on a ROCm GPU (no CPU fallback)")
    xp = data.packed if home.type == "cuda" else data.packed.to("cuda:0")
    if xp.dtype != torch.uint8 or xp.dim() != 2 or not xp.is_contiguous() or xp.shape[0] != data.N:
        raise RuntimeError("select_snps: data.packed must be a contiguous uint8 [N, ld] matrix")
    with torch.cuda.device(xp.device):
        kidx = torch.from_numpy(np.nonzero(keep)[0].astype(np.int64)).to(xp.device)
        c = snp_counts(xp, data.M)[kidx].to(torch.int64).sum(dim=0).cpu()
        n_obs, S = int(c[0]), int(c[1])
        if data.flipped:                                     # the file's own codes: 2 - g at every observed call
            S = 2 * n_obs - S
        total = S + 3 * (data.N * M_out - n_obs)             # the reader's sum of codes, 3s included
        flip_file = total >= data.N * M_out                  # mean >= 1
        ld_out = ModelLayout.row_stride(M_out)
        out = torch.empty((data.N, ld_out), dtype=torch.uint8, device=xp.device)
        check(lib.nadm_select_snps(ptr(xp), xp.shape[1], data.N, ptr(kidx), M_out, int(bool(flip_file) != bool(data.flipped)), ptr(out),
                                   ld_out, stream()), "select_snps")
        if home.type != "cuda":
            out = out.to(home)
        else:
            torch.cuda.current_stream().synchronize()        # kidx is freed on return
    return PackedGenotypes(out, data.N, M_out, bool(flip_file))
