"""Standard errors of ``P``: the per-SNP Fisher information of a SNP's frequency row given the ancestry fractions, inverted per SNP.

The sampling error of ``p_jk`` comes from the sample axis -- from how many allele copies of ancestry ``k`` were observed at SNP ``j``
-- and differs by orders of magnitude between a component carried by thousands of unadmixed samples and one that exists only as
small fractions of admixed ones.  With ``pi_ij = sum_k q_ik p_jk`` and a call binomial(2, pi_ij), the expected information of the
row ``p_j.`` is

    I_j[a][b] = sum_i m_ij 2 / (pi_ij (1 - pi_ij)) q_ia q_ib                  (m: the call is observed)

and ``SE_jk = sqrt((I_j^-1)_kk)``, the inverse taken over the SNP's FREE components in float64.  A component is *fixed* when
``p_jk <= bound`` or ``p_jk >= 1 - bound`` (the maximum is then not interior and normal theory does not apply) and *unseen* when
``I_j[k][k] = 0`` (nobody observed at the SNP carries it); both are dropped from the block and get NaN, and so does every entry of a
SNP whose free block is not positive definite or that nobody observes.  ``n_eff_jk = p (1 - p) / SE^2`` is the effective number of
allele copies behind ``p_jk``: exactly ``2 n_j`` for K = 1, twice the observed samples of population k for one-hot Q rows.

The standard error is CONDITIONAL ON Q: the uncertainty of the ancestry fractions themselves is not in it.  Q is estimated from all
SNPs and a row of P from one, so the cross term is small: on simulated panels the median ratio of this SE to
the rms error of a JOINT block-EM fit of Q and P about the truth was 1.006 (300 samples x 3000 SNPs, K = 3; 94.5 % of |z| < 1.96),
and 1.006 of the spread of P refitted at the true Q, which is why it is usable as it is.

``p_info`` is ``nadm_snp_info`` (include/nadm.h: reproducible bit for bit) over blocks of rows, ``se_from_info`` the float64
inversion (``nadm_snp_info_se``, a thread per SNP, on a GPU; LAPACK's batched Cholesky through torch on the CPU), ``p_se`` the two together,
``Engine.p_se`` runs it on the resident matrix with the engine's own P and the encoder's final Q.  K <= 16: the K (K + 1) / 2
running sums of a SNP live in one thread's registers.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import model_operands, stream

EPS = 1e-6           # clip of pi and of 1 - pi: the projection's (project.EPS)
BOUND = 1e-4         # a p within this of 0 or 1 is fixed (polish clips P at 1e-6, training at 0 / 1)
ROW_BLOCK = 32768    # rows per nadm_snp_info call: bounds the scratch by 8 slices x M x (T + 1) x 4 bytes
MAX_K = 16
SNP_BATCH = 1 << 16  # SNPs per batched factorisation (the CPU route)
TOO_WIDE = "K must be <= 16 for standard errors of P (the K (K + 1) / 2 running sums of a SNP live in one thread's registers)"


class PseResult(NamedTuple):
    """Per SNP and component, on the information's device: ``se`` and ``n_eff`` float64 ``[M, K]`` (NaN where no standard error is
    defined), ``n`` int32 ``[M]`` the observed calls, ``fixed`` and ``unseen`` bool ``[M, K]``."""
    se: torch.Tensor
    n_eff: torch.Tensor
    n: torch.Tensor
    fixed: torch.Tensor
    unseen: torch.Tensor


def n_pairs(K: int) -> int:
    return K * (K + 1) // 2


def p_info(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, eps: float = EPS, row_block: int = ROW_BLOCK):
    """The expected information of every SNP's row of ``P [M, K]`` given ``Q [b, K]`` (host or device; row s of Q belongs to
    ``idx[s]``) over the rows ``idx`` (int32, default: every row) of the packed device matrix ``xp [rows, ld]``: ``(info, n)`` on xp's
    device, float64 ``[M, K (K + 1) / 2]`` (the pairs a <= b, a-major) and int32 ``[M]``.  The rows go through ``nadm_snp_info`` in
    blocks of at most ``row_block`` (a multiple of 64) and the blocks' float64 results are added in block order: a fixed function of
    the shape, and the scratch stays bounded whatever b is."""
    M, row_block = int(M), int(row_block)
    if row_block < 64 or row_block % 64 != 0:
        raise RuntimeError("p_info: row_block must be a positive multiple of 64")
    if np.ndim(P) == 2 and int(np.shape(P)[1]) > MAX_K:
        raise RuntimeError(f"p_info: {TOO_WIDE}")
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="p_info")
    kp, ld, dev = int(Pp.shape[1]), int(xp.shape[1]), xp.device
    n_scr = int(lib.nadm_snp_info_scratch_floats(min(b, row_block), M, kp))
    if n_scr <= 0:
        raise RuntimeError(f"p_info: a block of {b} rows over {M} SNPs with K = {K} is not supported")
    scratch = torch.empty(n_scr, dtype=torch.float32, device=dev)
    info = n = None
    for s in range(0, b, row_block):
        bb = min(row_block, b - s)
        blk_info = torch.empty((M, n_pairs(K)), dtype=torch.float64, device=dev)
        blk_n = torch.empty(M, dtype=torch.int32, device=dev)
        rows, xb = (idx[s:s + bb], xp) if idx is not None else (None, xp[s:s + bb])
        Qb = Qp[s:s + bb]
        check(lib.nadm_snp_info(ptr(xb), ld, ptr(rows), bb, M, ptr(Qb), Qp.stride(0), K, kp, ptr(Pp), float(eps), ptr(blk_info), ptr(blk_n),
                                ptr(scratch), stream()), "snp_info")
        info, n = (blk_info, blk_n) if info is None else (info + blk_info, n + blk_n)
    return info, n


def _as_f64(a, device) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(device=device, dtype=torch.float64)


def _se_lapack(info, free, n, ia, ib):
    """The CPU route of ``se_from_info``: the free blocks, padded with the identity, through LAPACK's batched factorisation."""
    M, K = free.shape
    eye = torch.eye(K, dtype=torch.float64)
    se = torch.full((M, K), float("nan"), dtype=torch.float64)
    for s in range(0, M, SNP_BATCH):
        f = free[s:s + SNP_BATCH]
        A = torch.zeros((f.shape[0], K, K), dtype=torch.float64)
        A[:, ia, ib] = info[s:s + SNP_BATCH]
        A[:, ib, ia] = info[s:s + SNP_BATCH]
        ff = f.to(torch.float64)
        A = A * ff[:, :, None] * ff[:, None, :] + torch.diag_embed(1.0 - ff)
        L, flag = torch.linalg.cholesky_ex(A)
        bad = (flag != 0) | (n[s:s + SNP_BATCH] == 0) | ~torch.isfinite(L).all(dim=(1, 2))
        L = torch.where(bad[:, None, None], eye, L)
        var = torch.diagonal(torch.cholesky_inverse(L), dim1=1, dim2=2)
        ok = f & ~bad[:, None] & (var > 0) & torch.isfinite(var)
        se[s:s + SNP_BATCH] = torch.where(ok, torch.sqrt(var.clamp_min(0.0)), se[s:s + SNP_BATCH])
    return se


def se_from_info(info: torch.Tensor, P, n: torch.Tensor, bound: float = BOUND) -> PseResult:
    """The float64 standard errors from the information (any device, the CPU included): ``info [M, K (K + 1) / 2]`` as ``p_info``
    writes it, ``P [M, K]``, ``n [M]``.  Fixed and unseen components are taken out of a SNP's block by zeroing their rows and columns
    and putting 1 on their diagonal.  On a GPU the blocks are inverted by ``nadm_snp_info_se``, a thread-per-SNP float64 Cholesky
    kernel (include/nadm.h; K <= 16); on the CPU by ``torch.linalg.cholesky_ex`` + ``cholesky_inverse`` over batches of SNPs.  (The
    batched torch route is NOT used on the device: on the ROCm build it flagged positive definite blocks and returned wrong
    inverses at batches of 65536 blocks.)  A SNP whose free block is not positive definite, or with ``n = 0``, is NaN throughout."""
    if not 0.0 <= float(bound) < 0.5:
        raise RuntimeError("se_from_info: bound must be in [0, 0.5)")
    dev = info.device
    info = info.to(torch.float64)
    Pt = _as_f64(P, dev)
    if Pt.dim() != 2 or info.dim() != 2:
        raise RuntimeError("se_from_info: info must be [M, K (K + 1) / 2] and P [M, K]")
    M, K = Pt.shape
    n = torch.as_tensor(n).to(dev)
    if tuple(info.shape) != (M, n_pairs(K)) or tuple(n.shape) != (M,):
        raise RuntimeError(f"se_from_info: P is [{M}, {K}]: info must be [{M}, {n_pairs(K)}] and n [{M}]")
    ia, ib = torch.triu_indices(K, K, device=dev)                     # the pairs a <= b, a-major: info's column order
    diag = info[:, ia == ib]
    fixed = (Pt <= float(bound)) | (Pt >= 1.0 - float(bound))
    unseen = diag == 0
    free = ~(fixed | unseen)
    if dev.type == "cuda":
        if K > MAX_K:
            raise RuntimeError(f"se_from_info: {TOO_WIDE}")
        info, n32, drop = info.contiguous(), n.to(torch.int32).contiguous(), (~free).to(torch.uint8).contiguous()
        se = torch.empty((M, K), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(lib.nadm_snp_info_se(ptr(info), ptr(drop), ptr(n32), M, K, ptr(se), stream()), "snp_info_se")
    else:
        se = _se_lapack(info, free, n, ia, ib)
    n_eff = Pt * (1.0 - Pt) / (se * se)
    return PseResult(se, n_eff, n.to(torch.int32), fixed, unseen)


def p_se(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, bound: float = BOUND) -> PseResult:
    """Standard errors of ``P [M, K]`` given ``Q`` for every SNP of the packed device matrix (arguments as ``p_info``; ``bound``:
    ``se_from_info``).  Conditional on Q (module docstring)."""
    info, n = p_info(xp, M, P, Q, idx)
    return se_from_info(info, P, n, bound)


def write_se(path, se) -> None:
    """``se [M, K]`` in the ``.P`` text format (``io.savetxt`` of the float32 values), NaN as ``nan``."""
    from .io import savetxt
    a = np.asarray(se.cpu() if torch.is_tensor(se) else se).astype(np.float32)
    if a.ndim != 2:
        raise RuntimeError("write_se: se must be a matrix [M, K]")
    a[np.isnan(a)] = np.float32("nan")                                  # one NaN: the positive quiet one, printed as `nan`
    savetxt(path, a)


def write_results(save_dir, name: str, results: Sequence[PseResult]) -> None:
    """``{save_dir}/{name}.{K}.P_se`` per head."""
    import os
    os.makedirs(save_dir, exist_ok=True)
    for r in results:
        write_se(os.path.join(save_dir, f"{name}.{int(r.se.shape[1])}.P_se"), r.se)


def log_results(results: Sequence[PseResult], log) -> None:
    """Per K one line: the median standard error, the median effective number of allele copies per component, and how many
    SNP-components are fixed, unseen, or without a standard error for any reason."""
    for r in results:
        M, K = r.se.shape
        se, ne = r.se.cpu().numpy(), r.n_eff.cpu().numpy()
        have = ~np.isnan(se)
        med = float(np.median(se[have])) if have.any() else float("nan")
        per_k = ", ".join(f"{np.median(ne[have[:, k], k]):.1f}" if have[:, k].any() else "nan" for k in range(K))
        log.info(f"P standard errors (K={K}): median SE {med:.5f}; median n_eff per component {per_k}; of {M * K} SNP-components "
                 f"{int(r.fixed.sum())} fixed, {int(r.unseen.sum())} unseen, {int((~have).sum())} NaN")
