"""Standard errors of ``Q`` given ``P``: the per-sample Fisher information of a sample's row of ancestry fractions, inverted per
sample under the constraint that the row sums to one.  The mirror image of ``pse.py``.

A projected sample (``infer --refine``, ``project.project_q``) gets a row of ``Q`` and nothing else, and a sample with 3 % of its
calls observed gets one that looks as confident as a fully typed sample's.  Its sampling error comes from the SNP axis.  With
``pi_ij = sum_k q_ik p_jk`` and a call binomial(2, pi_ij), the expected information of the row ``q_i.`` is

    A_i[a][b] = sum_j o_ij 2 / (pi_ij (1 - pi_ij)) p_ja p_jb                  (o: the call is observed)

and, every component being free under ``sum_k q_ik = 1``,

    Cov_i = A^-1 - A^-1 1 1^T A^-1 / (1^T A^-1 1)         SE_ik = sqrt(Cov_i[k][k])

in float64.  What is built is the equivalent DROP-ONE form: leave component ``c`` out, ``J[a][b] = (A_ab - A_cb) - (A_ac - A_cc)``
for ``a, b != c``, ``SE_ia = sqrt((J^-1)_aa)``; ``c = K - 1`` gives every component but the last and ``c = 0`` the last one, so the
inversion kernel of ``pse.py`` (``nadm_snp_info_se``, "SNP" read as "sample", ``K - 1`` columns, nothing dropped) does the work
unchanged.  tests/qse_oracle.py holds both forms and shows that they agree.

Boundary components are NOT dropped, unlike ``pse``: most samples of a real panel are unadmixed, and dropping their zero components
would leave SE = 0 for what remains.  For a component at the floor the SE is what the estimate's spread would be were the boundary
not there -- a DETECTION LIMIT ("0 +- 2.5 %": an ancestry share below about two SEs could not have been told from none), not the
spread of the truncated estimator, which is smaller.  ``at_bound`` marks those entries (``q <= bound`` or ``q >= 1 - bound``).

NaN throughout a sample's row: no observed call (``n = 0``); a block that is not positive definite, or so close to singular that a
component's variance is inflated more than ``VIF_CAP`` = 1e12-fold by the others (two columns of P collinear over the sample's observed
SNPs: sums that carry fp32 rounding say nothing beyond that).  K = 1: the row is the constant 1 and its SE exactly 0.

The standard error is CONDITIONAL ON P.  That is right for projected samples, whose calls had no part in P.  For the samples of the
training panel it leaves out P's own error (``pse.py`` gives that, conditional on Q in turn): each is a lower bound there, and the
joint answer is ``bootstrap.bootstrap_q``'s.  Calibration on simulated panels: DESIGN.md section 4.18.

``q_info`` is ``nadm_sample_info`` (include/nadm.h: reproducible bit for bit) over blocks of rows, ``se_from_info`` the float64
inversion (``nadm_snp_info_se`` on a GPU; LAPACK's batched Cholesky through torch on the CPU, ``pse._se_lapack``), ``q_se`` the two
together, ``Engine.q_se`` runs it on the resident matrix with the engine's own P and the encoder's final Q.  K <= 16: the
K (K + 1) / 2 running sums of a sample live in one thread's registers.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import model_operands, stream
from .pse import _as_f64, _se_lapack, n_pairs

EPS = 1e-6           # clip of pi and of 1 - pi: the projection's (project.EPS)
BOUND = 1e-4         # a q within this of 0 or 1 is marked at_bound (the projection floors Q at 1e-5)
ROW_BLOCK = 32768    # rows per nadm_sample_info call: bounds the scratch by (1023 + 128) blocks x 256 x (T + 1) x 4 bytes
MAX_K = 16
VIF_CAP = 1e12       # (J^-1)_aa J_aa above this: the block is numerically singular
TOO_WIDE = "K must be <= 16 for standard errors of Q (the K (K + 1) / 2 running sums of a sample live in one thread's registers)"


class QseResult(NamedTuple):
    """Per sample and component, on the information's device: ``se`` float64 ``[b, K]`` (NaN throughout a sample without a standard
    error), ``n`` int32 ``[b]`` the observed calls, ``at_bound`` bool ``[b, K]`` (the SE there is a detection limit), ``cov`` None
    (the place of the full covariance, which nothing computes yet)."""
    se: torch.Tensor
    n: torch.Tensor
    at_bound: torch.Tensor
    cov: Optional[torch.Tensor] = None


def q_info(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, eps: float = EPS, row_block: int = ROW_BLOCK):
    """The expected information of every sample's row of ``Q [b, K]`` (host or device; row s belongs to ``idx[s]``) given ``P [M, K]``
    over the rows ``idx`` (int32, default: every row) of the packed device matrix ``xp [rows, ld]``: ``(info, n)`` on xp's device,
    float64 ``[b, K (K + 1) / 2]`` (the pairs a <= b, a-major) and int32 ``[b]``.  The rows go through ``nadm_sample_info`` in blocks
    of at most ``row_block`` (a multiple of 256) so that the scratch stays bounded whatever b is; a row is its own output, so the
    blocks are independent and the result does not depend on ``row_block``."""
    M, row_block = int(M), int(row_block)
    if row_block < 256 or row_block % 256 != 0:
        raise RuntimeError("q_info: row_block must be a positive multiple of 256")
    if np.ndim(P) == 2 and int(np.shape(P)[1]) > MAX_K:
        raise RuntimeError(f"q_info: {TOO_WIDE}")
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="q_info")
    kp, ld, dev = int(Pp.shape[1]), int(xp.shape[1]), xp.device
    n_scr = int(lib.nadm_sample_info_scratch_floats(min(b, row_block), M, kp))
    if n_scr <= 0:
        raise RuntimeError(f"q_info: a block of {b} rows over {M} SNPs with K = {K} is not supported")
    scratch = torch.empty(n_scr, dtype=torch.float32, device=dev)
    info = torch.empty((b, n_pairs(K)), dtype=torch.float64, device=dev)
    n = torch.empty(b, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for s in range(0, b, row_block):
            bb = min(row_block, b - s)
            rows, xb = (idx[s:s + bb], xp) if idx is not None else (None, xp[s:s + bb])
            check(lib.nadm_sample_info(ptr(xb), ld, ptr(rows), bb, M, ptr(Pp), K, kp, ptr(Qp[s:s + bb]), Qp.stride(0), float(eps),
                                       ptr(info[s:s + bb]), ptr(n[s:s + bb]), ptr(scratch), stream()), "sample_info")
    return info, n


def drop_one(info: torch.Tensor, K: int, c: int) -> torch.Tensor:
    """``info [b, K (K + 1) / 2]`` -> the information of the K - 1 components left free when component ``c`` takes up the constraint,
    ``J[a][b] = (A_ab - A_cb) - (A_ac - A_cc)`` over ``a <= b``, both != c, a-major: ``[b, (K - 1) K / 2]``.  (In this order of the
    differences a component whose column of P equals c's gets a row of exact zeros.)"""
    A = torch.zeros((info.shape[0], K, K), dtype=torch.float64, device=info.device)
    ia, ib = torch.triu_indices(K, K, device=info.device)
    A[:, ia, ib] = info
    A[:, ib, ia] = info
    keep = [a for a in range(K) if a != c]
    ja, jb = torch.triu_indices(K - 1, K - 1, device=info.device)
    ka, kb = torch.as_tensor(keep, device=info.device)[ja], torch.as_tensor(keep, device=info.device)[jb]
    return ((A[:, ka, kb] - A[:, c, kb]) - (A[:, ka, c] - A[:, c, c, None])).contiguous()


def _se_free(J: torch.Tensor, n: torch.Tensor, k: int) -> torch.Tensor:
    """sqrt(diag(J^-1)) of every ``k x k`` block of ``J [b, k (k + 1) / 2]``, NaN throughout a block that is not positive definite,
    has ``n = 0`` or a variance inflation above ``VIF_CAP``: the device's kernel or the CPU's LAPACK route, as ``pse.se_from_info``."""
    b, dev = J.shape[0], J.device
    ia, ib = torch.triu_indices(k, k, device=dev)
    if dev.type == "cuda":
        n32, drop = n.to(torch.int32).contiguous(), torch.zeros((b, k), dtype=torch.uint8, device=dev)
        se = torch.empty((b, k), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(lib.nadm_snp_info_se(ptr(J), ptr(drop), ptr(n32), b, k, ptr(se), stream()), "snp_info_se")
    else:
        se = _se_lapack(J, torch.ones((b, k), dtype=torch.bool), n, ia, ib)
    vif = se * se * J[:, ia == ib]
    bad = torch.isnan(se).any(dim=1) | ~(vif <= VIF_CAP).all(dim=1)
    return torch.where(bad[:, None], torch.full_like(se, float("nan")), se)


def se_from_info(info: torch.Tensor, Q, n: torch.Tensor, bound: float = BOUND) -> QseResult:
    """The float64 standard errors from the information (any device, the CPU included): ``info [b, K (K + 1) / 2]`` as ``q_info``
    writes it, ``Q [b, K]``, ``n [b]``.  The drop-one form of the module docstring, twice (c = K - 1 and c = 0).  On a GPU the blocks
    are inverted by ``nadm_snp_info_se``, on the CPU by ``pse._se_lapack``; torch's batched factorisation is NOT used on the device
    (``pse.se_from_info`` records why).  No component is dropped at the boundary; ``at_bound`` marks ``q <= bound`` and ``q >= 1 -
    bound``.  A sample with ``n = 0`` or a singular block is NaN throughout; K = 1 gives exactly 0."""
    if not 0.0 <= float(bound) < 0.5:
        raise RuntimeError("se_from_info: bound must be in [0, 0.5)")
    dev = info.device
    info = info.to(torch.float64)
    Qt = _as_f64(Q, dev)
    if Qt.dim() != 2 or info.dim() != 2:
        raise RuntimeError("se_from_info: info must be [b, K (K + 1) / 2] and Q [b, K]")
    b, K = Qt.shape
    n = torch.as_tensor(n).to(dev)
    if tuple(info.shape) != (b, n_pairs(K)) or tuple(n.shape) != (b,):
        raise RuntimeError(f"se_from_info: Q is [{b}, {K}]: info must be [{b}, {n_pairs(K)}] and n [{b}]")
    if K > MAX_K:
        raise RuntimeError(f"se_from_info: {TOO_WIDE}")
    at_bound = (Qt <= float(bound)) | (Qt >= 1.0 - float(bound))
    nan = torch.full((b, 1), float("nan"), dtype=torch.float64, device=dev)
    if K == 1:
        se = torch.where(n[:, None] > 0, torch.zeros_like(nan), nan)
    else:
        first = _se_free(drop_one(info, K, K - 1), n, K - 1)            # components 0 .. K - 2
        last = _se_free(drop_one(info, K, 0), n, K - 1)[:, -1:]         # component K - 1
        se = torch.cat([first, last], dim=1)
        se = torch.where(torch.isnan(se).any(dim=1, keepdim=True), nan, se)
    return QseResult(se, n.to(torch.int32), at_bound, None)


def q_se(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, bound: float = BOUND) -> QseResult:
    """Standard errors of ``Q [b, K]`` given ``P [M, K]`` for the rows ``idx`` of the packed device matrix (arguments as ``q_info``;
    ``bound``: ``se_from_info``).  Conditional on P (module docstring)."""
    info, n = q_info(xp, M, P, Q, idx)
    return se_from_info(info, Q, n, bound)


def concat(results: Sequence[QseResult]) -> QseResult:
    """The results of consecutive batches of rows as one."""
    return QseResult(torch.cat([r.se for r in results]), torch.cat([r.n for r in results]), torch.cat([r.at_bound for r in results]), None)


def write_se(path, se) -> None:
    """``se [N, K]`` in the ``.Q`` text format (``io.savetxt`` of the float32 values), NaN as ``nan``."""
    from .io import savetxt
    a = np.asarray(se.cpu() if torch.is_tensor(se) else se).astype(np.float32)
    if a.ndim != 2:
        raise RuntimeError("write_se: se must be a matrix [N, K]")
    a[np.isnan(a)] = np.float32("nan")                                  # one NaN: the positive quiet one, printed as `nan`
    savetxt(path, a)


def write_results(save_dir, name: str, results: Sequence[QseResult]) -> None:
    """``{save_dir}/{name}.{K}.Q_info_se`` per head (``.Q_se`` is the bootstrap's, which is not conditional on P)."""
    import os
    os.makedirs(save_dir, exist_ok=True)
    for r in results:
        write_se(os.path.join(save_dir, f"{name}.{int(r.se.shape[1])}.Q_info_se"), r.se)


def log_results(results: Sequence[QseResult], log) -> None:
    """Per K: the median standard error, the 95th percentile of the samples' largest one, how many samples have one above 0.1 (the
    five worst by index with their observed calls: the ones to look at), how many entries are at the bound and how many are NaN."""
    for r in results:
        N, K = r.se.shape
        se, n = r.se.cpu().numpy(), r.n.cpu().numpy()
        have = ~np.isnan(se)
        rows = have.all(axis=1)
        worst = np.where(rows, np.where(have, se, 0.0).max(axis=1), np.nan)
        med = float(np.median(se[have])) if have.any() else float("nan")
        p95 = float(np.percentile(worst[rows], 95)) if rows.any() else float("nan")
        wide = np.flatnonzero(rows & (np.nan_to_num(worst) > 0.1))
        log.info(f"Q standard errors given P (K={K}): median SE {med:.5f}; 95th percentile of a sample's largest SE {p95:.5f}; of {N} "
                 f"samples {len(wide)} have an SE above 0.1; of {N * K} entries {int(r.at_bound.sum())} at the bound (their SE is a "
                 f"detection limit), {int((~have).sum())} NaN")
        if len(wide):
            top = wide[np.argsort(-worst[wide], kind="stable")[:5]]
            log.info("    least certain samples (0-based index: largest SE, observed calls): " +
                     ", ".join(f"{int(i)}: {worst[i]:.3f}, {int(n[i])}" for i in top))
