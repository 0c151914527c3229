"""Relatedness: admixture-aware kinship (REAP, Thornton et al. 2012) from the packed genotype matrix, ``Q`` and one head's ``P``.

ADMIXTURE-type models assume unrelated samples; a family in the panel tends to come out as an ancestry component of its own.  The
REAP estimator checks that assumption with the individual-specific allele frequencies ``pi_ij = sum_k q_ik p_jk`` -- exactly the
``.Q`` and ``.P`` this project writes:

    phi_ab = sum_j (g_aj - 2 pi_aj)(g_bj - 2 pi_bj) / (4 sum_j sqrt(pi_aj (1 - pi_aj) pi_bj (1 - pi_bj)))

over the SNPs both samples were called at.  Expected values: 0 for an unrelated pair, 0.25 for parent-child and full sibs, 0.5 for
a duplicate or twin, (1 + f) / 2 for a sample with itself (f: its inbreeding coefficient).  Every block of pairs is one
``nadm_kinship`` call (include/nadm.h: two Gram products over the SNP axis on the matrix pipe, reproducible bit for bit).

``kinship`` is the dense form, ``kinship_pairs`` lists the related pairs holding one block at a time (any N),
``Engine.kinship`` runs the latter on the resident matrix with the engine's own P and the encoder's final Q.

A parent-child pair and a pair of full siblings both have phi = 0.25; what tells them apart are the probabilities k0, k1, k2 that the
pair shares 0, 1 or 2 alleles identical by descent (parent-child 0, 1, 0; full sibs 1/4, 1/2, 1/4).  ``ibd_pairs`` adds them to the
listed pairs with PC-Relate's estimators (Conomos et al. 2016) on the same pi: k2 from the dominance-coded genotypes, k0 of a
first-degree or closer pair from the opposite homozygotes it shows against those expected of a pair with no allele IBD, of a more
distant pair from 1 - 4 phi + k2.  Every block that holds a listed pair is one ``nadm_ibd`` call (include/nadm.h: four Gram products
on the matrix pipe, K <= 16).  The estimates are unconstrained: values slightly outside [0, 1] are normal, nothing is clipped.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, model_operands, n_rows, stream
from ._pairs import PairList, mirror, walk

ROWS = 1024                  # rows per block side of the dense and the pair form
MIN_PHI = 2.0 ** -4.5        # lower edge of third-degree relatives (0.0442)
# lower edges of the usual degree bands (KING's): duplicate / twin, first, second, third degree
BANDS = ((2.0 ** -1.5, "duplicate or twin"), (2.0 ** -2.5, "first degree"), (2.0 ** -3.5, "second degree"), (2.0 ** -4.5, "third degree"))
MAX_K = 16                   # widest head of the IBD sums (nadm_ibd)
TOO_WIDE = "K must be <= 16 for the IBD-sharing probabilities (a sample's Q row lives in its builder thread's registers beside the operand image)"
# k0 below this in the first-degree band: parent-offspring, otherwise full siblings.  A convention between the expected 0 and 1/4 (as
# the --warn of the fit check is), not a calibration
PO_MAX_K0 = 0.1
RELATIONS = ("duplicate or twin", "parent-offspring", "full siblings", "second degree", "third degree", "unrelated")


def kinship_scratch(ba: int, bb: int, M: int, device) -> torch.Tensor:
    n = int(lib.nadm_kinship_scratch_floats(ba, bb, M))
    if n <= 0:
        raise RuntimeError(f"kinship: a block of {ba} x {bb} rows over {M} SNPs is not supported (1..4096 rows a side)")
    return torch.empty(n, dtype=torch.float32, device=device)


def kinship_block(xp: torch.Tensor, M: int, Pp: torch.Tensor, k: int, idxA: Optional[torch.Tensor], QA: torch.Tensor,
                  idxB: Optional[torch.Tensor], QB: torch.Tensor, pimin: float = 0.0, scratch: Optional[torch.Tensor] = None):
    """One ``nadm_kinship`` call on the current stream: the rows ``idxA`` (int32, None: rows 0..ba) against the rows ``idxB`` of the
    packed device matrix ``xp [rows, ld]``; ``Pp [M, kp]`` padded (``pad_P``), ``QA [ba, >= kp]`` / ``QB [bb, >= kp]`` padded
    (``pad_Q``; row s belongs to ``idx[s]``).  Returns ``(num, den)`` float64 ``[ba, bb]`` and ``n`` int32 ``[ba, bb]``:
    ``phi = num / (4 den)``."""
    ba, bb = int(QA.shape[0]), int(QB.shape[0])
    check_packed(xp, idxA, ba)
    check_packed(xp, idxB, bb)
    for t in (Pp, QA, QB):
        if t.dtype != torch.float32 or t.dim() != 2 or t.device != xp.device or t.stride(1) != 1:
            raise RuntimeError("kinship_block: P and Q must be float32 matrices on the packed matrix's device")
    if not Pp.is_contiguous() or Pp.shape[0] != M:
        raise RuntimeError(f"kinship_block: P must be a contiguous [{M}, kp] matrix")
    if QA.stride(0) != QB.stride(0):
        raise RuntimeError("kinship_block: QA and QB must have the same row stride")
    dev = xp.device
    if scratch is None:
        scratch = kinship_scratch(ba, bb, M, dev)
    num = torch.empty((ba, bb), dtype=torch.float64, device=dev)
    den = torch.empty((ba, bb), dtype=torch.float64, device=dev)
    n = torch.empty((ba, bb), dtype=torch.int32, device=dev)
    check(lib.nadm_kinship(ptr(xp), xp.shape[1], ptr(idxA), ba, ptr(idxB), bb, M, ptr(Pp), k, Pp.shape[1], ptr(QA), ptr(QB),
                           QA.stride(0), pimin, ptr(num), ptr(den), ptr(n), ptr(scratch), stream()), "kinship")
    return num, den, n


def _phi(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / (4 den), NaN where den == 0 (no SNP both samples were called at)."""
    return torch.where(den != 0, num / (4.0 * den), torch.full_like(num, float("nan")))


def _blocks(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor], rows: int, pimin: float):
    """The ``rows`` x ``rows`` blocks of pairs with a <= b, row band by row band: yields ``(a, b, phi [ba, bb] float64, n [ba, bb]
    int32)`` of the rows a.. against the rows b.., one ``nadm_kinship`` call each."""
    check_packed(xp, idx, n_rows(xp, idx))                  # (ahead of the range of ``rows``, as the refusals have always come)
    rows, blocks = walk(n_rows(xp, idx), rows, idx, xp.device)
    _, K, Pp, Qp = model_operands(xp, M, idx, P, Q)
    scratch = kinship_scratch(rows, rows, M, xp.device)
    for a, ba, ia, b, bb, ib in blocks:
        num, den, nn = kinship_block(xp, M, Pp, K, ia, Qp[a:a + ba], ib, Qp[b:b + bb], pimin, scratch)
        yield a, b, _phi(num, den), nn


def kinship(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, rows: int = ROWS, pimin: float = 0.0):
    """Dense kinship of the rows ``idx`` (default: every row) of the packed device matrix ``xp [rows, ld]`` for the allele
    frequencies ``P [M, K]`` and ancestry fractions ``Q [N, K]`` (host or device; row s of Q belongs to ``idx[s]``).  Returns
    ``(phi float64 [N, N], n int32 [N, N])`` on xp's device: the blocks of ``rows`` x ``rows`` pairs with ib <= jb are computed,
    the rest mirrored (phi is symmetric bit for bit).  The diagonal holds (1 + f_a) / 2.  ``pimin`` drops the calls whose
    individual-specific frequency is outside [pimin, 1 - pimin]."""
    N = n_rows(xp, idx)
    phi = torch.empty((N, N), dtype=torch.float64, device=xp.device)
    n = torch.empty((N, N), dtype=torch.int32, device=xp.device)
    for a, b, ph, nn in _blocks(xp, M, P, Q, idx, rows, pimin):
        mirror(phi, a, b, ph, upper=True)                    # the upper triangle of a diagonal block is the one that counts
        mirror(n, a, b, nn, upper=True)
    return phi, n


def kinship_pairs(xp: torch.Tensor, M: int, P, Q, min_phi: float = MIN_PHI, rows: int = ROWS, pimin: float = 0.0,
                  idx: Optional[torch.Tensor] = None):
    """The related pairs: ``(i, j, phi, n, inbreeding)`` with ``i < j`` int64, ``phi`` float64 and ``n`` int32 of every pair with
    ``phi >= min_phi`` (default: the lower edge of third-degree relatives), ordered by i then j, and ``inbreeding`` float64 [N] =
    ``2 phi_aa - 1`` of every sample, all on xp's device.  One ``rows`` x ``rows`` block is held at a time: works at any N."""
    N = n_rows(xp, idx)
    inb = torch.empty(N, dtype=torch.float64, device=xp.device)
    pairs = PairList(N, min_phi)
    for a, b, ph, nn in _blocks(xp, M, P, Q, idx, rows, pimin):
        if a == b:
            inb[a:a + ph.shape[0]] = 2.0 * torch.diagonal(ph) - 1.0
        pairs.add(a, b, ph, nn)
    return pairs.result() + (inb,)


def band_counts(phi) -> list:
    """Number of pairs per degree band, ``[(label, lower edge, count)]``, from the phi of the listed pairs."""
    phi = np.asarray(phi, dtype=np.float64)
    out, upper = [], np.inf
    for edge, label in BANDS:
        out.append((label, edge, int(((phi >= edge) & (phi < upper)).sum())))
        upper = edge
    return out


def write_pairs(path, i, j, phi, n, *more) -> None:
    """One line ``i j phi n`` per pair, then one column per further integer vector of ``more``: integers as integers, phi with the 17
    digits that read back to the same float64."""
    ints = [np.asarray(v).tolist() for v in (n,) + more]
    with open(path, "w") as fb:
        for a, b, p, *cs in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), np.asarray(phi, dtype=np.float64).tolist(), *ints):
            fb.write(f"{a:d} {b:d} {p:.17g} " + " ".join(f"{c:d}" for c in cs) + "\n")


# ------------------------------------------------------------------------------------------------ IBD-sharing probabilities
def ibd_scratch(ba: int, bb: int, M: int, device) -> torch.Tensor:
    n = int(lib.nadm_ibd_scratch_floats(ba, bb, M))
    if n <= 0:
        raise RuntimeError(f"ibd: a block of {ba} x {bb} rows over {M} SNPs is not supported (1..4096 rows a side)")
    return torch.empty(n, dtype=torch.float32, device=device)


def ibd_block(xp: torch.Tensor, M: int, Pp: torch.Tensor, k: int, idxA: Optional[torch.Tensor], QA: torch.Tensor, fA: torch.Tensor,
              idxB: Optional[torch.Tensor], QB: torch.Tensor, fB: torch.Tensor, pimin: float = 0.0,
              scratch: Optional[torch.Tensor] = None):
    """One ``nadm_ibd`` call on the current stream: the operands of ``kinship_block`` and the inbreeding coefficients ``fA [ba]`` /
    ``fB [bb]`` (float32, row s belongs to ``idx[s]``).  Returns ``(k2num, k2den, exp0)`` float64 and ``ibs0`` int32, each
    ``[ba, bb]``: ``ibd_of`` turns them into k0, k1, k2.  K <= 16."""
    ba, bb = int(QA.shape[0]), int(QB.shape[0])
    check_packed(xp, idxA, ba)
    check_packed(xp, idxB, bb)
    for t in (Pp, QA, QB):
        if t.dtype != torch.float32 or t.dim() != 2 or t.device != xp.device or t.stride(1) != 1:
            raise RuntimeError("ibd_block: P and Q must be float32 matrices on the packed matrix's device")
    if not Pp.is_contiguous() or Pp.shape[0] != M:
        raise RuntimeError(f"ibd_block: P must be a contiguous [{M}, kp] matrix")
    if Pp.shape[1] > MAX_K:
        raise RuntimeError(f"ibd_block: {TOO_WIDE}")
    if QA.stride(0) != QB.stride(0):
        raise RuntimeError("ibd_block: QA and QB must have the same row stride")
    for f, b in ((fA, ba), (fB, bb)):
        if f.dtype != torch.float32 or f.dim() != 1 or f.device != xp.device or not f.is_contiguous() or f.numel() != b:
            raise RuntimeError("ibd_block: fA and fB must be contiguous float32 vectors of ba and bb entries on the packed matrix's device")
    dev = xp.device
    if scratch is None:
        scratch = ibd_scratch(ba, bb, M, dev)
    k2num, k2den, exp0 = (torch.empty((ba, bb), dtype=torch.float64, device=dev) for _ in range(3))
    ibs0 = torch.empty((ba, bb), dtype=torch.int32, device=dev)
    check(lib.nadm_ibd(ptr(xp), xp.shape[1], ptr(idxA), ba, ptr(idxB), bb, M, ptr(Pp), k, Pp.shape[1], ptr(QA), ptr(QB), QA.stride(0),
                       ptr(fA), ptr(fB), pimin, ptr(k2num), ptr(k2den), ptr(ibs0), ptr(exp0), ptr(scratch), stream()), "ibd")
    return k2num, k2den, exp0, ibs0


def ibd_of(phi: torch.Tensor, k2num: torch.Tensor, k2den: torch.Tensor, ibs0: torch.Tensor, exp0: torch.Tensor):
    """``(k0, k1, k2)`` float64 from the four sums and the pairs' kinship coefficient: k2 = k2num / k2den (NaN where k2den == 0);
    k0 = ibs0 / exp0 where phi >= 2^-2.5, the first-degree edge of ``BANDS`` (NaN where exp0 == 0), else 1 - 4 phi + k2;
    k1 = 1 - k0 - k2.  Unconstrained: nothing is clipped or renormalised."""
    phi, k2num, k2den, exp0 = (t.to(torch.float64) for t in (phi, k2num, k2den, exp0))
    nan = torch.full_like(k2num, float("nan"))
    k2 = torch.where(k2den != 0, k2num / k2den, nan)
    k0 = torch.where(phi >= BANDS[1][0], torch.where(exp0 != 0, ibs0.to(torch.float64) / exp0, nan), 1.0 - 4.0 * phi + k2)
    return k0, 1.0 - k0 - k2, k2


def ibd_pairs(xp: torch.Tensor, M: int, P, Q, min_phi: float = MIN_PHI, rows: int = ROWS, pimin: float = 0.0,
              idx: Optional[torch.Tensor] = None):
    """The related pairs with their IBD-sharing probabilities: ``(i, j, phi, n, inbreeding, k0, k1, k2, ibs0)``.  The first five are
    ``kinship_pairs``' own, bit for bit (it runs first and yields every sample's f = 2 phi_aa - 1; a sample without an observed call
    has none and enters with f = 0: every one of its calls is masked); then the blocks are walked again, a block that holds no listed
    pair is skipped, every other one is one ``nadm_ibd`` call, and the four sums are gathered at the listed pairs.  ``k0, k1, k2``
    float64 and ``ibs0`` int32, one per listed pair.  K <= 16."""
    if np.ndim(P) == 2 and int(np.shape(P)[1]) > MAX_K:
        raise RuntimeError(f"ibd_pairs: {TOO_WIDE}")
    i, j, phi, n, inb = kinship_pairs(xp, M, P, Q, min_phi, rows, pimin, idx)
    dev = xp.device
    f = torch.where(torch.isnan(inb), torch.zeros_like(inb), inb).to(torch.float32)
    rows, blocks = walk(n_rows(xp, idx), rows, idx, dev)
    _, K, Pp, Qp = model_operands(xp, M, idx, P, Q)
    sums = [torch.zeros(i.numel(), dtype=torch.float64, device=dev) for _ in range(3)]
    ibs0 = torch.zeros(i.numel(), dtype=torch.int32, device=dev)
    ia_blk, jb_blk = torch.div(i, rows, rounding_mode="floor"), torch.div(j, rows, rounding_mode="floor")
    listed = set(zip(ia_blk.tolist(), jb_blk.tolist()))       # the blocks that hold a listed pair (i < j: a <= b)
    scratch = ibd_scratch(rows, rows, M, dev) if listed else None
    for a, ba, ia, b, bb, ib in blocks:
        if (a // rows, b // rows) not in listed:
            continue
        got = ibd_block(xp, M, Pp, K, ia, Qp[a:a + ba], f[a:a + ba], ib, Qp[b:b + bb], f[b:b + bb], pimin, scratch)
        at = torch.nonzero((ia_blk == a // rows) & (jb_blk == b // rows), as_tuple=True)[0]
        ii, jj = i[at] - a, j[at] - b
        for out, blk in zip(sums + [ibs0], got):
            out[at] = blk[ii, jj]
    k2num, k2den, exp0 = sums
    return (i, j, phi, n, inb) + ibd_of(phi, k2num, k2den, ibs0, exp0) + (ibs0,)


def relation(phi, k0, po_k0: float = PO_MAX_K0) -> list:
    """A label per pair from its kinship coefficient and k0: the bands of ``BANDS``, the first-degree one split into
    "parent-offspring" (k0 < ``po_k0``) and "full siblings" (the rest, a NaN k0 included); "unrelated" below the last band.
    The default ``PO_MAX_K0`` = 0.1 is a convention between the expected 0 and 1/4, not a calibration."""
    out = []
    for p, z in zip(np.asarray(phi, dtype=np.float64).reshape(-1).tolist(), np.asarray(k0, dtype=np.float64).reshape(-1).tolist()):
        label = next((name for edge, name in BANDS if p >= edge), "unrelated")
        if label == "first degree":
            label = "parent-offspring" if z < po_k0 else "full siblings"
        out.append(label)
    return out


def relation_counts(labels) -> list:
    """``[(label, count)]`` over ``RELATIONS``, in their order."""
    labels = list(labels)
    return [(name, labels.count(name)) for name in RELATIONS]


def write_ibd(path, i, j, phi, n, k0, k1, k2, ibs0, labels) -> None:
    """One line ``i j phi n k0 k1 k2 ibs0 relation`` per listed pair: integers as integers, floats with the 17 digits that read back
    to the same float64, the label with its spaces replaced by ``_``."""
    cols = [np.asarray(v).tolist() for v in (i, j)] + [np.asarray(phi, dtype=np.float64).tolist(), np.asarray(n).tolist()]
    cols += [np.asarray(v, dtype=np.float64).tolist() for v in (k0, k1, k2)] + [np.asarray(ibs0).tolist(), list(labels)]
    with open(path, "w") as fb:
        for a, b, p, c, z0, z1, z2, s0, lab in zip(*cols):
            fb.write(f"{a:d} {b:d} {p:.17g} {c:d} {z0:.17g} {z1:.17g} {z2:.17g} {s0:d} {lab.replace(' ', '_')}\n")
