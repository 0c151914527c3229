"""Hardy-Weinberg proportions GIVEN ANCESTRY: a per-SNP score test from the packed genotype matrix, ``Q`` and one head's ``P``.

The admixture likelihood says a genotype is binomial(2, pi_ij) with the individual-specific allele frequency ``pi_ij = sum_k q_ik
p_jk``: Hardy-Weinberg proportions given the sample's ancestry.  SNPs that break it -- heterozygote drop-out, paralogs called as one
locus, batch effects -- bias ``P`` and ``Q``.  The plain test (plink ``--hwe``) cannot find them in a structured panel: the Wahlund
effect makes it reject good SNPs.  With a per-SNP inbreeding coefficient ``F``,

    P(g = 0) = (1 - pi)^2 + F pi (1 - pi)     P(g = 1) = 2 pi (1 - pi) (1 - F)     P(g = 2) = pi^2 + F pi (1 - pi)

the score of ``F`` at ``F = 0`` is ``t = (1 - pi) / pi`` for g = 2, ``-1`` for g = 1 and ``pi / (1 - pi)`` for g = 0: mean 0 and
variance 1 for every pi, and uncorrelated with the score of pi, so that an estimated ``P`` needs no correction.  Over the observed
calls of a SNP, ``Z = sum t / sqrt(n)`` is N(0, 1) under the model (positive: excess homozygotes) and ``F = sum t / n`` estimates
the inbreeding coefficient.  For rare variants (pi near 0 or 1) ``t`` is heavy-tailed and the normal approximation as poor as a
chi-square HWE test's; ``pimin`` drops those calls.

``snp_hwe_sums`` is one ``nadm_snp_hwe`` call (include/nadm.h: reproducible bit for bit), ``snp_hwe`` forms the statistics in
float64, ``hwe_keep`` the keep-list, ``Engine.snp_hwe`` runs it on the resident matrix with the engine's own P and the encoder's
final Q.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import model_operands, stream

EPS = 1e-6           # clip of pi and of 1 - pi: the projection's (project.EPS)
ALPHA = 1e-6         # plink's customary --hwe threshold


class HweResult(NamedTuple):
    """Per SNP, on the packed matrix's device: ``Z``, ``F``, ``Fhet`` (= 1 - Hobs / Hexp), the two-sided ``p`` and ``Hexp`` as
    float64, ``n`` and ``Hobs`` as int32.  ``Z``, ``F`` and ``p`` are NaN where ``n = 0``, ``Fhet`` where ``Hexp = 0``."""
    Z: torch.Tensor
    F: torch.Tensor
    Fhet: torch.Tensor
    p: torch.Tensor
    n: torch.Tensor
    Hobs: torch.Tensor
    Hexp: torch.Tensor


def snp_hwe_sums(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, pimin: float = 0.0, eps: float = EPS):
    """One ``nadm_snp_hwe`` call on the current stream for the rows ``idx`` (int32, default: every row) of the packed device matrix
    ``xp [rows, ld]``, the allele frequencies ``P [M, K]`` and the ancestry fractions ``Q [b, K]`` (host or device; row s of Q belongs
    to ``idx[s]``).  Returns ``(U, Hexp, n, Hobs)`` on xp's device: float64, float64, int32, int32 ``[M]``."""
    M = int(M)
    b, K, Pp, Qp = model_operands(xp, M, idx, P, Q, what="snp_hwe")
    n_scr = int(lib.nadm_snp_hwe_scratch_floats(b, M))
    if n_scr <= 0:
        raise RuntimeError(f"snp_hwe: a block of {b} rows over {M} SNPs is not supported")
    dev = xp.device
    scratch = torch.empty(n_scr, dtype=torch.float32, device=dev)
    U = torch.empty(M, dtype=torch.float64, device=dev)
    Hexp = torch.empty(M, dtype=torch.float64, device=dev)
    n = torch.empty(M, dtype=torch.int32, device=dev)
    Hobs = torch.empty(M, dtype=torch.int32, device=dev)
    check(lib.nadm_snp_hwe(ptr(xp), xp.shape[1], ptr(idx), b, M, ptr(Qp), Qp.stride(0), K, Pp.shape[1], ptr(Pp), float(eps), float(pimin),
                           ptr(U), ptr(Hexp), ptr(n), ptr(Hobs), ptr(scratch), stream()), "snp_hwe")
    return U, Hexp, n, Hobs


def stats_from_sums(U: torch.Tensor, Hexp: torch.Tensor, n: torch.Tensor, Hobs: torch.Tensor) -> HweResult:
    """The float64 statistics from the four sums (any device): the only divisions by sums."""
    nan = torch.full_like(U, float("nan"))
    nf = n.to(torch.float64)
    seen = n > 0
    Z = torch.where(seen, U / torch.sqrt(nf), nan)
    F = torch.where(seen, U / nf, nan)
    Fhet = torch.where(Hexp > 0, 1.0 - Hobs.to(torch.float64) / Hexp, nan)
    p = torch.special.erfc(Z.abs() / math.sqrt(2.0))
    return HweResult(Z, F, Fhet, p, n, Hobs, Hexp)


def snp_hwe(xp: torch.Tensor, M: int, P, Q, idx: Optional[torch.Tensor] = None, pimin: float = 0.0, eps: float = EPS) -> HweResult:
    """The score test of Hardy-Weinberg proportions given ancestry for every SNP of the packed device matrix (arguments as
    ``snp_hwe_sums``): ``Z = U / sqrt(n)``, ``F = U / n``, ``Fhet = 1 - Hobs / Hexp`` and the two-sided ``p = erfc(|Z| / sqrt 2)``."""
    return stats_from_sums(*snp_hwe_sums(xp, M, P, Q, idx, pimin, eps))


def hwe_keep(p, alpha: float = ALPHA, n=None) -> np.ndarray:
    """bool ``[M]`` on the host: the SNPs with ``p >= alpha``, or with no observed call (``n = 0``, or a NaN ``p`` where ``n`` is not
    given) -- a SNP nobody observes carries no evidence and is kept."""
    p = np.asarray(p.cpu() if torch.is_tensor(p) else p, dtype=np.float64)
    none = np.isnan(p) if n is None else (np.asarray(n.cpu() if torch.is_tensor(n) else n) == 0)
    if none.shape != p.shape:
        raise RuntimeError("hwe_keep: p and n must have one entry per SNP")
    with np.errstate(invalid="ignore"):
        return (p >= float(alpha)) | none


def write_table(path, ids, res) -> None:
    """One line ``id n het_obs het_exp F Z p`` per SNP in the order given: integers as integers, floats with the 17 digits that
    read back to the same float64, NaN as ``nan``.  ``F`` is the score estimate ``U / n``."""
    cols = [np.asarray(a.cpu() if torch.is_tensor(a) else a) for a in (res.n, res.Hobs, res.Hexp, res.F, res.Z, res.p)]
    if any(len(c) != len(ids) for c in cols):
        raise RuntimeError("write_table: one ID per SNP is needed")
    n, ho, he, F, Z, p = (c.tolist() for c in cols)
    with open(path, "w") as fb:
        for row in zip(ids, n, ho, he, F, Z, p):
            fb.write("{} {:d} {:d} {:.17g} {:.17g} {:.17g} {:.17g}\n".format(*row))
