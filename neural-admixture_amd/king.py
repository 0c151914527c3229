"""Relatedness before the fit: KING-robust kinship (Manichaikul et al. 2010) from the packed genotype matrix alone, the maximal set of
unrelated samples, and the selection of samples.

``relate`` (REAP) needs a run's ``.Q`` and ``.P``, which were estimated with the relatives still in the panel.  KING-robust needs no
allele frequencies and no model: over the SNPs both samples were called at,

    phi_ab = 1/2 - (het_a + het_b - 2 hethet + 4 ibs0) / (4 min(het_a, het_b))

from five integer counts per pair (include/nadm.h, ``nadm_king``: a Gram product of 0 / 1 indicators over the SNP axis on the int8
matrix pipe, int32 sums, exact and reproducible bit for bit).  Expected: 0.5 duplicate, 0.25 first degree, 0.125 second degree, 0
unrelated within a population, negative between populations.  This is what ``plink2 --king-cutoff`` does in front of ADMIXTURE-type
tools: compute the kinship, keep a maximal set without a pair above a cutoff, fit on it and project the rest.

``king_block`` is one call, ``king`` the dense form, ``king_pairs`` lists the related pairs holding one block at a time (any N),
``unrelated_set`` picks the samples to keep (host, deterministic), ``select_samples`` is what ``--keep`` / ``--remove`` of the command
line apply right after the read, ``Engine.king`` runs ``king_pairs`` on the resident matrix.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import check_packed, n_rows, stream
from ._pairs import PairList, mirror, walk

ROWS = 1024                  # rows per block side of the dense and the pair form
MIN_PHI = 2.0 ** -3.5        # lower edge of second-degree relatives (0.0884): plink2's customary --king-cutoff


def king_scratch(ba: int, bb: int, M: int, device) -> torch.Tensor:
    n = int(lib.nadm_king_scratch_ints(ba, bb, M))
    if n <= 0:
        raise RuntimeError(f"king: a block of {ba} x {bb} rows over {M} SNPs is not supported (1..4096 rows a side, M < 2^31)")
    return torch.empty(n, dtype=torch.int32, device=device)


def king_block(xp: torch.Tensor, M: int, idxA: Optional[torch.Tensor], idxB: Optional[torch.Tensor], ba: int, bb: int,
               scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``nadm_king`` call on the current stream: the rows ``idxA`` (int32, None: rows 0..ba) against the rows ``idxB`` of the packed
    device matrix ``xp [rows, ld]``.  Returns the int32 ``[5, ba, bb]`` counts ``n, hethet, ibs0, het_a, het_b``."""
    ba, bb = int(ba), int(bb)
    check_packed(xp, idxA, ba, "king_block")
    check_packed(xp, idxB, bb, "king_block")
    if scratch is None:
        scratch = king_scratch(ba, bb, int(M), xp.device)
    counts = torch.empty((5, ba, bb), dtype=torch.int32, device=xp.device)
    check(lib.nadm_king(ptr(xp), xp.shape[1], ptr(idxA), ba, ptr(idxB), bb, int(M), ptr(counts), ptr(scratch), stream()), "king")
    return counts


def phi_from_counts(counts):
    """float64 phi from the ``[5, ...]`` counts (numpy array or torch tensor; the result is of the same kind): the numerator as an
    integer, ONE division in float64, NaN where ``min(het_a, het_b) == 0``."""
    if torch.is_tensor(counts):
        c = counts.to(torch.int64)
        f64 = lambda v: v.to(torch.float64)                   # noqa: E731
        where, minimum, nan = torch.where, torch.minimum, torch.full(c.shape[1:], float("nan"), dtype=torch.float64, device=c.device)
    else:
        c = np.asarray(counts).astype(np.int64)
        f64 = lambda v: v.astype(np.float64)                  # noqa: E731
        where, minimum, nan = np.where, np.minimum, np.full(c.shape[1:], np.nan)
    hethet, ibs0, het_a, het_b = c[1], c[2], c[3], c[4]
    num, mn = het_a + het_b - 2 * hethet + 4 * ibs0, minimum(het_a, het_b)
    ok = mn > 0
    return where(ok, 0.5 - f64(num) / f64(where(ok, 4 * mn, 1)), nan)


def _blocks(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor], rows: int):
    """The ``rows`` x ``rows`` blocks of pairs with a <= b, row band by row band: yields ``(a, b, counts [5, ba, bb] int32)`` of the
    rows a.. against the rows b.., one ``nadm_king`` call each."""
    N = n_rows(xp, idx)
    check_packed(xp, idx, N, "king")
    rows, blocks = walk(N, rows, idx, xp.device)
    scratch = king_scratch(rows, rows, int(M), xp.device)
    for a, ba, ia, b, bb, ib in blocks:
        yield a, b, king_block(xp, M, ia, ib, ba, bb, scratch)


def king(xp: torch.Tensor, M: int, idx: Optional[torch.Tensor] = None, rows: int = ROWS):
    """Dense KING-robust kinship of the rows ``idx`` (default: every row) of the packed device matrix ``xp [rows, ld]``.  Returns
    ``(phi float64 [N, N], counts int32 [5, N, N])`` on xp's device: the blocks of ``rows`` x ``rows`` pairs with a <= b are computed,
    the rest mirrored (``het_a`` and ``het_b`` exchanged in the mirror; phi is symmetric bit for bit)."""
    N = n_rows(xp, idx)
    counts = torch.empty((5, N, N), dtype=torch.int32, device=xp.device)
    for a, b, c in _blocks(xp, M, idx, rows):
        mirror(counts, a, b, c, swap=[0, 1, 2, 4, 3])
    return phi_from_counts(counts), counts


def king_pairs(xp: torch.Tensor, M: int, min_phi: float = MIN_PHI, rows: int = ROWS, idx: Optional[torch.Tensor] = None):
    """The related pairs: ``(i, j, phi, n, hethet, ibs0)`` with ``i < j`` int64, ``phi`` float64 and the counts int32 of every pair
    with ``phi >= min_phi`` (default: the lower edge of second-degree relatives), ordered by i then j, on xp's device.  One ``rows`` x
    ``rows`` block is held at a time: works at any N."""
    N = n_rows(xp, idx)
    pairs = PairList(N, min_phi)
    for a, b, c in _blocks(xp, M, idx, rows):
        pairs.add(a, b, phi_from_counts(c), c[0], c[1], c[2])
    return pairs.result()


def unrelated_set(N: int, i, j) -> np.ndarray:
    """bool ``[N]``: a maximal set of samples without a related pair, from the related pairs ``(i[k], j[k])``.  Deterministic:
      1. while related pairs remain, the sample with the most remaining related partners goes, the highest index on a tie;
      2. then the removed samples are gone through in ascending index, and every one without a related partner among the kept
         ones comes back.
    No kept pair is related, and every removed sample is related to a kept one."""
    N = int(N)
    i = np.asarray(i.cpu() if torch.is_tensor(i) else i, dtype=np.int64).reshape(-1)
    j = np.asarray(j.cpu() if torch.is_tensor(j) else j, dtype=np.int64).reshape(-1)
    if i.shape != j.shape or (len(i) and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= N)):
        raise RuntimeError(f"unrelated_set: i and j must be index vectors of one length with values in 0..{N - 1}")
    adj = [set() for _ in range(N)]
    for a, b in zip(i.tolist(), j.tolist()):
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    keep = np.ones(N, dtype=bool)
    deg = np.asarray([len(s) for s in adj], dtype=np.int64)
    removed = []
    while deg.max(initial=0) > 0:
        v = int(N - 1 - np.argmax(deg[::-1]))                # the highest index among the largest degrees
        keep[v] = False
        removed.append(v)
        for u in adj[v]:
            if keep[u]:
                deg[u] -= 1
        deg[v] = 0
    for v in sorted(removed):
        if not any(keep[u] for u in adj[v]):
            keep[v] = True
    return keep


def select_samples(data, keep):
    """The samples ``keep`` (bool ``[N]``) of ``data`` (:class:`~.io.PackedGenotypes`) as a PackedGenotypes of ``keep.sum()`` samples in
    file order, on the device the input is on.  The orientation is decided again on the subset by the reader's rule (flip 0 <-> 2 when
    the mean code of the file's own genotypes, 3s included, is >= 1), so the result is byte for byte what ``read_bed_packed`` returns
    for a BED that holds only those samples; ``flipped`` says whether the result is flipped against the file."""
    from .io import PackedGenotypes
    from .ld import snp_counts
    if not hasattr(data, "packed") or not torch.is_tensor(data.packed):
        raise RuntimeError("select_samples: data must be a PackedGenotypes")
    keep = np.asarray(keep.cpu() if torch.is_tensor(keep) else keep)
    if keep.dtype != np.bool_ or keep.shape != (data.N,):
        raise RuntimeError(f"select_samples: keep must be a bool vector with one entry per sample ({data.N})")
    N_out = int(keep.sum())
    if N_out < 1:
        raise RuntimeError("select_samples: keep selects no sample")
    home = data.packed.device
    if home.type != "cuda" and not torch.cuda.is_available():
        raise RuntimeError("select_samples: the selection runs on a ROCm GPU (no CPU fallback)")
    xp = data.packed if home.type == "cuda" else data.packed.to("cuda:0")
    if xp.dtype != torch.uint8 or xp.dim() != 2 or not xp.is_contiguous() or xp.shape[0] != data.N:
        raise RuntimeError("select_samples: data.packed must be a contiguous uint8 [N, ld] matrix")
    with torch.cuda.device(xp.device):
        ridx = torch.from_numpy(np.nonzero(keep)[0].astype(np.int32)).to(xp.device)
        c = snp_counts(xp, data.M, ridx).to(torch.int64).sum(dim=0).cpu()
        n_obs, S = int(c[0]), int(c[1])
        if data.flipped:                                     # the file's own codes: 2 - g at every observed call
            S = 2 * n_obs - S
        total = S + 3 * (N_out * data.M - n_obs)             # the reader's sum of codes, 3s included
        flip_file = total >= N_out * data.M                  # mean >= 1
        rows = xp.index_select(0, ridx.to(torch.int64))
        every = torch.arange(data.M, dtype=torch.int64, device=xp.device)
        out = torch.empty_like(rows)
        check(lib.nadm_select_snps(ptr(rows), rows.shape[1], N_out, ptr(every), data.M, int(bool(flip_file) != bool(data.flipped)),
                                   ptr(out), out.shape[1], stream()), "select_snps")
        if home.type != "cuda":
            out = out.to(home)
        else:
            torch.cuda.current_stream().synchronize()        # rows and every are freed on return
    return PackedGenotypes(out, N_out, data.M, bool(flip_file))
