"""What the analyses that work the pairs of a sample list block by block share (relate, king, fitcheck): the walk over the ``rows`` x
``rows`` blocks, the mirror of the computed blocks into a dense matrix, and the list of the pairs at or above a threshold."""
from __future__ import annotations

from typing import Optional

import torch

MAX_ROWS = 4096              # rows per block side at most: NADM_KINSHIP_ / NADM_IBD_ / NADM_KING_ / NADM_RESID_COR_MAX_ROWS


def block_rows(rows: int) -> int:
    """The refusal of a block side outside 1..MAX_ROWS, for the caller that has to refuse before it knows the list (fitcheck)."""
    rows = int(rows)
    if rows < 1 or rows > MAX_ROWS:
        raise RuntimeError("rows must be in 1..4096")
    return rows


def walk(N: int, rows: int, idx: Optional[torch.Tensor], device, ordered: bool = False):
    """``(rows, blocks)``: the block side in use, ``min(rows, N)`` (it sizes the one scratch buffer), and an iterator over the blocks of
    the pairs of ``N`` list positions, row band by row band: ``(a, ba, rows_a, b, bb, rows_b)``, the positions a.. against b.. and their
    matrix rows (those ``idx`` names, without one the positions themselves).  ``ordered``: every block; otherwise those with a <= b."""
    rows = min(block_rows(rows), N)

    def rows_of(s, b):
        return idx[s:s + b] if idx is not None else torch.arange(s, s + b, dtype=torch.int32, device=device)

    def blocks():
        for a in range(0, N, rows):
            ba = min(rows, N - a)
            ra = rows_of(a, ba)
            for b in range(0 if ordered else a, N, rows):
                bb = min(rows, N - b)
                yield a, ba, ra, b, bb, rows_of(b, bb)
    return rows, blocks()


def mirror(out: torch.Tensor, a: int, b: int, blk: torch.Tensor, upper: bool = False, swap=None) -> None:
    """Block (a, b), a <= b, of a walk into the dense ``out [..., N, N]``, and its transpose into (b, a).  ``upper``: of a diagonal
    block only the upper triangle counts and is mirrored (kinship: the two halves are different floating-point sums); otherwise a
    diagonal block goes in as computed.  ``swap``: the order of the leading planes in the transpose (king: het_a <-> het_b)."""
    ba, bb = blk.shape[-2:]
    if a == b and upper:
        blk = torch.triu(blk) + torch.triu(blk, 1).transpose(-1, -2)
    out[..., a:a + ba, b:b + bb] = blk
    if a != b:
        out[..., b:b + bb, a:a + ba] = (blk if swap is None else blk[swap]).transpose(-1, -2)


class PairList:
    """The pairs i < j with ``phi >= min_phi`` and their value in every further matrix, block by block; ``result``: by i, then j."""

    def __init__(self, N: int, min_phi: float):
        self.N, self.min_phi, self.cols = N, min_phi, None

    def add(self, a: int, b: int, phi: torch.Tensor, *more: torch.Tensor) -> None:
        keep = phi >= self.min_phi                           # (NaN compares false)
        if a == b:
            keep = torch.triu(keep, 1)
        ii, jj = torch.nonzero(keep, as_tuple=True)          # row-major: by i, then j
        vals = (ii + a, jj + b, phi[ii, jj]) + tuple(m[ii, jj] for m in more)
        if self.cols is None:
            self.cols = [[] for _ in vals]
        for c, v in zip(self.cols, vals):
            c.append(v)

    def result(self) -> tuple:
        i, j, *rest = (torch.cat(c) for c in self.cols)
        order = torch.argsort(i * self.N + j)                # the blocks of one row band come one after the other
        return tuple(v[order] for v in (i, j, *rest))
