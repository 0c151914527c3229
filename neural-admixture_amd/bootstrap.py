"""Bootstrap standard errors for Q (what ADMIXTURE's ``-B`` does, written as ``.Q_se`` / ``.Q_bias``): resample the SNPs with
replacement, refit, and take the spread of the refits.  Without it "12 % component 3" could mean 12 +- 1 or 12 +- 9.

A replicate is the masked block EM of project.py on the weighted likelihood ``sum_j w_j l_j``, ``w_j`` = how often SNP ``j`` was drawn:
no resampled copy of the matrix is made.  Only the Q step sees the weights (``nadm_project_q_w``, include/nadm.h); in the P step a SNP's
weight multiplies numerator and denominator alike and cancels, so ``nadm_project_p`` runs unchanged.  The draw is a fixed function of
(seed, replicate, block) that include/nadm.h states ("the bootstrap draw"): ``block_weights`` restates it on the host in numpy.

SNPs are drawn in blocks of ``block`` consecutive SNPs.  ``block = 1`` is ADMIXTURE's per-SNP bootstrap and assumes independent SNPs;
on data that was not LD-pruned a block of hundreds of SNPs keeps the error bar honest.

``bootstrap_q`` is the driver.  The centre is the block EM's own answer from the given one (the error bar belongs to the EM estimate);
every replicate starts at the centre, which rules out label switching -- and means that a replicate stopped at the round limit has
not moved as far as it would: its spread, and so the SE, comes out too SMALL (the same trap as cv's leak).
``BootResult.hit_limit`` says when that happened.  No standard error of P is computed: resampling SNPs says nothing about the
sampling error of one SNP's frequency.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np
import torch

from . import project

MIN_BLOCKS = 50      # fewer blocks than this: the spread of so few draws is itself noisy (a warning, not a refusal)
_DRAWS = 1 << 22     # draws per numpy pass of block_weights


class BootResult(NamedTuple):
    """One head's bootstrap: ``q_centre [N, k]`` the block EM's answer on the data as it is (float32, device); ``se [N, k]`` the
    standard deviation of the replicates' Q (n - 1 in the denominator) and ``bias [N, k]`` = their mean - ``q_centre`` (float64,
    device); ``centre_shift`` = max |q_centre - the Q given|; ``centre_rounds`` the rounds the centre's fit ran; ``rounds_run`` the
    rounds of every replicate; ``hit_limit``: the centre or a replicate ran all its ``rounds`` (a fit that met ``tol`` in its very
    last round counts too: the two cannot be told apart, and the warning is the safe side); ``n_blocks`` the blocks drawn from."""
    k: int
    q_centre: torch.Tensor
    se: torch.Tensor
    bias: torch.Tensor
    centre_shift: float
    centre_rounds: int
    rounds_run: List[int]
    hit_limit: bool
    n_blocks: int


def _mix32(x: np.ndarray) -> np.ndarray:
    """mix32 of include/nadm.h on a uint32 array (numpy's uint32 array arithmetic wraps)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _row_key(seed: int, i: int) -> np.uint32:
    lo, hi = np.array([seed & 0xFFFFFFFF], dtype=np.uint32), np.array([(seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return _mix32(_mix32(np.array([i & 0xFFFFFFFF], dtype=np.uint32) ^ hi) + lo + np.uint32(0x9E3779B9))[0]


def n_blocks(M: int, block: int) -> int:
    return -(-int(M) // int(block))


def block_counts(M: int, block: int, seed: int, rep: int) -> np.ndarray:
    """How often each of the ``nb = ceil(M / block)`` blocks is drawn in replicate ``rep``: int64 [nb], summing to nb."""
    M, block, seed, rep = int(M), int(block), int(seed), int(rep)
    if block < 1:
        raise RuntimeError("block must be >= 1")
    if not 0 < M <= 1 << 31:
        raise RuntimeError("M must be in 1..2^31")
    if not 0 <= seed < 1 << 64:
        raise RuntimeError("seed must be in 0..2^64-1")
    if not 0 <= rep < 1 << 31:
        raise RuntimeError("rep must be in 0..2^31-1")
    nb = n_blocks(M, block)
    if nb < 2:
        raise RuntimeError(f"the bootstrap needs at least 2 blocks of SNPs: {M} SNPs in blocks of {block} give {nb}")
    key = _row_key(seed, rep)
    cnt = np.zeros(nb, dtype=np.int64)
    for t0 in range(0, nb, _DRAWS):
        t = np.arange(t0, min(t0 + _DRAWS, nb), dtype=np.uint32)
        c = (_mix32(key ^ t).astype(np.uint64) * np.uint64(nb)) >> np.uint64(32)
        cnt += np.bincount(c.astype(np.int64), minlength=nb)
    if int(cnt.max()) > 255:
        raise RuntimeError(f"a block was drawn {int(cnt.max())} times; a weight must fit a byte (<= 255)")
    return cnt


def block_weights(M: int, block: int, seed: int, rep: int) -> np.ndarray:
    """The weights of replicate ``rep``: uint8 [M], ``w_j`` = how often block ``j // block`` was drawn (the last block may be short)."""
    return np.repeat(block_counts(M, block, seed, rep).astype(np.uint8), int(block))[:int(M)]


def bootstrap_q(xp: torch.Tensor, M: int, Ps: Sequence, Qs: Sequence, B: int = 200, block: int = 1, rounds: int = 50, tol: float = 1e-5,
                seed: int = 0) -> List[BootResult]:
    """Bootstrap standard errors of every head ``(Ps[h] [M, k_h], Qs[h] [N, k_h])`` (host or device, not modified) on the packed device
    matrix ``xp [N, ld]``.  The centre is ``project.polish(xp, M, Ps, Qs, rounds, tol)``; replicate ``r`` is
    ``project.polish(xp, M, P_centre, Q_centre, rounds, tol, weights=block_weights(M, block, seed, r))``; mean and sum of squared
    deviations of the replicates' Q are kept on the device in float64 (Welford), nothing of size B x N x K.  One ``BootResult`` per head."""
    B, block, rounds, M = int(B), int(block), int(rounds), int(M)
    if B < 2:
        raise RuntimeError("the bootstrap needs B >= 2 replicates")
    if rounds < 1:
        raise RuntimeError("rounds must be >= 1")
    if len(Ps) != len(Qs) or not Ps:
        raise RuntimeError("bootstrap_q needs one P and one Q per head")
    block_counts(M, block, seed, 0)                                    # the refusals of the draw, before any fit
    dev = xp.device
    Pc, Qc, _, _, done0 = project.polish(xp, M, Ps, Qs, rounds, tol)
    shift = [float((Qc[h].double() - torch.as_tensor(Qs[h]).to(dev).double()).abs().max()) for h in range(len(Ps))]
    mean = [torch.zeros(Q.shape, dtype=torch.float64, device=dev) for Q in Qc]
    m2 = [torch.zeros(Q.shape, dtype=torch.float64, device=dev) for Q in Qc]
    ran: List[int] = []
    for r in range(B):
        w = torch.from_numpy(block_weights(M, block, seed, r)).to(dev)
        _, Qr, _, _, done = project.polish(xp, M, Pc, Qc, rounds, tol, weights=w)
        ran.append(int(done))
        for h, Q in enumerate(Qr):
            d = Q.double() - mean[h]
            mean[h] += d / (r + 1)
            m2[h] += d * (Q.double() - mean[h])
    late = done0 >= rounds or any(x >= rounds for x in ran)
    nb = n_blocks(M, block)
    return [BootResult(int(Qc[h].shape[1]), Qc[h], torch.sqrt(m2[h] / (B - 1)), mean[h] - Qc[h].double(), shift[h], int(done0), list(ran),
                       bool(late), nb) for h in range(len(Ps))]


def log_results(results: Sequence[BootResult], log, rounds: int) -> None:
    """Per K the mean and the largest standard error and how far the given Q was from the EM estimate; a warning that names
    --boot_rounds for every K whose fits ran into the round limit, and one for a draw from fewer than MIN_BLOCKS blocks."""
    for r in results:
        log.info(f"Bootstrap SE (K={r.k}): mean {float(r.se.mean()):.5f}, max {float(r.se.max()):.5f} over {len(r.rounds_run)} replicates "
                 f"of {r.n_blocks} blocks; max |Q - EM estimate| {r.centre_shift:.5f}")
    late = [r for r in results if r.hit_limit]
    if late:
        log.info(f"    Warning: a fit for K = {', '.join(str(r.k) for r in late)} stopped at the limit of {int(rounds)} rounds, not at the "
                 "tolerance; replicates start at the estimate, so such a standard error is too small: raise --boot_rounds.")
    if results and results[0].n_blocks < MIN_BLOCKS:
        log.info(f"    Warning: only {results[0].n_blocks} blocks of SNPs to draw from (< {MIN_BLOCKS}); the standard errors are themselves "
                 "noisy: lower --block.")


def write_results(save_dir, name: str, results: Sequence[BootResult]) -> None:
    """``{save_dir}/{name}.{K}.Q_se`` and ``.Q_bias`` per head (ADMIXTURE's names), N x K in the ``.Q`` text format."""
    import os
    from .io import savetxt
    os.makedirs(save_dir, exist_ok=True)
    for r in results:
        savetxt(os.path.join(save_dir, f"{name}.{r.k}.Q_se"), r.se.float().cpu().numpy())
        savetxt(os.path.join(save_dir, f"{name}.{r.k}.Q_bias"), r.bias.float().cpu().numpy())
