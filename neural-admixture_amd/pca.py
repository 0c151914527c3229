"""Principal components of the standardised genotype matrix, as ``smartpca``, ``plink --pca`` and FastPCA compute them, straight from
the packed matrix in HBM.

With ``f_j = S_j / (2 n_j)`` the allele frequency of SNP ``j`` among its ``n_j`` observed calls (``nadm_snp_counts``), ``c_j = 2 f_j``
and ``s_j = 1 / sqrt(2 f_j (1 - f_j))`` -- 0 for a SNP nobody observed, a monomorphic one and one whose minor-allele frequency is
below ``maf`` -- the matrix is ``Z_ij = o_ij (g_ij - c_j) s_j``: centred, scaled, a missing call at the mean.  ``M_eff`` SNPs have
``s_j > 0``, and the spectrum reported is that of the GRM ``Z Z^T / M_eff``.  ``Z`` is never formed: the randomised subspace
iteration of FastPCA (Galinsky et al. 2016; ``iters = 10`` is that paper's default, not tuned here) needs ``Z W`` and ``Z^T Q`` only,
and those are the two observed-calls pair products of include/nadm.h (``nadm_obs_project`` / ``nadm_obs_project_t``) with the
centring and scaling folded into their fp32 operands:

    Z W   = obs_project(W1 = s o W, W2 = -c o s o W)
    Z^T Q = s o (O1 - c o O2),   (O1, O2) = obs_project_t(Q)

``svd.RSVD`` is not this: it restates the reference's initialisation (raw codes, no centring, no scaling, missing = 3).

The orthonormalisations run on the host with numpy's QR and the small eigenproblem with numpy's ``eigh``, both in float64; the Gram
matrix of the last product comes from ``svd.gram64``.  No device BLAS or solver is called, for the reason ``svd.py`` gives."""
from __future__ import annotations

import logging
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import lib, check, ptr
from ._packed import stream
from .ld import _rows as _shape, snp_counts        # (the checks of the matrix, its gather list and M that the LD kernels' callers make)

log = logging.getLogger(__name__)

MAX_COLUMNS = 32             # columns of one product (include/nadm.h: CP in {16, 32})


class PcaResult(NamedTuple):
    eigenvalues: np.ndarray      # float64 [pcs], descending: of Z Z^T / M_eff
    eigenvectors: np.ndarray     # float64 [N, pcs], unit norm, the entry of largest magnitude positive
    M_eff: int                   # SNPs with s_j > 0
    explained: np.ndarray        # float64 [pcs]: eigenvalue / trace(Z Z^T / M_eff)
    total: float                 # trace(Z Z^T) / M_eff, from the counts


def check_args(pcs: int, oversample: int, iters: int, maf: float) -> int:
    """The refusals that need neither data nor a GPU; returns ``L = pcs + oversample``."""
    pcs, oversample, iters = int(pcs), int(oversample), int(iters)
    if pcs < 1:
        raise RuntimeError("pca: pcs must be >= 1")
    if oversample < 0:
        raise RuntimeError("pca: oversample must be >= 0")
    if pcs + oversample > MAX_COLUMNS:
        raise RuntimeError(f"pca: pcs + oversample must be <= {MAX_COLUMNS} (the columns of one product), got {pcs} + {oversample}")
    if iters < 0:
        raise RuntimeError("pca: iters must be >= 0")
    if not 0.0 <= float(maf) < 0.5:
        raise RuntimeError("pca: maf must be in [0, 0.5)")
    return pcs + oversample


def pad_columns(L: int) -> int:
    """The column stride of a product of ``L`` columns: 16 or 32."""
    if not 1 <= int(L) <= MAX_COLUMNS:
        raise RuntimeError(f"the products take 1..{MAX_COLUMNS} columns, got {int(L)}")
    return 16 if int(L) <= 16 else 32


def standardise(cnt, maf: float = 0.0):
    """Per SNP from ``nadm_snp_counts``' ``[M, 3]`` (observed calls, their sum, their sum of squares), in float64 on the host:
    ``(c [M], s [M], M_eff, total)`` -- the centre ``2 f``, the scale ``1 / sqrt(2 f (1 - f))`` or 0 (nobody observed, monomorphic,
    minor-allele frequency below ``maf``), the number of SNPs with ``s > 0`` and ``sum_ij Z_ij^2 / M_eff``.  Refuses ``M_eff == 0``."""
    cn = np.asarray(cnt.cpu() if torch.is_tensor(cnt) else cnt, dtype=np.int64)
    if cn.ndim != 2 or cn.shape[1] != 3:
        raise RuntimeError("standardise: counts must be [M, 3]")
    n, S, S2 = (cn[:, i].astype(np.float64) for i in range(3))
    ok = cn[:, 0] > 0
    f = np.zeros(len(n), dtype=np.float64)
    f[ok] = S[ok] / (2.0 * n[ok])
    use = ok & (cn[:, 1] > 0) & (cn[:, 1] < 2 * cn[:, 0]) & (np.minimum(f, 1.0 - f) >= float(maf))
    c = 2.0 * f
    s = np.zeros(len(n), dtype=np.float64)
    s[use] = 1.0 / np.sqrt(2.0 * f[use] * (1.0 - f[use]))
    m_eff = int(use.sum())
    if m_eff == 0:
        raise RuntimeError("pca: no SNP is left to standardise: every SNP is unobserved, monomorphic or below the minor-allele "
                           f"frequency {float(maf):g}")
    # sum_i o (g - c)^2 = S2 - S^2 / n with c = S / n
    total = float((s[use] ** 2 * (S2[use] - S[use] ** 2 / n[use])).sum() / m_eff)
    return c, s, m_eff, total


def _operand(t: torch.Tensor, rows: int, CP: int, what: str) -> None:
    if t.dtype != torch.float32 or tuple(t.shape) != (rows, CP) or not t.is_contiguous() or t.device.type != "cuda":
        raise RuntimeError(f"{what} must be a contiguous float32 [{rows}, {CP}] matrix on the GPU")


def obs_project(xp: torch.Tensor, M: int, W1: torch.Tensor, W2: torch.Tensor, C: int, idx: Optional[torch.Tensor] = None,
                scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Y[s, c] = sum_j (g o)_sj W1[j, c] + o_sj W2[j, c]`` over the rows ``idx`` (int32, default: every row) of the packed device
    matrix ``xp [rows, ld]``: float32 ``[b, CP]``.  ``W1, W2`` float32 ``[M, CP]`` on xp's device, CP 16 or 32, ``C`` columns in use
    (pad columns zero)."""
    b = _shape(xp, M, idx, "obs_project")
    CP = int(W1.shape[1]) if W1.dim() == 2 else 0
    _operand(W1, int(M), CP, "obs_project: W1")
    _operand(W2, int(M), CP, "obs_project: W2")
    need = int(lib.nadm_obs_project_scratch_floats(b, int(M), CP))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(max(need, 4), dtype=torch.float32, device=xp.device)
    Y = torch.empty((b, CP), dtype=torch.float32, device=xp.device)
    check(lib.nadm_obs_project(ptr(xp), xp.shape[1], ptr(idx), b, int(M), ptr(W1), ptr(W2), int(C), CP, ptr(Y), ptr(scratch), stream()),
          "obs_project")
    return Y


def obs_project_t(xp: torch.Tensor, M: int, Yin: torch.Tensor, C: int, idx: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None):
    """``O1[j, c] = sum_s (g o)_sj Yin[s, c]`` and ``O2[j, c] = sum_s o_sj Yin[s, c]`` over the rows ``idx``: two float32 ``[M, CP]``.
    ``Yin`` float32 ``[b, CP]`` on xp's device (row s belongs to idx[s]), CP 16 or 32, ``C`` columns in use (pad columns zero)."""
    b = _shape(xp, M, idx, "obs_project_t")
    CP = int(Yin.shape[1]) if Yin.dim() == 2 else 0
    _operand(Yin, b, CP, "obs_project_t: Yin")
    need = int(lib.nadm_obs_project_t_scratch_floats(b, int(M), CP))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(max(need, 4), dtype=torch.float32, device=xp.device)
    O1 = torch.empty((int(M), CP), dtype=torch.float32, device=xp.device)
    O2 = torch.empty((int(M), CP), dtype=torch.float32, device=xp.device)
    check(lib.nadm_obs_project_t(ptr(xp), xp.shape[1], ptr(idx), b, int(M), ptr(Yin), int(C), CP, ptr(O1), ptr(O2), ptr(scratch),
                                 stream()), "obs_project_t")
    return O1, O2


def omega(M: int, L: int, seed: int) -> np.ndarray:
    """The start of the iteration: float32 ``[M, L]`` standard normals from ``np.random.default_rng(seed)``."""
    return np.random.default_rng(seed).standard_normal(size=(int(M), int(L)), dtype=np.float32)


def orient(U: np.ndarray) -> np.ndarray:
    """Columns at unit norm, the entry of largest magnitude positive."""
    U = U / np.linalg.norm(U, axis=0, keepdims=True)
    big = U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])]
    return U * np.where(big < 0, -1.0, 1.0)


def subspace_pcs(times, t_times, M: int, L: int, CP: int, pcs: int, iters: int, seed: int, dev, m_eff):
    """The randomised subspace iteration shared by ``pca`` and ``residpca.resid_pca``, on the two operators of a matrix ``A [b, M]``:
    ``times(W)`` takes float64 ``[M, CP]`` on the device (pad columns 0) to ``A W`` as host float64 ``[b, L]``, ``t_times(Q)`` takes
    host float64 ``[b, <= L]`` to ``A^T Q`` as float64 ``[M, CP]`` on the device (pad columns 0).  Start ``omega(M, L, seed)``,
    ``iters`` rounds with numpy's QR in float64 on the host between the products, then a Rayleigh-Ritz step in float64: the Gram
    matrix of the last product through ``svd.gram64``, divided by ``m_eff`` (a number, or a callable asked once the last product has
    run).  Returns ``(eigenvalues [pcs] of A A^T / m_eff, descending and >= 0, eigenvectors [b, pcs] oriented)``."""
    from .svd import gram64

    def orth(Y):
        return np.linalg.qr(Y, mode="reduced")[0]

    W0 = torch.zeros((M, CP), dtype=torch.float64, device=dev)
    W0[:, :L] = torch.from_numpy(omega(M, L, seed)).to(dev)
    Y = times(W0)
    for _ in range(iters):
        Y = times(t_times(orth(Y)))
    Q = orth(Y)                                          # [b, min(b, L)]
    Bt = t_times(Q)
    T = gram64(Bt[:, :Q.shape[1]]).cpu().numpy() / (m_eff() if callable(m_eff) else m_eff)
    lam, Wv = np.linalg.eigh(T)
    order = np.argsort(lam)[::-1][:pcs]
    return np.maximum(lam[order], 0.0), orient(Q @ Wv[:, order])


def pca(xp: torch.Tensor, M: int, pcs: int = 10, oversample: int = 10, iters: int = 10, maf: float = 0.0, seed: int = 42,
        idx=None) -> PcaResult:
    """The top ``pcs`` principal components of the samples ``idx`` (default: every row) of the packed device matrix ``xp [rows, ld]``:
    eigenvalues and eigenvectors of ``Z Z^T / M_eff`` (module docstring) by ``iters`` rounds of subspace iteration on
    ``L = pcs + oversample <= 32`` columns started at ``omega(M, L, seed)``, then a Rayleigh-Ritz step in float64."""
    L = check_args(pcs, oversample, iters, maf)
    pcs, iters, M = int(pcs), int(iters), int(M)
    if idx is not None and not torch.is_tensor(idx):
        idx = torch.from_numpy(np.ascontiguousarray(np.asarray(idx), dtype=np.int32)).to(xp.device)
    b = _shape(xp, M, idx, "pca")
    if pcs > b:
        raise RuntimeError(f"pca: {pcs} components were asked of {b} samples")
    with torch.cuda.device(xp.device):
        c, s, m_eff, total = standardise(snp_counts(xp, M, idx), maf)
        dev, CP = xp.device, pad_columns(L)
        sd = torch.from_numpy(s).to(dev)[:, None]
        cd = torch.from_numpy(c).to(dev)[:, None]
        fwd_scratch = torch.empty(max(int(lib.nadm_obs_project_scratch_floats(b, M, CP)), 4), dtype=torch.float32, device=dev)
        t_scratch = torch.empty(max(int(lib.nadm_obs_project_t_scratch_floats(b, M, CP)), 4), dtype=torch.float32, device=dev)

        def z_times(Wd):                                     # Z W: W float64 [M, CP] on the device, pad columns 0 -> host float64 [b, L]
            sw = sd * Wd
            Y = obs_project(xp, M, sw.to(torch.float32), (-(cd * sw)).to(torch.float32), L, idx, fwd_scratch)
            return Y[:, :L].cpu().numpy().astype(np.float64)

        def zt_times(Qh):                                    # Z^T Q: Q host float64 [b, <= L] -> float64 [M, CP] on the device, pad columns 0
            Qp = np.zeros((b, CP), dtype=np.float32)
            Qp[:, :Qh.shape[1]] = Qh
            O1, O2 = obs_project_t(xp, M, torch.from_numpy(Qp).to(dev), L, idx, t_scratch)
            return sd * (O1.to(torch.float64) - cd * O2.to(torch.float64))

        values, vectors = subspace_pcs(z_times, zt_times, M, L, CP, pcs, iters, seed, dev, m_eff)
    return PcaResult(values, vectors, m_eff, values / total, total)


def log_result(res: PcaResult, logger=log) -> None:
    logger.info(f"    PCA of the standardised genotypes over {res.M_eff} SNPs (total variance {res.total:.6g}):")
    for k, (v, e) in enumerate(zip(res.eigenvalues, res.explained), start=1):
        logger.info(f"      PC{k}: eigenvalue {v:.6g}, {100.0 * e:.3f} % of the variance")


def write_result(stem: str, res: PcaResult) -> None:
    """``{stem}.eigenval``: one eigenvalue per line; ``{stem}.eigenvec``: one line per sample in plink's layout, two identifier
    columns -- the 0-based sample index twice, how the ``kinship`` mode names samples -- and then ``PC1 ..``.  Numbers carry the 17
    digits that read back to the same float64."""
    with open(f"{stem}.eigenval", "w") as fb:
        for v in np.asarray(res.eigenvalues, dtype=np.float64).tolist():
            fb.write(f"{v:.17g}\n")
    with open(f"{stem}.eigenvec", "w") as fb:
        for i, row in enumerate(np.asarray(res.eigenvectors, dtype=np.float64).tolist()):
            fb.write(f"{i} {i} " + " ".join(f"{x:.17g}" for x in row) + "\n")
