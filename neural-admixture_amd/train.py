"""Drop-in for ``neural_admixture.model.train.train`` (train.py:19-149): same positional signature,
same returns ``(Ps, Qs, model)``.  The PCA-space GMM decoder init is the reference's scikit-learn call for
1000-Genomes-sized inputs and its float64 restatement in device ops (_gmm_em.py, same means to 1e-13) for N > 20000;
packing, the step loop and the final-Q pass run on the MI355X engine."""
from __future__ import annotations

import contextlib
import logging
import sys
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .engine import PRECISIONS
from .model import NeuralAdmixture
from .report import loglikelihood_packed

logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(message)s")
log = logging.getLogger(__name__)


def pca_project_gpu(data, V_CM: np.ndarray, device: torch.device, chunk_rows: int = 4096) -> np.ndarray:
    """X_pca [N, C] float32 = (G/2) @ V.T with a missing call counted as 1.5 (train.py:49-55), computed by the pass-1
    kernel (nadm_pca_project) from 2-bit packed rows streamed to the GPU ``chunk_rows`` at a time."""
    from ._lib import lib, check, ptr
    from .layout import ModelLayout
    from .io import packed_chunks
    C_, M = V_CM.shape
    N = data.shape[0]
    ld, CP = ModelLayout.row_stride(M), 8
    Vd = torch.zeros((M, CP), dtype=torch.float32, device=device)
    Vd[:, :C_] = torch.as_tensor(np.ascontiguousarray(V_CM.T), dtype=torch.float32).to(device)
    chunks = int(lib.nadm_encode_chunks(M))
    zpart = torch.empty(chunks * min(N, chunk_rows) * CP, dtype=torch.float32, device=device)
    fold = torch.empty(min(N, chunk_rows) * CP, dtype=torch.float32, device=device)     # chunk partials folded in a fixed order
    idx = torch.arange(min(N, chunk_rows), dtype=torch.int32, device=device)
    out = np.empty((N, C_), dtype=np.float32)
    st = torch.cuda.current_stream().cuda_stream
    for s, e, pk in packed_chunks(data, ld, chunk_rows):
        xp = pk.to(device)
        check(lib.nadm_pca_project(ptr(xp), ld, ptr(idx), e - s, M, ptr(Vd), CP, ptr(zpart), st), "pca_project")
        check(lib.nadm_sum_rows(ptr(zpart), chunks, (e - s) * CP, ptr(fold), st), "sum_rows")
        out[s:e] = fold[: (e - s) * CP].view(e - s, CP)[:, :C_].cpu().numpy()
    return out


def gmm_p_init(data_np, V_CM: np.ndarray, K: Optional[int], min_k, max_k, n_components: int, seed: int,
               device: Optional[torch.device] = None, fit: str = "auto") -> np.ndarray:
    """P_init [sum(ks), M] = clip(GMM means @ V, 5e-6, 1-5e-6) in the PCA subspace (train.py:49-68).
    Note the projection keeps missing (3) as 1.5, exactly like the reference (train.py:52).
    ``data_np``: uint8 [N,M] array or an io.PackedGenotypes.  With a GPU ``device`` and n_components <= 8 the
    projection runs on the GPU (pca_project_gpu); otherwise on the host, 1024 rows at a time like the reference.
    The mixture fit (``fit``): "sklearn" = the reference's scikit-learn call, "em" = its float64 restatement in device ops
    (_gmm_em.py), "native" = the same on host threads (gmm.py + csrc/nadm_gmm.cpp), "device" = the same with the sums over the samples
    in HIP kernels (csrc/nadm_gmm_dev.hip: 8 components, K <= 16), "auto" = "device" where it applies and pays (a GPU run with
    N >= 20000), else "native" -- all give the library's means to 1e-10 (the device form to 1e-9)."""
    N = data_np.shape[0]
    if device is not None and device.type == "cuda" and n_components <= 8:
        X_pca = pca_project_gpu(data_np, V_CM, device)
    else:
        rows = data_np.unpack_rows if hasattr(data_np, "unpack_rows") else (lambda s, e: data_np[s:e])
        X_pca = np.zeros((N, n_components), dtype=np.float32)
        for i in range(0, N, 1024):
            X_pca[i:i + 1024] = (rows(i, min(N, i + 1024)).astype(np.float32) / 2) @ V_CM.T
    X_pca = X_pca.astype("float64")
    ks = [K] if K is not None else list(range(min_k, max_k + 1))
    how = fit
    from . import gmm as _gmm
    # "auto" / "native": the library's algorithm restated on the host (gmm.py + csrc/nadm_gmm.cpp: same seeding draws, same EM, means equal
    # to 1e-10 -- tests/test_abi_and_host.py): ~0.05 s at N = 2504 where the library takes 0.55 s + a 1.0 s import, ~0.2 s at N = 100k
    # (restarts and sample ranges on threads) where it takes 22-45 s; several K run concurrently.  "em": the same in float64 device ops
    # (_gmm_em.py; pays the device BLAS's first-use cost).  "sklearn": the library itself, several K as concurrent child processes.
    if how == "em":
        from ._gmm_em import fit_means as fit_means_device
        means = [fit_means_device(X_pca, k, seed, device) for k in ks]
    elif how == "device" or (how == "auto" and device is not None and device.type == "cuda"
                             and all(_gmm.device_form_applies(N, n_components, k) for k in ks)):
        with torch.cuda.device(device):                            # (a few launches per iteration: the K of a multi-head run one after the other)
            means = [_gmm.fit_means(X_pca, k, seed, stream=torch.cuda.current_stream().cuda_stream) for k in ks]
    elif how in ("auto", "native"):
        from .gmm import fit_means as fit_means_host
        if len(ks) > 1:
            from concurrent.futures import ThreadPoolExecutor     # (the C call releases the GIL; each fit runs its restarts on threads of its own)
            # (each fit sizes its restart x worker threads for the whole host, csrc/nadm_gmm.cpp: two at a time keep K = 2..10 from
            # putting several hundred spinning threads on it -- ADVICE r05)
            with ThreadPoolExecutor(max_workers=min(2, len(ks))) as pool:
                means = list(pool.map(lambda k_: fit_means_host(X_pca, k_, seed), ks))
        else:
            means = [fit_means_host(X_pca, ks[0], seed)]
    else:
        means = _gmm_means_parallel(X_pca, ks, seed) if len(ks) > 2 else None
        if means is None:
            from ._gmm_fit import fit_means
            means = [fit_means(X_pca, k, seed) for k in ks]
    return np.concatenate([np.clip(m @ V_CM, 5e-6, 1 - 5e-6) for m in means], axis=0)


def _gmm_means_parallel(X_pca: np.ndarray, ks, seed: int):
    """The multi-head run fits one GMM per K (train.py:65-67, a list comprehension in the reference).  The fits are
    independent and deterministic (random_state), so they run as concurrent child processes (_gmm_fit.py as a script:
    numpy + sklearn only, no fork of the process that owns the GPU context).  Returns None on any failure -- the caller
    then fits sequentially in-process, which gives the same numbers."""
    import os
    import subprocess
    import tempfile
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gmm_fit.py")
    procs = []
    try:
        with tempfile.TemporaryDirectory() as td:
            xp = os.path.join(td, "x.npy")
            np.save(xp, X_pca)
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            procs = [subprocess.Popen([sys.executable, script, xp, str(k), str(seed), os.path.join(td, f"m{k}.npy")], env=env,
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for k in ks]
            codes = [p.wait(timeout=600) for p in procs]
            if any(codes):
                log.info(f"    concurrent GMM fits failed (exit codes {codes}); fitting in-process instead")
                return None
            return [np.load(os.path.join(td, f"m{k}.npy")) for k in ks]
    except (OSError, subprocess.SubprocessError, ValueError) as e:
        log.info(f"    concurrent GMM fits failed ({type(e).__name__}: {e}); fitting in-process instead")
        return None
    finally:
        for p in procs:                         # no orphans: a timed-out / failed batch must not keep running beside the fallback
            if p.poll() is None:
                p.kill()
                p.wait()


def class_sums_gpu(data, y: np.ndarray, K: int, device: torch.device, chunk_rows: int = 4096) -> np.ndarray:
    """uint32 [K, M]: per class the exact sum of the raw 2-bit codes (0, 1, 2, missing 3) over the rows labelled with it, rows with
    y == -1 left out -- computed by nadm_class_sums from 2-bit packed rows.  A matrix that already lives on the GPU (a
    PackedGenotypes read with keep_on_device) is summed where it is, in one call; anything else is packed on the host and streamed
    ``chunk_rows`` at a time, the calls adding into the same array."""
    import ctypes as C
    from ._lib import lib, check, ptr
    from .layout import ModelLayout
    from .io import packed_chunks
    N, M = data.shape
    resident = hasattr(data, "packed") and data.packed.is_cuda
    ld = int(data.packed.shape[1]) if hasattr(data, "packed") else ModelLayout.row_stride(M)
    sums = torch.zeros((K, M), dtype=torch.int32, device=device)           # (the bits of uint32: read back through a view)
    st = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        for s, e, pk in packed_chunks(data, ld, N if resident else chunk_rows):
            yb = y[s:e]
            order = np.argsort(yb, kind="stable")                         # rows grouped by class, -1 first
            start = np.searchsorted(yb[order], np.arange(K + 1)).astype(np.int64)
            if start[K] == start[0]:
                continue                                                   # no labelled row in this chunk
            idx = torch.from_numpy(order.astype(np.int32)).to(device)
            xp = pk.to(device).contiguous()
            check(lib.nadm_class_sums(ptr(xp), ld, e - s, M, ptr(idx), start.ctypes.data_as(C.POINTER(C.c_int64)), K, ptr(sums), st),
                  "class_sums")                                            # (xp / idx go back to the allocator in stream order)
    return sums.cpu().numpy().view(np.uint32)


def supervised_init(data_np, pops, K: int, unlabelled=(), device: Optional[torch.device] = None):
    """Supervised mode (train.py:74-83): population names -> class indices in sorted order, and
    P_init [K,M] = per-class mean of the RAW codes (0,1,2, missing 3; not halved, not clipped -- the first
    restrict_P brings it into [0,1]).  ``data_np``: uint8 [N,M] or an io.PackedGenotypes.
    ``unlabelled``: names in ``pops`` that stand for "no label" (one string or a collection; ADMIXTURE's .pop files use "-").
    Those samples get y = -1, the classes are the sorted unique REMAINING names, and a class mean runs over the rows labelled with
    it only -- the semi-supervised case the reference does not take.  With a GPU ``device`` the per-class sums come from the packed
    matrix (class_sums_gpu), else from the host loop; both are exact integers and share the float64 division, so they give the
    same bits."""
    skip = {unlabelled} if isinstance(unlabelled, str) else set(unlabelled)
    names = sorted(np.unique([a for a in pops if a not in skip]))
    if K is None or len(names) != K:
        raise AssertionError(f"Number of ancestries in training ground truth ({len(names)}) is not equal to the value of K ({K})")
    lut = {a: i for i, a in enumerate(names)}
    y = np.asarray([-1 if a in skip else lut[a] for a in pops], dtype=np.int64)
    N, M = data_np.shape
    if len(y) != N:
        raise RuntimeError("pops must hold one population label per sample")
    if device is not None and device.type == "cuda":
        sums = class_sums_gpu(data_np, y, K, device).astype(np.float64)
    else:
        rows = data_np.unpack_rows if hasattr(data_np, "unpack_rows") else (lambda s, e: data_np[s:e])
        sums = np.zeros((K, M), dtype=np.float64)
        for i in range(0, N, 1024):
            blk, yb = rows(i, min(N, i + 1024)), y[i:i + 1024]
            for k in range(K):
                if np.any(yb == k):
                    sums[k] += blk[yb == k].sum(axis=0, dtype=np.float64)
    P = (sums / np.bincount(y[y >= 0], minlength=K)[:, None]).astype(np.float32)
    return y, P


@contextlib.contextmanager
def capped_host_threads(limit: int = 4):
    """Caps torch's intra-op pool and the BLAS / OpenMP pools (threadpoolctl) at ``limit`` threads for the duration of the
    block, never raising a pool that is smaller already.  The host side of a run is a launch loop plus a few small numpy /
    scikit-learn calls; with the default pools of a large host (256 threads here, shared with other jobs) their barriers
    spin long enough to stall the HIP runtime's own threads: a full default run on one MI355X takes 2.5 / 5.1 / 14.3-17 s
    (2504 x 600k K=7 / K=2..10 / 100k x 500k K=8) with the default pools and 1.9 / 4.8 / 13.1 s with them capped, the
    mixture fit alone 1.6 -> 1.0 s.  The reference's CLI caps them with --threads (entry.py:138-146); this makes the
    boundary function behave the same when it is called directly."""
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(prev, limit)))
    limits = None
    try:
        from threadpoolctl import ThreadpoolController, threadpool_limits
        per_api = {}
        for lib_info in ThreadpoolController().info():
            api, n = lib_info.get("user_api"), lib_info.get("num_threads")
            if api and n:
                per_api[api] = min(per_api.get(api, limit), n, limit)
        limits = threadpool_limits(limits=per_api) if per_api else None
    except ImportError:                          # threadpoolctl comes with scikit-learn; without it only torch's pool is capped
        pass
    try:
        yield
    finally:
        if limits is not None:
            limits.restore_original_limits()
        torch.set_num_threads(prev)


class AfterOption(NamedTuple):
    """An option of train() that runs after training.  train(), the CLI's ``train`` mode and tests/test_after_training.py read these
    records: a new option is a record, its keywords in train()'s signature and docstring, and its block at the end of _train."""
    kw: str                          # train()'s keyword that switches it on (> 0 or True); the CLI flag is "--" + kw
    params: Tuple[str, ...]          # every keyword of train() that belongs to it, ``kw`` first
    check: Optional[Callable]        # its own value checks: check(after) raises ValueError
    k16: Optional[str]               # needs every K <= 16: the reason the CLI gives; None: any K
    writer: Optional[str]            # the module whose write_results(save_dir, name, results) writes model.after_results[kw]
    cli_before_gpu: bool = True      # the CLI refuses before its GPU check (--polish, the oldest, after it)


def _check_polish(o):
    if o.polish < 0:
        raise ValueError("polish must be >= 0 rounds")


def _check_cv(o):
    if o.cv != 0 and not 2 <= o.cv <= 64:
        raise ValueError("cv must be 0 or a number of folds in 2..64")
    if o.cv > 0 and o.cv_rounds < 1:
        raise ValueError("cv_rounds must be >= 1")


def _check_bootstrap(o):
    if o.bootstrap != 0 and o.bootstrap < 2:
        raise ValueError("bootstrap must be 0 or a number of replicates >= 2")
    if o.bootstrap > 0 and (o.boot_rounds < 1 or o.boot_block < 1):
        raise ValueError("boot_rounds and boot_block must be >= 1")


AFTER_TRAINING = (                                        # in the order they run
    AfterOption("polish", ("polish", "polish_tol"), _check_polish, None, None, cli_before_gpu=False),
    AfterOption("cv", ("cv", "cv_rounds", "cv_tol"), _check_cv, None, None),
    AfterOption("bootstrap", ("bootstrap", "boot_block", "boot_rounds", "boot_tol"), _check_bootstrap, None, "bootstrap"),
    AfterOption("p_se", ("p_se",), None, "the K (K + 1) / 2 running sums of a SNP live in one thread's registers", "pse"),
    AfterOption("q_se", ("q_se",), None, "the K (K + 1) / 2 running sums of a sample live in one thread's registers", "qse"),
    AfterOption("fit_check", ("fit_check",), None, "a sample's Q row and a chunk's refitted frequencies live in registers and LDS",
                "fitcheck"),
)
AFTER_KEYWORDS = tuple(p for opt in AFTER_TRAINING for p in opt.params)


def train(epochs: int, batch_size: int, learning_rate: float, K: int, seed: int, data: torch.Tensor, device: torch.device,
          num_gpus: int, hidden_size: int, master: bool, V: np.ndarray, pops, min_k: int = None, max_k: int = None,
          n_components: int = None, *, parallelism: str = "dp", host_threads: int = 4, gmm: str = "auto", precision: str = "highest",
          unlabelled=None, supervised_loss_weight: float = 100.0, polish: int = 0, polish_tol: float = 1e-5, cv: int = 0,
          cv_rounds: int = 50, cv_tol: float = 1e-5, bootstrap: int = 0, boot_block: int = 1, boot_rounds: int = 50, boot_tol: float = 1e-5,
          p_se: bool = False, q_se: bool = False, fit_check: bool = False):
    """The reference's boundary function (see the module docstring and _train).  The host thread pools (torch intra-op, BLAS,
    OpenMP) are capped at ``host_threads`` while it runs -- the reference's CLI does that with --threads (entry.py:138-146), and
    this package's CLI passes its --threads here; the epoch loop itself always runs with torch's pool at 1 (model.py).
    ``gmm`` (keyword, CLI --gmm): who fits the decoder-init mixture (gmm_p_init's ``fit``): "sklearn" is the reference's own call.
    ``precision`` (keyword, CLI --precision): the matmul precision of the training step, "highest" (fp32-class products, the default)
    or "medium" (bf16-class: the reference's torch.set_float32_matmul_precision('medium')).
    ``unlabelled`` (keyword, CLI --unlabelled): names in ``pops`` that mean "this sample has no label" (one string or a collection;
    None, the default: every entry is a class name, the reference's contract).  Such samples take part in the reconstruction loss
    like any other and stay out of the supervised term and of the class means of the decoder init (supervised_init).
    ``supervised_loss_weight`` (keyword, CLI --supervised_loss_weight): the weight of the supervised term, 100 like the reference's
    default.
    The options that run after training (AFTER_TRAINING), in this order, each on the matrices about to be returned: single-GPU,
    unsupervised runs only; 0 or False (the defaults) call nothing; what has a file format is logged and left in the returned model's
    ``after_results`` under the option's keyword (absent without it), from where the CLI writes it.
    ``polish`` / ``polish_tol`` (keyword, CLI --polish / --polish_tol): up to ``polish`` rounds of block EM over the OBSERVED calls
    (Engine.polish) started from the trained P and the encoder's Q; the returned ``Ps`` and ``Qs`` are then the polished ones --
    training reads a missing call as genotype 0, which pulls P down wherever calls are missing -- while the returned model stays as
    trained.
    ``cv`` / ``cv_rounds`` / ``cv_tol`` (keyword, CLI --cv / --cv_rounds / --cv_tol): the cross-validation error of every K over
    ``cv`` folds of held-out CALLS (cv.cv_error, fold seed ``seed``), refitted from those matrices, is logged as
    ``CV error (K=k): x``.
    ``bootstrap`` / ``boot_block`` / ``boot_rounds`` / ``boot_tol`` (keyword, CLI --bootstrap / --block / --boot_rounds / --boot_tol):
    bootstrap standard errors of every K's Q from ``bootstrap`` replicates that resample the SNPs in blocks of ``boot_block``
    (bootstrap.bootstrap_q, draw seed ``seed``), refitted from those matrices (files: .Q_se / .Q_bias).
    ``p_se`` (keyword, CLI --p_se): the standard errors of every K's P from the per-SNP Fisher information given the Q about to be
    returned (pse.p_se; every K <= 16; file: .P_se).
    ``q_se`` (keyword, CLI --q_se): the standard errors of every K's Q from the per-sample Fisher information given the P about to be
    returned (qse.q_se; every K <= 16; file: .Q_info_se).  Conditional on P: for the samples P was fitted to it leaves out P's own error.
    ``fit_check`` (keyword, CLI --fit_check): the model-fit check of every K (fitcheck.fit_check: the correlation of leave-one-out
    residuals, grouped by largest component; every K <= 16; above 4096 samples the pairs of a subset drawn with ``seed``; files:
    .cor_pop / .cor_sample)."""
    after = SimpleNamespace(**{name: value for name, value in locals().items() if name in AFTER_KEYWORDS})   # (first: only arguments yet)
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'highest' or 'medium'")
    k_max = K if K is not None else (max_k or 0)           # the largest K asked for
    for opt in AFTER_TRAINING:
        if opt.check is not None:
            opt.check(after)
        if not getattr(after, opt.kw) > 0:
            continue
        if num_gpus > 1 or pops is not None:
            raise ValueError(f"{opt.kw} needs a single-GPU, unsupervised run (it ignores labels and works on the whole resident matrix)")
        if opt.k16 is not None and k_max > 16:
            raise ValueError(f"{opt.kw} needs every K <= 16")
    with capped_host_threads(max(1, int(host_threads))):
        return _train(epochs, batch_size, learning_rate, K, seed, data, device, num_gpus, hidden_size, master, V, pops, min_k, max_k,
                      n_components, parallelism=parallelism, gmm=gmm, precision=precision, unlabelled=unlabelled,
                      supervised_loss_weight=supervised_loss_weight, after=after)


def _train(epochs: int, batch_size: int, learning_rate: float, K: int, seed: int, data: torch.Tensor, device: torch.device,
           num_gpus: int, hidden_size: int, master: bool, V: np.ndarray, pops, min_k: int = None, max_k: int = None,
           n_components: int = None, *, parallelism: str = "dp", gmm: str = "auto", precision: str = "highest", unlabelled=None,
           supervised_loss_weight: float = 100.0, after: SimpleNamespace):
    """See module docstring.  ``data`` uint8 [N,M] CPU tensor (or an ``io.PackedGenotypes``, e.g. from
    ``io.read_bed_packed``); ``V`` numpy [C,M] (RSVD output,
    svd.py:83); returns Ps (list of [M,k] float32), Qs (list of [N,k] float32), model.
    ``parallelism`` (keyword, not in the reference): "dp" = samples sharded over the GPUs, gradients summed over ranks like the reference's DDP (here: reduce-scatter,
    optimizer on the rank's slice, all-gather); "snp" = SNPs sharded (snp_parallel.py): same trajectory up to summation order, two tiny all-reduces
    per step instead of the 4*M*(C+S)-byte one.
    ``after``: train()'s after-training keywords (AFTER_TRAINING), already checked."""
    eng_cls = NeuralAdmixture.engine_snp_cls if parallelism == "snp" else NeuralAdmixture.engine_cls
    if not eng_cls.supports(device):
        raise RuntimeError("neural_admixture_amd.train requires a ROCm GPU device; the CPU path is the reference's own")
    N, M = data.shape
    if n_components is None:
        n_components = V.shape[0]
    total_K = K if K is not None else sum(range(min_k, max_k + 1))
    y_num = None
    if master and pops is None:
        log.info("")
        log.info("    Running Gaussian Mixture in PCA subspace...")
        log.info("")
        P = gmm_p_init(data if hasattr(data, "unpack_rows") else data.numpy(), V, K, min_k, max_k, n_components, seed, device, fit=gmm)
    elif master:
        log.info("")
        log.info("    Running Supervised Mode...")
        log.info("")
        y_num, P = supervised_init(data if hasattr(data, "unpack_rows") else data.numpy(), pops, K,
                                   unlabelled=() if unlabelled is None else unlabelled, device=device)
        if (y_num < 0).any():
            log.info(f"    Labelled samples: {int((y_num >= 0).sum())}, unlabelled samples: {int((y_num < 0).sum())}.")
            log.info("")
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    if num_gpus > 1 and dist.is_available() and dist.is_initialized():
        if master:
            P_init = torch.as_tensor(P, dtype=torch.float32, device=device).contiguous()
            Vt = torch.as_tensor(V.T, dtype=torch.float32, device=device).contiguous()
            log.info("    Broadcasting to all GPUs...")
            if pops is not None:
                pops = torch.as_tensor(y_num, dtype=torch.int64, device=device)
        else:
            P_init = torch.empty((total_K, M), dtype=torch.float32, device=device)
            Vt = torch.empty((M, n_components), dtype=torch.float32, device=device)
            if pops is not None:
                pops = torch.empty(len(pops), dtype=torch.int64, device=device)
        if pops is not None:
            dist.broadcast(pops, src=0)        # train.py:107-108
        dist.broadcast(P_init, src=0)          # train.py:109
        dist.broadcast(Vt, src=0)              # train.py:110
        dist.barrier()
        if master:
            log.info("    Finished broadcasting!")
    else:
        P_init = torch.as_tensor(P, dtype=torch.float32).contiguous()
        Vt = torch.as_tensor(V.T, dtype=torch.float32).contiguous()
        if pops is not None:
            pops = torch.as_tensor(y_num, dtype=torch.int64)

    if master and precision != "highest":
        log.info(f"    Matmul precision: {precision} (bf16-class products in the genotype passes).")
    model = NeuralAdmixture(K, epochs, batch_size, learning_rate, device, seed, num_gpus, master, None, min_k, max_k,
                            supervised_loss_weight=supervised_loss_weight, parallelism=parallelism, precision=precision)
    Qs, Ps, raw = model.launch_training(P_init, data, hidden_size, Vt.shape[1], Vt, M, N, pops)

    if after.polish > 0:                                   # (the log-likelihood below is then that of the polished matrices)
        Pp, Qp, ll0, ll1, ran = model.engine.polish(after.polish, after.polish_tol)
        Ps, Qs = [x.cpu().numpy() for x in Pp], [x.cpu().numpy() for x in Qp]
        log.info(f"    Log-likelihood of the observed calls before polishing: {ll0:.3f}")
        log.info(f"    Log-likelihood of the observed calls after polishing:  {ll1:.3f}")
        log.info(f"    Polishing rounds run: {ran}")
        log.info("")
    xp, done = model.engine.xp, raw.after_results          # what is logged below and has a writer goes there under its keyword
    if after.cv > 0:                                       # on the matrices about to be returned
        from . import cv as _cv
        _cv.log_results(_cv.cv_error(xp, M, Ps, Qs, after.cv, after.cv_rounds, after.cv_tol, seed), log)
        log.info("")
    if after.bootstrap > 0:                                # likewise; the written .Q stays the one above, the centre goes with the results
        from . import bootstrap as _boot
        done["bootstrap"] = _boot.bootstrap_q(xp, M, Ps, Qs, after.bootstrap, after.boot_block, after.boot_rounds, after.boot_tol, seed)
        _boot.log_results(done["bootstrap"], log, after.boot_rounds)
        log.info("")
    if after.p_se:                                         # likewise: of the P about to be returned, given the Q about to be returned
        from . import pse as _pse
        done["p_se"] = [_pse.p_se(xp, M, P_k, Q_k) for P_k, Q_k in zip(Ps, Qs)]
        _pse.log_results(done["p_se"], log)
        log.info("")
    if after.q_se:                                         # likewise: of the Q about to be returned, given the P about to be returned
        from . import qse as _qse
        done["q_se"] = [_qse.q_se(xp, M, P_k, Q_k) for P_k, Q_k in zip(Ps, Qs)]
        _qse.log_results(done["q_se"], log)
        log.info("")
    if after.fit_check:                                    # likewise: of the P and Q about to be returned
        from . import fitcheck as _fit
        n_all = int(xp.shape[0])
        pairs = None if n_all <= _fit.MAX_ROWS else np.sort(np.random.default_rng(seed).choice(n_all, size=_fit.MAX_ROWS, replace=False))
        done["fit_check"] = [_fit.fit_check(xp, M, P_k, Q_k, None, pairs) for P_k, Q_k in zip(Ps, Qs)]
        _fit.log_results(done["fit_check"], log)
        log.info("")
    if master:
        ks = [K] if K is not None else list(range(min_k, max_k + 1))
        for i, k in enumerate(ks):
            logl = model.logliks[i] if model.logliks is not None else loglikelihood_packed(model.engine, data, Ps[i], Qs[i])
            if K is not None:
                log.info(f"    Log-likelihood: {logl:2f}.")
            else:
                log.info(f"    Log-likelihood for K={k}: {logl:2f}.")
    return Ps, Qs, raw
