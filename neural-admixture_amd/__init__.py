"""MI355X-native Neural ADMIXTURE training engine (hot path only).

Drop-in for the reference's ``neural_admixture.model.train.train`` boundary: same signature, same
returns, hand-written gfx950 HIP kernels behind a C ABI (``include/nadm.h`` / ``csrc/libnadm.so``).
PyTorch is used for device memory, streams and ``torch.distributed`` only.
"""
from . import _lib          # noqa: F401  (fails loudly if libnadm.so is missing)
from .layout import ModelLayout   # noqa: F401
from .engine import Engine        # noqa: F401
from .model import Q_P, NeuralAdmixture   # noqa: F401
from .train import train          # noqa: F401
from .project import project_q    # noqa: F401  (Q refined against a fixed P, no encoder needed)
from .project import project_p, polish    # noqa: F401  (P refitted against a fixed Q; the two alternated)
from .relate import kinship, kinship_pairs    # noqa: F401  (admixture-aware kinship of sample pairs from Q and P)
from .king import king_pairs, unrelated_set, select_samples    # noqa: F401  (KING-robust kinship from the genotypes alone, the unrelated set, the selection of samples; the dense form is king.king)
from .ld import snp_counts, ld_band, prune, select_snps    # noqa: F401  (LD pruning: windowed r^2, the keep-list, the selection)
from .hwe import snp_hwe, snp_hwe_sums, hwe_keep    # noqa: F401  (Hardy-Weinberg score test given ancestry, per SNP, from Q and P)
from .cv import cv_error, mask_fold, heldout_deviance    # noqa: F401  (cross-validation error for choosing K, over held-out calls)
from .bootstrap import bootstrap_q, block_weights    # noqa: F401  (bootstrap standard errors of Q: SNPs resampled, weighted refits)
from .qse import q_se, q_info                  # noqa: F401  (standard errors of Q given P: per-sample Fisher information, inverted under the sum constraint)
from .pse import p_se, p_info, se_from_info    # noqa: F401  (standard errors of P: per-SNP Fisher information given Q, inverted)
from .fitcheck import resid_cor, em_sums, fit_check, group_means, sample_means    # noqa: F401  (model-fit check: correlation of leave-one-out residuals)
from . import pca                 # noqa: F401  (principal components of the standardised genotypes: pca.pca; the module, whose name its function shares)
from .pca import obs_project, obs_project_t    # noqa: F401  (its two products: the observed-calls pair products)
from . import residpca            # noqa: F401  (residual PCA given Q and P: what structure the K components leave, and in which samples)
from .residpca import resid_pca, resid_project, resid_project_t    # noqa: F401  (its function and its two products of the standardised residuals)
from . import pack2bit            # noqa: F401  (the reference's native module by its own names: pack2bit.cu:144-147)

__all__ = ["train", "Engine", "ModelLayout", "Q_P", "NeuralAdmixture", "pack2bit", "project_q", "project_p", "polish", "kinship", "kinship_pairs", "king_pairs", "unrelated_set", "select_samples",
           "snp_counts", "ld_band", "prune", "select_snps", "snp_hwe", "snp_hwe_sums", "hwe_keep", "cv_error", "mask_fold", "heldout_deviance",
           "bootstrap_q", "block_weights", "p_se", "p_info", "se_from_info", "q_se", "q_info", "resid_cor", "em_sums", "fit_check", "group_means",
           "sample_means", "pca", "obs_project", "obs_project_t", "residpca", "resid_pca", "resid_project",
           "resid_project_t"]
