"""Thin command line with the reference's flags (entry.py:20-67): ``python -m neural_admixture_amd train|infer|king|kinship|prune|hwe|cv|bootstrap|pse|qse|fit|pca|residpca|date ...``.
Reads BED input straight into the packed layout, runs the RSVD + GMM initialisation, trains on the MI355X engine and
writes ``{name}.{K}.Q/.P``, ``{name}.pt`` and ``{name}_config.json`` exactly where the reference does
(src/main.py:38-44, src/inference.py:91-92).  BED and VCF inputs are read natively (io.read_bed_packed, io.read_vcf_packed);
PGEN needs pgenlib through the reference's own reader.  ``--num_gpus N`` spawns one process per GPU like the reference
(entry.py:186-190); ``--threads`` sets the size of the host thread pools like the reference's (entry.py:138-146): torch's pool
at once, the BLAS / OpenMP pools inside train() (host_threads=), the environment variables for child processes."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

from .engine import row_ranges
from .train import AFTER_KEYWORDS, AFTER_TRAINING
from .io import (chrom_codes, find_run_files, genetic_map, read_bim, read_bim_map, read_fam, read_id_list, read_run_matrix, read_sample_list, resolve_ids,
                 resolve_samples, write_id_list)

logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(message)s")
log = logging.getLogger(__name__)


def _add_precision(p):
    p.add_argument("--precision", choices=("highest", "medium"), default="highest",
                   help="matmul precision of the genotype passes: 'highest' (fp32-class products, default) or 'medium' (bf16-class, "
                        "what the reference's torch.set_float32_matmul_precision('medium') gives)")


def _add_extract(p):
    p.add_argument("--extract", type=str, default=None, metavar="FILE",
                   help="use only the SNPs whose IDs (column 2 of the .bim) FILE lists, one per line -- a {name}.prune.in of the 'prune' "
                        "mode, or any list plink --extract would read.  BED input only.  Default: every SNP")


def _add_samples(p):
    g = p.add_mutually_exclusive_group()
    g.add_argument("--keep", type=str, default=None, metavar="FILE",
                   help="use only the samples FILE lists, one 'FID IID' (or the IID alone) per line as in the .fam -- a {name}.king.in of "
                        "the 'king' mode, or any list plink --keep would read.  BED input only.  Default: every sample")
    g.add_argument("--remove", type=str, default=None, metavar="FILE",
                   help="leave out the samples FILE lists (a {name}.king.out, or any list plink --remove would read).  BED input only")


def parse_train_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture train", description="Rapid population clustering with autoencoders - training mode")
    p.add_argument("--epochs", type=int, default=250)
    p.add_argument("--batch_size", type=int, default=800)
    p.add_argument("--learning_rate", type=float, default=20e-4)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--k", type=int)
    p.add_argument("--min_k", type=int)
    p.add_argument("--max_k", type=int)
    p.add_argument("--hidden_size", type=int, default=1024)
    p.add_argument("--save_dir", required=True, type=str)
    p.add_argument("--data_path", required=True, type=str)
    p.add_argument("--name", required=True, type=str)
    p.add_argument("--supervised_loss_weight", type=float, default=100,
                   help="weight of the supervised term (default 100, the reference's); lower it when unlabelled samples come out "
                        "with a single ancestry")
    p.add_argument("--pops_path", type=str, default="")
    p.add_argument("--unlabelled", type=str, default="-", metavar="TOKEN",
                   help="line of --pops_path that marks a sample WITHOUT a label (default '-', the convention of ADMIXTURE's .pop "
                        "files): such samples train the reconstruction only and get their Q like any other.  A population can "
                        "therefore not be named TOKEN itself; pass another token if one is literally named '-'")
    p.add_argument("--n_components", type=int, default=8)
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--threads", type=int, default=1,
                   help="host thread pools (torch, BLAS, OpenMP), like the reference's flag (entry.py:46,138-146; default 1 as there). "
                        "The GPU step does not use them; the decoder-init mixture fit and the host side of the readers do: 4 is a good value")
    p.add_argument("--parallelism", choices=("dp", "snp"), default="dp",
                   help="multi-GPU sharding: dp = samples (the reference's DDP), snp = SNPs (two tiny all-reduces per step)")
    p.add_argument("--gmm", choices=("auto", "sklearn", "native", "device", "em"), default="auto",
                   help="decoder-init mixture fit (model/train.py:60-68): sklearn = the reference's own scikit-learn GaussianMixture call; "
                        "auto (default) = its float64 restatement on host threads / HIP kernels (same means to 1e-10, no library import: "
                        "0.1 s instead of 1.5 s on a 1000-Genomes-sized run); see INTEGRATION.md section 3")
    p.add_argument("--share_gpu", action="store_true",
                   help="functional check of a --num_gpus N run on a ONE-GPU box: every rank uses cuda:0 and gloo carries the "
                        "tensors (RCCL refuses two ranks per device)")
    p.add_argument("--polish", type=int, default=0, metavar="N",
                   help="after training, up to N rounds of block EM over the OBSERVED calls only (a Q step with P fixed, then a P step "
                        "with the new Q), started from the trained P and the encoder's Q: the written .Q/.P are then a masked "
                        "maximum-likelihood fit (training reads a missing call as genotype 0).  The .pt checkpoint stays as trained.  "
                        "Single-GPU, unsupervised runs only.  0 (default): off")
    p.add_argument("--polish_tol", type=float, default=1e-5,
                   help="stop polishing once no entry of Q or P moves by this much in a round")
    p.add_argument("--cv", type=int, default=0, metavar="FOLDS",
                   help="after training (and after --polish), the cross-validation error of every K over FOLDS folds of held-out "
                        "genotype CALLS, refitted from the matrices about to be written and logged as 'CV error (K=k): x' like "
                        "ADMIXTURE's --cv; the fold draw uses --seed.  Single-GPU, unsupervised runs only.  0 (default): off")
    _add_cv_refit(p)
    p.add_argument("--bootstrap", type=int, default=0, metavar="B",
                   help="after training (and after --polish), bootstrap standard errors of every K's Q from B replicates that resample "
                        "the SNPs, refitted from the matrices about to be written: {name}.{K}.Q_se and .Q_bias like ADMIXTURE's -B; "
                        "the draw uses --seed.  Single-GPU, unsupervised runs only.  0 (default): off")
    _add_boot_refit(p)
    p.add_argument("--p_se", action="store_true",
                   help="after training (and after --polish), standard errors of every K's P from the per-SNP Fisher information given "
                        "the Q about to be written: {name}.{K}.P_se, M x K like the .P file, nan where no standard error is defined.  "
                        "Conditional on Q; every K must be <= 16.  Single-GPU, unsupervised runs only")
    p.add_argument("--q_se", action="store_true",
                   help="after training (and after --polish), standard errors of every K's Q from the per-sample Fisher information given "
                        "the P about to be written: {name}.{K}.Q_info_se, N x K like the .Q file, nan for a sample without one.  "
                        "Conditional on P (for the training samples it leaves out P's own error; --bootstrap gives the joint one); an "
                        "entry at 0 or 1 carries a detection limit, not a spread.  Every K must be <= 16.  Single-GPU, unsupervised runs only")
    p.add_argument("--fit_check", action="store_true",
                   help="after training (and after --polish), the model-fit check of every K from the matrices about to be written: the "
                        "pairwise correlation of leave-one-out residuals (evalAdmix's statistic), summarised per group of samples (largest "
                        "component) in {name}.{K}.cor_pop and per sample in {name}.{K}.cor_sample, as the 'fit' mode writes them.  Run it "
                        "with --polish: the statistic assumes a P at the fixed point of its own EM step.  Every K must be <= 16; the pairs of "
                        "at most 4096 samples are taken (a seeded subset above that).  Single-GPU, unsupervised runs only")
    _add_precision(p)
    _add_extract(p)
    _add_samples(p)
    return p.parse_args(argv)


def parse_infer_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture infer", description="Rapid population clustering with autoencoders - inference mode")
    p.add_argument("--out_name", required=True, type=str)
    p.add_argument("--save_dir", required=True, type=str)
    p.add_argument("--data_path", required=True, type=str)
    p.add_argument("--name", required=True, type=str)
    p.add_argument("--batch_size", type=int, default=1024)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--threads", type=int, default=1)
    p.add_argument("--refine", type=int, default=0, metavar="N",
                   help="after the encoder pass, refine every sample's Q with up to N masked EM steps against the trained allele "
                        "frequencies {save_dir}/{name}.{K}.P held fixed (projection: only a sample's observed calls count). "
                        "0 (default): the encoder's Q as it is")
    p.add_argument("--refine_tol", type=float, default=1e-4,
                   help="stop refining a batch once no entry of Q moves by this much in a step")
    p.add_argument("--q_se", action="store_true",
                   help="with --refine: standard errors of the refined Q from the per-sample Fisher information given the fixed P, "
                        "written next to the .Q as {out_name}.{K}.Q_info_se (N x K, nan for a sample without an observed call); a sample "
                        "with few observed calls shows there.  An entry at 0 or 1 carries a detection limit.  Every K must be <= 16")
    p.add_argument("--bound", type=float, default=1e-4,
                   help="--q_se logs a fraction within this of 0 or 1 as at the bound (default 1e-4)")
    _add_precision(p)
    _add_extract(p)
    _add_samples(p)
    return p.parse_args(argv)


def _add_run_args(p, multi_k, out="files"):
    """What the analysis parsers share: where the data and the run's files are, the K of the run (``multi_k``: --k or --min_k ..
    --max_k; False: one required --k; None: no K), the host threads, --keep / --remove and -- unless ``out`` is None -- the output
    name (of the written ``out``) and --extract."""
    for flag in ("--data_path", "--save_dir", "--name"):
        p.add_argument(flag, required=True, type=str)
    if multi_k is not None:
        p.add_argument("--k", required=not multi_k, type=int)
    if multi_k:
        p.add_argument("--min_k", type=int)
        p.add_argument("--max_k", type=int)
    p.add_argument("--threads", type=int, default=1)
    _add_samples(p)
    if out is not None:
        p.add_argument("--out_name", type=str, default=None, help=f"name of the written {out} (default: --name)")
        _add_extract(p)


def parse_kinship_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture kinship",
                                description="Admixture-aware kinship (REAP) of the samples from a run's .P and .Q files")
    _add_run_args(p, multi_k=False)
    p.add_argument("--min_phi", type=float, default=2.0 ** -4.5,
                   help="list the pairs with a kinship coefficient of at least this (default 0.0442, the lower edge of third-degree relatives)")
    p.add_argument("--pimin", type=float, default=0.0,
                   help="drop a call whose individual-specific allele frequency is outside [pimin, 1 - pimin] (default 0: every observed call counts)")
    p.add_argument("--ibd", action="store_true",
                   help="also estimate the IBD-sharing probabilities k0, k1, k2 of the listed pairs (PC-Relate's estimators on the same "
                        "frequencies) and write {out_name}.{k}.ibd, 'i j phi n k0 k1 k2 ibs0 relation' per pair: k0 tells a parent-offspring "
                        "pair (0) from full siblings (1/4), which share phi = 0.25.  K must be <= 16")
    p.add_argument("--po_k0", type=float, default=0.1,
                   help="with --ibd: a first-degree pair with k0 below this is labelled parent-offspring, otherwise full siblings (default "
                        "0.1, a convention between the expected 0 and 0.25, not a calibration); in (0, 0.25)")
    return p.parse_args(argv)


def parse_king_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture king",
                                description="KING-robust kinship of the samples from the genotype file alone, and a maximal set of "
                                            "unrelated samples to train on")
    _add_run_args(p, multi_k=None, out=None)
    _add_extract(p)
    p.add_argument("--cutoff", type=float, default=2.0 ** -3.5,
                   help="a pair with a kinship coefficient of at least this is related (default 0.0884, the lower edge of second-degree "
                        "relatives): it is listed, and one of its samples goes to the .king.out list")
    p.add_argument("--rows", type=int, default=1024, help="samples per side of a block of pairs, 1..4096 (default 1024)")
    return p.parse_args(argv)


def parse_prune_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture prune",
                                description="LD pruning: the SNPs to keep so that no two within a window have an r^2 above a threshold")
    _add_run_args(p, multi_k=None, out=None)
    p.add_argument("--window", type=int, default=50, help="a SNP is compared with its next window - 1 neighbours on its chromosome (default 50)")
    p.add_argument("--r2", type=float, default=0.1, help="of a pair with an r^2 above this the SNP with the smaller minor-allele frequency goes (default 0.1)")
    return p.parse_args(argv)


def parse_pca_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture pca",
                                description="Principal components of the standardised genotypes (the GRM of smartpca / plink --pca), "
                                            "from the genotype file alone")
    _add_run_args(p, multi_k=None, out="eigenvalues and eigenvectors")
    p.add_argument("--pcs", type=int, default=10, help="principal components to report (default 10)")
    p.add_argument("--oversample", type=int, default=10,
                   help="extra columns the subspace iteration carries (default 10); --pcs + --oversample is at most 32")
    p.add_argument("--iters", type=int, default=10, help="rounds of subspace iteration (default 10, FastPCA's)")
    p.add_argument("--maf", type=float, default=0.0,
                   help="leave out the SNPs whose minor-allele frequency is below this (default 0: only unobserved and monomorphic SNPs go)")
    p.add_argument("--seed", type=int, default=42)
    return p.parse_args(argv)


def parse_residpca_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture residpca",
                                description="Residual PCA: principal components of the standardised residuals given a run's .P and .Q "
                                            "files, read against the Marchenko-Pastur edge (use LD-pruned data)")
    _add_run_args(p, multi_k=True, out="eigenvalues and eigenvectors")
    p.add_argument("--pcs", type=int, default=10, help="principal components to report (default 10)")
    p.add_argument("--oversample", type=int, default=10,
                   help="extra columns the subspace iteration carries (default 10); --pcs + --oversample is at most 32")
    p.add_argument("--iters", type=int, default=10, help="rounds of subspace iteration (default 10)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--pimin", type=float, default=0.01,
                   help="leave out a call whose individual-specific allele frequency is outside [pimin, 1 - pimin] (default 0.01): its "
                        "standardised residual is heavy-tailed")
    p.add_argument("--pops_path", type=str, default=None, metavar="FILE",
                   help="one group label per sample, used only to name the groups at the two ends of a flagged PC (default: every "
                        "sample goes to its largest component, the groups are named 1..K)")
    p.add_argument("--warn", type=float, default=1.5,
                   help="log a warning for every PC whose eigenvalue exceeds this many times the Marchenko-Pastur edge (default 1.5: a "
                        "convention, not a calibration; LD between SNPs inflates the whole spectrum)")
    return p.parse_args(argv)


def parse_hwe_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture hwe",
                                description="Hardy-Weinberg test given ancestry: a per-SNP score test from a run's .P and .Q files")
    _add_run_args(p, multi_k=False)
    p.add_argument("--pimin", type=float, default=0.0,
                   help="drop a call whose individual-specific allele frequency is outside [pimin, 1 - pimin] (default 0: every observed "
                        "call counts); the score is heavy-tailed for rare variants, 0.01 to 0.05 guards against that")
    p.add_argument("--alpha", type=float, default=1e-6,
                   help="a SNP whose two-sided p-value is below this goes to the .hwe.out list (default 1e-6, plink's customary --hwe threshold)")
    return p.parse_args(argv)


def parse_date_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture date",
                                description="Admixture dating: the decay of weighted admixture LD with genetic distance (ROLLOFF / "
                                            "ALDER's statistic, summed over every SNP pair), from a run's .P and .Q files and the "
                                            "genetic map of the .bim.  Use data that was NOT LD-pruned")
    _add_run_args(p, multi_k=True, out="curves and dates")
    p.add_argument("--pops_path", type=str, default=None, metavar="FILE",
                   help="one group label per sample of the .fam; with --target, the samples to date")
    p.add_argument("--target", type=str, default=None, metavar="LABEL",
                   help="date the samples whose line of --pops_path is LABEL (default: every sample left after --keep / --remove)")
    p.add_argument("--min_share", type=float, default=0.05,
                   help="a curve is computed for every pair of components whose two mean shares in the group are both at least this (default 0.05)")
    p.add_argument("--pairs", type=str, default=None, metavar="a-b,...",
                   help="the component pairs to date, 1-based like the columns of the .Q file (e.g. 1-3,2-3), instead of --min_share's choice")
    p.add_argument("--binsize", type=float, default=0.05, help="bin width in cM (default 0.05, ALDER's convention)")
    p.add_argument("--mindist", type=float, default=0.5,
                   help="fit from this distance in cM on (default 0.5, ALDER's convention: background LD inside the sources sits below that)")
    p.add_argument("--maxdist", type=float, default=20.0, help="fit up to this distance in cM (default 20, ALDER's convention)")
    p.add_argument("--morgans", action="store_true", help="column 3 of the .bim is in Morgans (default: cM)")
    p.add_argument("--rate", type=float, default=1.0, metavar="CM_PER_MB",
                   help="where column 3 of the .bim is all zero: this many cM per Mb applied to the base-pair column (default 1.0); the "
                        "date scales with it")
    p.add_argument("--nmin", type=int, default=2, help="leave out a SNP pair with fewer jointly observed samples than this (default 2)")
    return p.parse_args(argv)


def parse_local_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture local",
                                description="Local ancestry: the posterior ancestry of every sample along the genome under the linkage "
                                            "model (one rate, single pulse, unphased), from a run's .P and .Q files and the genetic map of "
                                            "the .bim.  The model has no LD inside a source: prune first and pass the list with --extract")
    _add_run_args(p, multi_k=True, out="calls and tables")
    p.add_argument("--generations", type=str, default="auto", metavar="X|auto",
                   help="generations since admixture (e.g. from `date`); auto (default): the value that maximises the log-likelihood")
    p.add_argument("--grid", type=float, default=0.5, help="distance in cM between the points at which the posterior is written (default 0.5)")
    p.add_argument("--scan_samples", type=int, default=512, help="--generations auto looks at no more than this many samples (default 512)")
    p.add_argument("--morgans", action="store_true", help="column 3 of the .bim is in Morgans (default: cM)")
    p.add_argument("--rate", type=float, default=1.0, metavar="CM_PER_MB",
                   help="where column 3 of the .bim is all zero: this many cM per Mb applied to the base-pair column (default 1.0)")
    p.add_argument("--dosage", action="store_true", help="also write {out_name}.{K}.lanc.dosage.npy, float32 [N, points, K]")
    p.add_argument("--pops_path", type=str, default=None, metavar="FILE",
                   help="one group label per sample of the .fam; with --target, the samples to analyse")
    p.add_argument("--target", type=str, default=None, metavar="LABEL",
                   help="analyse the samples whose line of --pops_path is LABEL (default: every sample left after --keep / --remove)")
    p.add_argument("--warn", type=float, default=4.0,
                   help="warn of a sample whose mean local share is further from its Q than this many times the other samples' spread "
                        "(default 4, a convention)")
    return p.parse_args(argv)


def _add_cv_refit(p):
    p.add_argument("--cv_rounds", type=int, default=50, metavar="N",
                   help="round limit of a fold's refit (default 50).  The refit starts from the full-data answer, which has seen the "
                        "held-out calls: stopped early it leaks, and the error of a K that is too large comes out too low")
    p.add_argument("--cv_tol", type=float, default=1e-5,
                   help="stop a fold's refit once no entry of Q or P moves by this much in a round")


def _add_boot_refit(p):
    p.add_argument("--block", type=int, default=1, metavar="SNPS",
                   help="SNPs are resampled in blocks of this many consecutive SNPs (default 1, ADMIXTURE's per-SNP bootstrap, which "
                        "takes the SNPs as independent); on data that was not LD-pruned use a block of hundreds of SNPs")
    p.add_argument("--boot_rounds", type=int, default=50, metavar="N",
                   help="round limit of a replicate's refit (default 50).  A replicate starts at the estimate: stopped early it has "
                        "not moved far from it, and the standard error comes out too small")
    p.add_argument("--boot_tol", type=float, default=1e-5,
                   help="stop a replicate's refit once no entry of Q or P moves by this much in a round")


def parse_bootstrap_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture bootstrap",
                                description="Bootstrap standard errors of Q: SNPs resampled with replacement, from a run's .P and .Q files")
    _add_run_args(p, multi_k=True)
    p.add_argument("-B", "--replicates", type=int, default=200, help="bootstrap replicates (default 200, ADMIXTURE's)")
    _add_boot_refit(p)
    p.add_argument("--seed", type=int, default=42, help="seed of the draw")
    return p.parse_args(argv)


def parse_pse_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture pse",
                                description="Standard errors of P: the per-SNP Fisher information given Q, from a run's .P and .Q files")
    _add_run_args(p, multi_k=True)
    p.add_argument("--bound", type=float, default=1e-4,
                   help="a frequency within this of 0 or 1 is taken as fixed at the boundary and gets no standard error (default 1e-4)")
    return p.parse_args(argv)


def parse_qse_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture qse",
                                description="Standard errors of Q given P: the per-sample Fisher information, from a run's .P and .Q files")
    _add_run_args(p, multi_k=True)
    p.add_argument("--bound", type=float, default=1e-4,
                   help="a fraction within this of 0 or 1 is counted as at the bound: its standard error is a detection limit (default 1e-4)")
    return p.parse_args(argv)


def parse_fit_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture fit",
                                description="Model-fit check: pairwise correlation of leave-one-out residuals (evalAdmix's statistic), "
                                            "from a run's .P and .Q files")
    _add_run_args(p, multi_k=True)
    p.add_argument("--pops_path", type=str, default=None, metavar="FILE",
                   help="one group label per sample, used only for the summary (default: every sample goes to its largest component, the "
                        "groups are named 1..K)")
    p.add_argument("--subsample", type=int, default=0, metavar="S",
                   help="take the pairs among a seeded subset of S <= 4096 samples (the work grows with S^2; the frequencies are still "
                        "refitted from every sample).  Needed above 4096 samples.  0 (default): every sample")
    p.add_argument("--seed", type=int, default=42, help="seed of the --subsample draw")
    p.add_argument("--matrix", action="store_true", help="also write the S x S matrix of correlations, {out_name}.{K}.cor")
    p.add_argument("--warn", type=float, default=0.02,
                   help="log a warning for every group pair whose mean correlation exceeds this in magnitude (default 0.02: a convention, "
                        "not a calibration -- the spread of a pair's correlation under a good fit is about 1 / sqrt(SNPs both were called at))")
    return p.parse_args(argv)


def parse_cv_args(argv):
    p = argparse.ArgumentParser(prog="neural-admixture cv",
                                description="Cross-validation error for choosing K: held-out genotype calls, from a run's .P and .Q files")
    _add_run_args(p, multi_k=True, out="file")
    p.add_argument("--folds", type=int, default=5, help="folds the observed calls are cut into (default 5, ADMIXTURE's)")
    _add_cv_refit(p)
    p.add_argument("--seed", type=int, default=42, help="seed of the fold draw")
    return p.parse_args(argv)


def _check_cv_refit(folds, args, flag):
    """The checks `cv` and `train --cv` share: ``folds`` came with ``flag``."""
    if not 2 <= folds <= 64:
        raise SystemExit(f"    {flag} must be in 2..64.")
    if args.cv_rounds < 1:
        raise SystemExit("    --cv_rounds must be >= 1.")
    if not args.cv_tol >= 0.0:
        raise SystemExit("    --cv_tol must be >= 0.")
    if args.seed < 0:
        raise SystemExit("    --seed must be >= 0.")


def _check_boot_refit(B, args, flag):
    """The checks `bootstrap` and `train --bootstrap` share: ``B`` came with ``flag``."""
    if B < 2:
        raise SystemExit(f"    {flag} must be >= 2.")
    if args.block < 1:
        raise SystemExit("    --block must be >= 1.")
    if args.boot_rounds < 1:
        raise SystemExit("    --boot_rounds must be >= 1.")
    if not args.boot_tol >= 0.0:
        raise SystemExit("    --boot_tol must be >= 0.")
    if args.seed < 0:
        raise SystemExit("    --seed must be >= 0.")


def _check_polish(rounds, args, flag):
    if rounds < 0:
        raise SystemExit(f"    {flag} takes a number of rounds >= 0.")


_CHECK_VALUES = {"polish": _check_polish, "cv": _check_cv_refit, "bootstrap": _check_boot_refit}    # by train()'s keyword
_DEST = {"boot_block": "block"}                           # train()'s keywords whose flag has another name


def _check_after_training(args, before_gpu):
    """The refusals of `train`'s after-training options (train.AFTER_TRAINING), in their words throughout: an option's own values,
    then a sharded run, a supervised one and a K above 16.  ``before_gpu``: the options refused before the GPU check, like an
    analysis mode's arguments, or those refused after it; both before any data is read."""
    for opt in AFTER_TRAINING:
        value, flag = getattr(args, opt.kw), "--" + opt.kw
        if opt.cli_before_gpu != before_gpu or not value:
            continue
        if opt.kw in _CHECK_VALUES:
            _CHECK_VALUES[opt.kw](value, args, flag)
        if args.num_gpus > 1:
            raise SystemExit(f"    {flag} is single-GPU: run it with --num_gpus 1 (a sharded run holds a part of the samples or of P).")
        if args.pops_path:
            raise SystemExit(f"    {flag} ignores labels: it is not available with --pops_path (supervised runs).")
        if opt.k16 is not None and (args.k is not None or args.max_k is not None):
            _check_ks16([args.k if args.k is not None else args.max_k], flag, opt.kw)


def _need_gpu():
    if not torch.cuda.is_available():
        raise SystemExit("neural_admixture_amd needs a ROCm GPU; use the reference for --num_gpus 0 (CPU) runs.")


def _check_k_pimin(args):
    if args.k < 1 or args.k > 64:
        raise SystemExit("    --k must be in 1..64.")
    if not 0.0 <= args.pimin < 0.5:
        raise SystemExit("    --pimin must be in [0, 0.5).")


def _need_bed(data_path, why, formats=".bed"):
    """Ends the run unless the input is a BED: a VCF with ``why`` (what needs a .bim), anything else naming ``formats``."""
    name = os.path.basename(data_path)
    if ".vcf" in name:
        raise SystemExit(f"    {why}: it is not available for VCF input.")
    if ".bed" not in name:
        raise SystemExit(f"    Invalid format. Unrecognized file format. Make sure file ends with {formats}.")


def _bed_shape(data_path, need_bim=True):
    """(N, M, .bim path) of a BED input from the .fam file and the size of the .bed, without reading a genotype; a missing file (the
    .bim only with ``need_bim``) or a .bed that does not hold whole SNPs ends the run, naming it."""
    from pathlib import Path
    base = Path(data_path)
    bim, fam, bed = base.with_suffix(".bim"), base.with_suffix(".fam"), base.with_suffix(".bed")
    for f in (bim, fam, bed) if need_bim else (fam, bed):
        if not f.is_file():
            raise SystemExit(f"    {f} not found.")
    with open(fam) as fb:
        n = sum(1 for _ in fb)
    nb = (n + 3) // 4
    if n < 1 or (bed.stat().st_size - 3) < nb or (bed.stat().st_size - 3) % nb:
        raise SystemExit(f"    {bed} does not hold whole SNPs of the {n} samples of {fam}.")
    return n, (bed.stat().st_size - 3) // nb, bim


def _bed_ids(data_path):
    """(N, M, .bim path, SNP IDs, chromosome labels) of a BED input, before any genotype is read: ``_bed_shape`` and a .bim with one
    line per SNP of the .bed."""
    n, m, bim = _bed_shape(data_path)
    ids, chroms = read_bim(bim)
    if len(ids) != m:
        raise SystemExit(f"    {bim} lists {len(ids)} SNPs, the .bed holds {m}.")
    return n, m, bim, ids, chroms


def _extract_keep(data_path, extract):
    """--extract FILE -> bool [M] over the SNPs of the .bim, before any genotype is read; None without the flag.  VCF input, an unknown
    ID and a listed ID that the .bim holds twice end the run, naming the offender."""
    if not extract:
        return None
    _need_bed(data_path, "--extract resolves SNP IDs through a .bim file", ".bed or .vcf")
    if not os.path.isfile(extract):
        raise SystemExit(f"    {extract} not found.")
    _, m, bim, ids, _ = _bed_ids(data_path)
    keep = resolve_ids(ids, read_id_list(extract), str(bim), extract)
    log.info(f"    --extract: {int(keep.sum())} of {m} SNPs.")
    return keep


def _fam_ids(data_path):
    """The (FID, IID) of every sample of a BED input, before any genotype is read: ``_bed_shape`` and the .fam's first two columns."""
    from pathlib import Path
    _bed_shape(data_path, need_bim=False)
    return read_fam(Path(data_path).with_suffix(".fam"))


def _sample_keep(args):
    """--keep FILE / --remove FILE -> bool [N] over the samples of the .fam, before any genotype is read; None without either flag.
    VCF input, a missing file, non-unique IDs in the .fam and a name it does not hold end the run, naming the offender."""
    flag = "--keep" if args.keep else "--remove" if args.remove else None
    if flag is None:
        return None
    path = args.keep or args.remove
    _need_bed(args.data_path, f"{flag} resolves sample IDs through a .fam file", ".bed or .vcf")
    if not os.path.isfile(path):
        raise SystemExit(f"    {path} not found.")
    fam = _fam_ids(args.data_path)
    from pathlib import Path
    named = resolve_samples(fam, read_sample_list(path), str(Path(args.data_path).with_suffix(".fam")), path)
    keep = named if args.keep else ~named
    if not keep.any():
        raise SystemExit(f"    {flag} {path} leaves no sample.")
    return keep


def _filter_lines(lines, samples, path):
    """The lines of a one-line-per-sample-of-the-.fam file (``--pops_path``) that belong to the samples --keep / --remove leave."""
    if samples is None:
        return lines
    if len(lines) != len(samples):
        raise SystemExit(f"    {path} holds {len(lines)} lines, the .fam {len(samples)} samples (one line per sample of the .fam, "
                         "before --keep / --remove).")
    return [ln for ln, k in zip(lines, samples) if k]


def _read_on_gpu(args, keep=None, samples=None):
    """What an analysis mode does once its arguments and files are in order: the GPU check, the host threads, the genotypes in HBM."""
    _need_gpu()
    torch.set_num_threads(max(1, args.threads))
    return _read(args.data_path, torch.device("cuda:0"), keep_on_device=True, keep=keep, samples=samples)


def _out_stem(args):
    """``{save_dir}/{out_name}``, --name where no --out_name was given; makes the directory."""
    os.makedirs(args.save_dir, exist_ok=True)
    return os.path.join(args.save_dir, args.out_name or args.name)


def _write_id_lists(stem, ids, keep):
    """``{stem}.in`` and ``{stem}.out``: the kept and the removed SNP IDs, one per line in the order given."""
    write_id_list(f"{stem}.in", [s for s, k in zip(ids, keep) if k])
    write_id_list(f"{stem}.out", [s for s, k in zip(ids, keep) if not k])


def _prune_main(argv):
    """``prune`` mode: {save_dir}/{name}.prune.in and .prune.out, the kept and the removed SNP IDs of the .bim, one per line in file
    order (readable by plink --extract and by --extract here)."""
    from . import ld
    args = parse_prune_args(argv)
    if args.window < 2 or args.window > ld.MAX_WINDOW:
        raise SystemExit(f"    --window must be in 2..{ld.MAX_WINDOW}.")
    if not 0.0 <= args.r2 <= 1.0:
        raise SystemExit("    --r2 must be in [0, 1].")
    _need_bed(args.data_path, "prune needs the SNP IDs and chromosomes of a .bim file")
    _, _, _, ids, chroms = _bed_ids(args.data_path)         # before the GPU check and before any genotype is read
    samples = _sample_keep(args)
    data = _read_on_gpu(args, samples=samples)
    keep, stats = ld.prune(data.packed, data.M, args.window, args.r2, chrom=chrom_codes(chroms))
    os.makedirs(args.save_dir, exist_ok=True)
    _write_id_lists(os.path.join(args.save_dir, f"{args.name}.prune"), ids, keep)
    log.info(f"    LD pruning (window {args.window}, r2 {args.r2:g}): {stats['kept']} SNPs kept, {stats['removed']} removed "
             f"({stats['seconds']:.2f} seconds; {stats['ranges']} ranges).")
    log.info("    SNP lists saved.")


def _pca_main(argv):
    """``pca`` mode: the genotypes alone -> {out_name}.eigenval (one eigenvalue per line) and {out_name}.eigenvec (plink's layout: two
    identifier columns, here the 0-based sample index as the ``kinship`` mode names samples, then PC1 ..)."""
    from . import pca
    args = parse_pca_args(argv)
    try:
        pca.check_args(args.pcs, args.oversample, args.iters, args.maf)
    except RuntimeError as e:
        raise SystemExit(f"    {e}") from None
    keep = _extract_keep(args.data_path, args.extract)     # before the GPU check and before any genotype is read
    samples = _sample_keep(args)
    name = os.path.basename(args.data_path)
    if ".vcf" in name:
        if not os.path.isfile(args.data_path):
            raise SystemExit(f"    {args.data_path} not found.")
    elif ".bed" in name:
        _bed_shape(args.data_path, need_bim=False)
    else:
        raise SystemExit("    Invalid format. Unrecognized file format. Make sure file ends with .bed or .vcf.")
    data = _read_on_gpu(args, keep, samples)
    res = pca.pca(data.packed, data.M, pcs=args.pcs, oversample=args.oversample, iters=args.iters, maf=args.maf, seed=args.seed)
    pca.log_result(res, log)
    pca.write_result(_out_stem(args), res)
    log.info("    Eigenvalues and eigenvectors saved.")


def _hwe_main(argv):
    """``hwe`` mode: {save_dir}/{name}.{k}.P and .Q + the genotypes -> {out_name}.{k}.hwe (``id n het_obs het_exp F Z p`` per SNP in
    file order) and {out_name}.{k}.hwe.in / .hwe.out, the kept and the removed SNP IDs (readable by --extract)."""
    from . import hwe
    args = parse_hwe_args(argv)
    _check_k_pimin(args)
    if not 0.0 < args.alpha <= 1.0:
        raise SystemExit("    --alpha must be in (0, 1].")
    _need_bed(args.data_path, "hwe needs the SNP IDs of a .bim file")
    paths = _find_run_heads(args, [args.k], "hwe")         # before anything is read
    _, _, _, ids, _ = _bed_ids(args.data_path)              # before the GPU check and before any genotype is read
    keep = _extract_keep(args.data_path, args.extract)     # (the .P then has one row per listed SNP)
    if keep is not None:
        ids = [s for s, k in zip(ids, keep) if k]
    data, (P,), (Q,) = _load_run_heads(args, [args.k], paths, keep)
    res = hwe.snp_hwe(data.packed, data.M, P, Q, pimin=args.pimin)
    kept = hwe.hwe_keep(res.p, args.alpha, res.n)
    stem = f"{_out_stem(args)}.{args.k}.hwe"
    hwe.write_table(stem, ids, res)
    _write_id_lists(stem, ids, kept)
    Z = res.Z.cpu().numpy()
    Z = Z[~np.isnan(Z)]
    med, sd = (float(np.median(Z)), float(np.std(Z))) if len(Z) else (float("nan"), float("nan"))
    log.info(f"    Hardy-Weinberg test given ancestry (pimin {args.pimin:g}): {len(Z)} of {len(ids)} SNPs tested, "
             f"{int((~kept).sum())} removed at p < {args.alpha:g}.")
    log.info(f"    Z over the tested SNPs: median {med:.3f}, standard deviation {sd:.3f} (the model expects 0 and 1).")
    if sd > 1.2:
        log.info(f"    Warning: the standard deviation of Z is {sd:.2f}; K may be too small or the panel related.")
    log.info("    Test table and SNP lists saved.")


def _ks_asked(args):
    """The K list of --k or --min_k .. --max_k."""
    if args.k is not None and (args.min_k is not None or args.max_k is not None):
        raise SystemExit("    --k cannot be given together with --min_k / --max_k.")
    if args.k is not None:
        ks = [args.k]
    elif args.min_k is not None and args.max_k is not None:
        if args.max_k < args.min_k:
            raise SystemExit("    --max_k must be >= --min_k.")
        ks = list(range(args.min_k, args.max_k + 1))
    else:
        raise SystemExit("    Please provide either --k or both --min_k and --max_k.")
    if ks[0] < 1 or ks[-1] > 64:
        raise SystemExit("    --k, --min_k and --max_k must be in 1..64.")
    return ks


def _find_run_heads(args, ks, mode):
    """The paths of {save_dir}/{name}.{K}.P and .Q of every K, ``(P_paths, Q_paths)``: an input that is neither BED nor VCF, or a
    missing file, ends the run (``mode``: who asks) before anything is read."""
    name = os.path.basename(args.data_path)
    if ".bed" not in name and ".vcf" not in name:
        raise SystemExit("    Invalid format. Unrecognized file format. Make sure file ends with .bed or .vcf.")
    return find_run_files(args.save_dir, args.name, ks, "P", mode), find_run_files(args.save_dir, args.name, ks, "Q", mode)


def _load_run_heads(args, ks, paths, keep, check_n=None):
    """The files of ``_find_run_heads`` + the genotypes in HBM -> (data, Ps, Qs).  Every file is read and checked before the GPU check:
    the widths always, the row counts where the input tells N and M without reading a genotype (.bed: the .fam file and the size of
    the .bed), else once it is parsed; a matrix of the wrong shape ends the run, naming its file.  ``keep``: what --extract selects
    (the .P files then have one row per listed SNP).  ``check_n(N)``: a mode's own check of the sample count, as early as N is known."""
    P_paths, Q_paths = paths
    n_known = m_known = None
    samples = _sample_keep(args)                           # (the .Q files then have one row per kept sample)
    if ".bed" in os.path.basename(args.data_path):
        n_known, m_known, _ = _bed_shape(args.data_path, need_bim=False)
        if keep is not None:
            m_known = int(keep.sum())
        if samples is not None:
            n_known = int(samples.sum())
    Qs = [read_run_matrix(p, k, n_known) for p, k in zip(Q_paths, ks)]
    Ps = [read_run_matrix(p, k, m_known, "model" if m_known is not None else "data") for p, k in zip(P_paths, ks)]
    if check_n is not None and n_known is not None:
        check_n(n_known)
    data = _read_on_gpu(args, keep, samples)
    if check_n is not None and n_known is None:
        check_n(data.N)
    for paths_, mats, rows in ((Q_paths, Qs, data.N), (P_paths, Ps, data.M)):
        for path, a in zip(paths_, mats):
            if a.shape[0] != rows:
                raise SystemExit(f"    {path} holds a {a.shape[0]} x {a.shape[1]} matrix, the data needs {rows} x {a.shape[1]}.")
    return data, Ps, Qs


def _read_run_heads(args, ks, mode, check_n=None):
    """What an analysis mode over a run's files does once its own arguments are in order: the files are looked for, then --extract is
    resolved, then ``_load_run_heads``."""
    paths = _find_run_heads(args, ks, mode)
    return _load_run_heads(args, ks, paths, _extract_keep(args.data_path, args.extract), check_n)


def _cv_main(argv):
    """``cv`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> one ``CV error (K=k): x`` line per K
    in the log and {out_name}.cv (``K cv_error se n_heldout rounds`` per K)."""
    from . import cv
    args = parse_cv_args(argv)
    ks = _ks_asked(args)
    _check_cv_refit(args.folds, args, "--folds")
    data, Ps, Qs = _read_run_heads(args, ks, "cv")
    log.info(f"    Cross-validation over held-out calls: {args.folds} folds, at most {args.cv_rounds} refit rounds per fold.")
    results = cv.cv_error(data.packed, data.M, Ps, Qs, args.folds, args.cv_rounds, args.cv_tol, args.seed)
    cv.log_results(results, log)
    cv.write_table(f"{_out_stem(args)}.cv", results)
    log.info("    Cross-validation table saved.")


def _bootstrap_main(argv):
    """``bootstrap`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> {out_name}.{K}.Q_se and .Q_bias
    (N x K, the .Q text format) and one ``Bootstrap SE (K=k)`` line per K in the log."""
    from . import bootstrap
    args = parse_bootstrap_args(argv)
    ks = _ks_asked(args)
    _check_boot_refit(args.replicates, args, "-B / --replicates")
    data, Ps, Qs = _read_run_heads(args, ks, "bootstrap")
    log.info(f"    Bootstrap over SNPs: {args.replicates} replicates, blocks of {args.block}, at most {args.boot_rounds} refit rounds each.")
    results = bootstrap.bootstrap_q(data.packed, data.M, Ps, Qs, args.replicates, args.block, args.boot_rounds, args.boot_tol, args.seed)
    bootstrap.log_results(results, log, args.boot_rounds)
    bootstrap.write_results(args.save_dir, args.out_name or args.name, results)
    log.info("    Standard errors and biases of Q saved.")


def _check_ks16(ks, who, option):
    """The check a mode and its option of `train` share (``option``: train()'s keyword): the K list came with ``who``."""
    if max(ks) > 16:
        reason = next(opt.k16 for opt in AFTER_TRAINING if opt.kw == option)
        raise SystemExit(f"    {who} needs every K <= 16: {reason} (K = {max(ks)} was asked for).")


def _pse_main(argv):
    """``pse`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> {out_name}.{K}.P_se (M x K, the .P text
    format, nan where no standard error is defined) and one ``P standard errors (K=k)`` line per K in the log."""
    from . import pse
    args = parse_pse_args(argv)
    ks = _ks_asked(args)
    _check_ks16(ks, "pse", "p_se")
    if not 0.0 <= args.bound < 0.5:
        raise SystemExit("    --bound must be in [0, 0.5).")
    data, Ps, Qs = _read_run_heads(args, ks, "pse")
    log.info(f"    Standard errors of P given Q (expected Fisher information per SNP; fixed within {args.bound:g} of 0 or 1).")
    results = [pse.p_se(data.packed, data.M, P, Q, bound=args.bound) for P, Q in zip(Ps, Qs)]
    pse.log_results(results, log)
    pse.write_results(args.save_dir, args.out_name or args.name, results)
    log.info("    Standard errors of P saved.")


def _qse_main(argv):
    """``qse`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> {out_name}.{K}.Q_info_se (N x K, the .Q
    text format, nan throughout a sample without a standard error) and the ``Q standard errors given P (K=k)`` lines per K in the log."""
    from . import qse
    args = parse_qse_args(argv)
    ks = _ks_asked(args)
    _check_ks16(ks, "qse", "q_se")
    if not 0.0 <= args.bound < 0.5:
        raise SystemExit("    --bound must be in [0, 0.5).")
    data, Ps, Qs = _read_run_heads(args, ks, "qse")
    log.info(f"    Standard errors of Q given P (expected Fisher information per sample, every component free under the sum constraint; "
             f"at the bound within {args.bound:g} of 0 or 1).")
    results = [qse.q_se(data.packed, data.M, P, Q, bound=args.bound) for P, Q in zip(Ps, Qs)]
    qse.log_results(results, log)
    qse.write_results(args.save_dir, args.out_name or args.name, results)
    log.info("    Standard errors of Q saved.")


def _fit_main(argv):
    """``fit`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> {out_name}.{K}.cor_pop (a header line of
    group names, then the G x G mean correlations of leave-one-out residuals), {out_name}.{K}.cor_sample (``mean_cor n_pairs`` per
    sample), with --matrix {out_name}.{K}.cor (S x S, the .Q text format), and the summary and warning lines per K in the log."""
    from . import fitcheck
    args = parse_fit_args(argv)
    ks = _ks_asked(args)
    _check_ks16(ks, "fit", "fit_check")
    if not args.warn >= 0.0:
        raise SystemExit("    --warn must be >= 0.")
    if args.subsample != 0 and not 2 <= args.subsample <= fitcheck.MAX_ROWS:
        raise SystemExit(f"    --subsample must be in 2..{fitcheck.MAX_ROWS}.")
    if args.seed < 0:
        raise SystemExit("    --seed must be >= 0.")
    labels = None
    if args.pops_path is not None:
        if not os.path.isfile(args.pops_path):
            raise SystemExit(f"    {args.pops_path} not found.")
        with open(args.pops_path, "r") as fb:
            labels = [ln.strip() for ln in fb.read().splitlines()]

    def check_n(n):
        if labels is not None and len(labels) != n:
            raise SystemExit(f"    {args.pops_path} lists {len(labels)} labels, the data holds {n} samples.")
        if n > fitcheck.MAX_ROWS and args.subsample == 0:
            raise SystemExit(f"    The fit check takes the pairs of at most {fitcheck.MAX_ROWS} samples (its work grows with their square) "
                             f"and the data holds {n}: pass --subsample S with S <= {fitcheck.MAX_ROWS}.")
    data, Ps, Qs = _read_run_heads(args, ks, "fit", check_n)
    pairs = None
    if args.subsample != 0 and args.subsample < data.N:
        pairs = np.sort(np.random.default_rng(args.seed).choice(data.N, size=args.subsample, replace=False))
        log.info(f"    --subsample: the pairs among {args.subsample} of {data.N} samples (seed {args.seed}).")
    log.info("    Fit check: correlation of leave-one-out residuals; groups are " +
             ("the labels of --pops_path." if labels is not None else "the samples' largest components."))
    results = [fitcheck.fit_check(data.packed, data.M, P, Q, labels, pairs) for P, Q in zip(Ps, Qs)]
    fitcheck.log_results(results, log, args.warn)
    fitcheck.write_results(args.save_dir, args.out_name or args.name, results, matrix=args.matrix)
    log.info("    Residual correlations saved.")


def _residpca_main(argv):
    """``residpca`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes -> {out_name}.{K}.resid.eigenval and
    .resid.eigenvec (the ``pca`` mode's layout), the eigenvalue and its ratio to the Marchenko-Pastur edge per PC in the log, and for
    every PC above --warn a warning with the groups at its two ends and its five most extreme samples."""
    from . import residpca
    from .fitcheck import default_labels
    args = parse_residpca_args(argv)
    ks = _ks_asked(args)
    if max(ks) > residpca.MAX_K:
        raise SystemExit(f"    residpca needs every K <= 16: {residpca.TOO_WIDE} (K = {max(ks)} was asked for).")
    try:
        residpca.check_args(args.pcs, args.oversample, args.iters, args.pimin)
    except RuntimeError as e:
        raise SystemExit(f"    {e}") from None
    if not args.warn >= 0.0:
        raise SystemExit("    --warn must be >= 0.")
    labels = None
    if args.pops_path is not None:
        if not os.path.isfile(args.pops_path):
            raise SystemExit(f"    {args.pops_path} not found.")
        with open(args.pops_path, "r") as fb:
            labels = [ln.strip() for ln in fb.read().splitlines()]
        labels = _filter_lines(labels, _sample_keep(args), args.pops_path)

    def check_n(n):
        if labels is not None and len(labels) != n:
            raise SystemExit(f"    {args.pops_path} lists {len(labels)} labels, the data holds {n} samples.")
        if args.pcs > n:
            raise SystemExit(f"    --pcs {args.pcs} components were asked of {n} samples.")
    data, Ps, Qs = _read_run_heads(args, ks, "residpca", check_n)
    log.info("    Residual PCA given Q and P: standardised residuals, calls with a frequency outside "
             f"[{args.pimin:g}, {1.0 - args.pimin:g}] left out; groups are " +
             ("the labels of --pops_path." if labels is not None else "the samples' largest components."))
    results = [residpca.resid_pca(data.packed, data.M, P, Q, pcs=args.pcs, oversample=args.oversample, iters=args.iters,
                                  pimin=args.pimin, seed=args.seed) for P, Q in zip(Ps, Qs)]
    residpca.log_results(results, [labels if labels is not None else default_labels(Q)[0] for Q in Qs], log, args.warn)
    residpca.write_results(args.save_dir, args.out_name or args.name, results)
    log.info("    Residual eigenvalues and eigenvectors saved.")


def _date_main(argv):
    """``date`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes and the genetic map of the .bim ->
    {out_name}.{K}.wld (``d_cM pairs`` and one column per curve, a row per bin) and {out_name}.{K}.date (``a b generations se A se_A c
    z`` per curve), and a line per curve in the log."""
    from . import admixdate
    args = parse_date_args(argv)
    ks = _ks_asked(args)
    try:
        nbins = admixdate.check_args(args.binsize, args.mindist, args.maxdist, args.min_share)
    except RuntimeError as e:
        raise SystemExit(f"    {e}.") from None
    if not args.rate > 0.0:
        raise SystemExit("    --rate must be > 0 (cM per Mb).")
    if args.nmin < 2:
        raise SystemExit("    --nmin must be >= 2.")
    if args.target is not None and args.pops_path is None:
        raise SystemExit("    --target names a label of --pops_path: give that file.")
    pairs = None
    if args.pairs is not None:
        try:
            pairs = [tuple(int(v) - 1 for v in item.split("-")) for item in args.pairs.split(",")]
            ok = all(len(pr) == 2 and pr[0] != pr[1] and 0 <= min(pr) and max(pr) < min(ks) for pr in pairs)
        except ValueError:
            ok = False
        if not ok or len(pairs) < 1:
            raise SystemExit(f"    --pairs takes component pairs like 1-2,1-3: two different components in 1..{min(ks)} each.")
    _need_bed(args.data_path, "date needs the genetic map of a .bim file")
    labels = None
    if args.pops_path is not None:
        if not os.path.isfile(args.pops_path):
            raise SystemExit(f"    {args.pops_path} not found.")
        with open(args.pops_path, "r") as fb:
            labels = [ln.strip() for ln in fb.read().splitlines()]
    paths = _find_run_heads(args, ks, "date")              # before anything is read
    _, _, bim, _, chroms = _bed_ids(args.data_path)        # before the GPU check and before any genotype is read
    cm, from_rate = genetic_map(*read_bim_map(bim), morgans=args.morgans, rate=args.rate)
    keep = _extract_keep(args.data_path, args.extract)
    chrom = chrom_codes(chroms)
    if keep is not None:                                   # the map follows the kept SNPs
        cm, chrom = cm[keep], chrom[keep]
    try:
        admixdate.grid_cells(cm, chrom, args.binsize, nbins)
    except RuntimeError as e:
        raise SystemExit(f"    {bim}: {e}.") from None
    group = None
    if labels is not None:
        labels = _filter_lines(labels, _sample_keep(args), args.pops_path)
        if args.target is not None:
            group = np.asarray([lb == args.target for lb in labels], dtype=bool)
            if int(group.sum()) < 2:
                raise SystemExit(f"    --target {args.target}: {int(group.sum())} samples of {args.pops_path} carry that label; a "
                                 "covariance needs at least 2.")

    def check_n(n):
        if labels is not None and len(labels) != n:
            raise SystemExit(f"    {args.pops_path} lists {len(labels)} labels, the data holds {n} samples.")
        if n < 2:
            raise SystemExit("    date needs at least 2 samples.")
    data, Ps, Qs = _load_run_heads(args, ks, paths, keep, check_n)
    if from_rate:
        log.info(f"    Warning: column 3 of {bim} is all zero; the genetic map is {args.rate:g} cM per Mb of column 4, and every date "
                 "scales with that rate.")
    if keep is not None:
        log.info("    Warning: --extract is in use; if the list is LD-pruned, pruning has removed the signal that is dated here: run "
                 "date on the unpruned SNPs.")
    idx = None if group is None else torch.from_numpy(np.nonzero(group)[0].astype(np.int32)).to(data.packed.device)
    log.info(f"    Admixture dating of {data.N if group is None else int(group.sum())} samples: weighted LD in {nbins} bins of "
             f"{args.binsize:g} cM, fitted over [{args.mindist:g}, {args.maxdist:g}) cM, jackknife over {len(set(chrom.tolist()))} chromosomes.")
    for k, P, Q in zip(ks, Ps, Qs):
        try:
            res = admixdate.admix_date(data.packed, data.M, P, Q if group is None else Q[group], cm, chrom, idx=idx, pairs=pairs,
                                       binsize=args.binsize, dmin=args.mindist, maxdist=args.maxdist, min_share=args.min_share,
                                       nmin=args.nmin)
        except RuntimeError as e:
            raise SystemExit(f"    K={k}: {e}.") from None
        admixdate.log_results(res, k, log)
        admixdate.write_results(os.path.dirname(_out_stem(args)), args.out_name or args.name, k, res)
    log.info("    Weighted LD curves and dates saved.")


def _local_main(argv):
    """``local`` mode: {save_dir}/{name}.{K}.P and .Q for every K asked for + the genotypes and the genetic map of the .bim ->
    {out_name}.{K}.lanc (the called ancestry pair of every sample at every output point), .lanc.sample (per sample: log-likelihood,
    mean local share next to Q, switches, mean tract), .lanc.mean (per point: mean share and its deviation) and, with --dosage,
    .lanc.dosage.npy."""
    from . import localanc
    args = parse_local_args(argv)
    ks = _ks_asked(args)
    gens = None
    if args.generations != "auto":
        try:
            gens = float(args.generations)
        except ValueError:
            gens = float("nan")
        if not (gens > 0.0 and gens < float("inf")):
            raise SystemExit("    --generations takes a number > 0 or auto.")
    if not args.grid > 0.0:
        raise SystemExit("    --grid must be > 0 (cM).")
    if not args.rate > 0.0:
        raise SystemExit("    --rate must be > 0 (cM per Mb).")
    if args.scan_samples < 1:
        raise SystemExit("    --scan_samples must be >= 1.")
    if not args.warn > 0.0:
        raise SystemExit("    --warn must be > 0.")
    if max(ks) > localanc.MAX_K:
        raise SystemExit(f"    {localanc.TOO_WIDE}.")
    if args.target is not None and args.pops_path is None:
        raise SystemExit("    --target names a label of --pops_path: give that file.")
    _need_bed(args.data_path, "local needs the genetic map of a .bim file")
    labels = None
    if args.pops_path is not None:
        if not os.path.isfile(args.pops_path):
            raise SystemExit(f"    {args.pops_path} not found.")
        with open(args.pops_path, "r") as fb:
            labels = [ln.strip() for ln in fb.read().splitlines()]
    paths = _find_run_heads(args, ks, "local")             # before anything is read
    _, _, bim, ids, chroms = _bed_ids(args.data_path)      # before the GPU check and before any genotype is read
    cm_all, bp = read_bim_map(bim)
    cm, from_rate = genetic_map(cm_all, bp, morgans=args.morgans, rate=args.rate)
    keep = _extract_keep(args.data_path, args.extract)
    chrom = chrom_codes(chroms)
    if keep is not None:                                   # the map follows the kept SNPs
        cm, chrom, bp = cm[keep], chrom[keep], bp[keep]
        ids, chroms = [v for v, k in zip(ids, keep) if k], [v for v, k in zip(chroms, keep) if k]
    try:
        localanc.output_points(cm, chrom, args.grid)
    except RuntimeError as e:
        raise SystemExit(f"    {bim}: {e}.") from None
    group = None
    if labels is not None:
        labels = _filter_lines(labels, _sample_keep(args), args.pops_path)
        if args.target is not None:
            group = np.asarray([lb == args.target for lb in labels], dtype=bool)
            if int(group.sum()) < 1:
                raise SystemExit(f"    --target {args.target}: no sample of {args.pops_path} carries that label.")

    def check_n(n):
        if labels is not None and len(labels) != n:
            raise SystemExit(f"    {args.pops_path} lists {len(labels)} labels, the data holds {n} samples.")
    data, Ps, Qs = _load_run_heads(args, ks, paths, keep, check_n)
    if from_rate:
        log.info(f"    Warning: column 3 of {bim} is all zero; the genetic map is {args.rate:g} cM per Mb of column 4, and every tract "
                 "length scales with that rate.")
    if keep is None:
        log.info("    Warning: the model has no LD inside a source; on SNPs that were not LD-pruned the posterior is over-confident: run "
                 "prune and pass its list with --extract.")
    idx = None if group is None else torch.from_numpy(np.nonzero(group)[0].astype(np.int32)).to(data.packed.device)
    for k, P, Q in zip(ks, Ps, Qs):
        Qg = Q if group is None else Q[group]
        try:
            n = gens
            if n is None:
                n, grid, lls = localanc.scan_generations(data.packed, data.M, P, Qg, cm, chrom, idx=idx, scan_samples=args.scan_samples)
                for g_, l_ in zip(grid, lls):
                    log.info(f"    K={k}: {g_:9.3f} generations: log-likelihood {l_:.6e}")
                log.info(f"    K={k}: --generations auto chose {n:.4g}.")
            res = localanc.local_ancestry(data.packed, data.M, P, Qg, cm, chrom, n, idx=idx, grid=args.grid, dosage=args.dosage)
        except RuntimeError as e:
            raise SystemExit(f"    K={k}: {e}.") from None
        localanc.log_results(res, Qg, cm, k, log, args.warn)
        localanc.write_results(os.path.dirname(_out_stem(args)), args.out_name or args.name, k, res, Qg, cm, chroms, ids, bp)
    log.info("    Local ancestry calls and tables saved.")


def _king_main(argv):
    """``king`` mode: the genotypes alone -> {name}.king (``i j phi n hethet ibs0`` per pair at or above --cutoff, 0-based indices
    among the samples analysed, by i then j) and {name}.king.in / .king.out, the kept and the removed samples of ``king.unrelated_set`` as ``FID IID``
    lines of the .fam (readable by plink --keep / --remove and by --keep / --remove here)."""
    from pathlib import Path
    from . import king, relate
    from .io import check_unique_samples, write_sample_list
    args = parse_king_args(argv)
    if not args.cutoff == args.cutoff:
        raise SystemExit("    --cutoff must be a number.")
    if not 1 <= args.rows <= 4096:
        raise SystemExit("    --rows must be in 1..4096.")
    _need_bed(args.data_path, "king names the samples through a .fam file")
    fam = _fam_ids(args.data_path)                          # before the GPU check and before any genotype is read
    check_unique_samples(fam, str(Path(args.data_path).with_suffix(".fam")))
    keep = _extract_keep(args.data_path, args.extract)
    samples = _sample_keep(args)
    if samples is not None:
        fam = [s for s, k in zip(fam, samples) if k]
    data = _read_on_gpu(args, keep, samples)
    i, j, phi, n, hh, i0 = (v.cpu().numpy() for v in king.king_pairs(data.packed, data.M, args.cutoff, rows=args.rows))
    kept = king.unrelated_set(data.N, i, j)
    os.makedirs(args.save_dir, exist_ok=True)
    stem = os.path.join(args.save_dir, f"{args.name}.king")
    relate.write_pairs(stem, i, j, phi, n, hh, i0)
    write_sample_list(f"{stem}.in", [s for s, k in zip(fam, kept) if k])
    write_sample_list(f"{stem}.out", [s for s, k in zip(fam, kept) if not k])
    log.info(f"    {len(phi)} pairs with a KING-robust kinship coefficient >= {args.cutoff:.4f} among {data.N} samples:")
    for label, edge, count in relate.band_counts(phi):
        log.info(f"      {label} (>= {edge:.4f}): {count}")
    log.info(f"    {int((~kept).sum())} samples removed, {int(kept.sum())} kept: no two kept samples are related at the cutoff "
             f"(train --keep {args.name}.king.in, then infer --refine on the whole file).")
    log.info("    Kinship pairs and sample lists saved.")


def _kinship_main(argv):
    """``kinship`` mode: {save_dir}/{name}.{k}.P and .Q + the genotypes -> {out_name}.{k}.kin (``i j phi n`` per related pair, 0-based
    sample indices, by i then j) and {out_name}.{k}.inbreed (one inbreeding coefficient per sample); with --ibd also
    {out_name}.{k}.ibd (``i j phi n k0 k1 k2 ibs0 relation`` per listed pair) and the number of pairs per relation in the log."""
    from . import relate
    from .io import savetxt
    args = parse_kinship_args(argv)
    _check_k_pimin(args)
    if not args.min_phi == args.min_phi:
        raise SystemExit("    --min_phi must be a number.")
    if args.ibd and args.k > relate.MAX_K:
        raise SystemExit(f"    kinship --ibd needs K <= 16: {relate.TOO_WIDE} (K = {args.k} was asked for).")
    if not 0.0 < args.po_k0 < 0.25:
        raise SystemExit("    --po_k0 must be in (0, 0.25): between the k0 expected of a parent-offspring pair and of full siblings.")
    data, (P,), (Q,) = _read_run_heads(args, [args.k], "kinship")
    if args.ibd:
        i, j, phi, n, inb, k0, k1, k2, ibs0 = relate.ibd_pairs(data.packed, data.M, P, Q, args.min_phi, pimin=args.pimin)
    else:
        i, j, phi, n, inb = relate.kinship_pairs(data.packed, data.M, P, Q, args.min_phi, pimin=args.pimin)
    phi_h = phi.cpu().numpy()
    stem = f"{_out_stem(args)}.{args.k}"
    relate.write_pairs(f"{stem}.kin", i.cpu().numpy(), j.cpu().numpy(), phi_h, n.cpu().numpy())
    savetxt(f"{stem}.inbreed", inb.cpu().numpy().reshape(-1, 1))
    if args.ibd:
        k0_h = k0.cpu().numpy()
        labels = relate.relation(phi_h, k0_h, args.po_k0)
        relate.write_ibd(f"{stem}.ibd", i.cpu().numpy(), j.cpu().numpy(), phi_h, n.cpu().numpy(), k0_h, k1.cpu().numpy(), k2.cpu().numpy(),
                         ibs0.cpu().numpy(), labels)
        log.info(f"    IBD-sharing probabilities of the {len(labels)} listed pairs (first-degree pairs with k0 < {args.po_k0:g}: parent-offspring):")
        for label, count in relate.relation_counts(labels):
            if label != "unrelated" or count:
                log.info(f"      {label}: {count}")
    log.info(f"    {len(phi_h)} pairs with a kinship coefficient >= {args.min_phi:.4f} among {data.N} samples:")
    for label, edge, count in relate.band_counts(phi_h):
        log.info(f"      {label} (>= {edge:.4f}): {count}")
    close = int((phi_h >= relate.BANDS[2][0]).sum())
    if close:
        log.info(f"    Warning: {close} pairs are second-degree relatives or closer; related samples bias the fit "
                 "(the model assumes unrelated samples): consider removing one sample of each pair and training again "
                 "(the 'king' mode lists the samples to leave out: train --remove {name}.king.out).")
    log.info("    Kinship and inbreeding coefficients saved.")


def _read(path, device=None, keep_on_device=False, keep=None, samples=None):
    """The genotypes as PackedGenotypes; ``samples`` (bool per sample of the file, from --keep / --remove) and then ``keep`` (bool per
    SNP of the file, from --extract) select right after the read -- BED input only -- and everything downstream sees an ordinary
    PackedGenotypes of the kept ones."""
    from .io import read_bed_packed, read_vcf_packed
    name = os.path.basename(path)
    if ".vcf" in name:                                   # src/snp_reader.py:103
        log.info("    Input format is VCF.")
        data = read_vcf_packed(path, device, keep_on_device)
        log.info(f"    Data contains {data.N} samples and {data.M} SNPs.")
        return data
    if ".bed" not in name:
        raise SystemExit("    Invalid format. Unrecognized file format. Make sure file ends with .bed or .vcf (.pgen needs pgenlib "
                         "through the reference's own reader).")
    log.info("    Input format is BED.")
    data = read_bed_packed(path, device, keep_on_device)
    log.info(f"    Data contains {data.N} samples and {data.M} SNPs.")
    if samples is not None:
        from .king import select_samples
        data = select_samples(data, samples)
        log.info(f"    Using the {data.N} samples of --keep / --remove.")
    if keep is not None:
        from .ld import select_snps
        data = select_snps(data, keep)
        log.info(f"    Using the {data.M} SNPs of --extract.")
    return data


def _train_worker(rank, args, num_gpus, data, V, pops, t0):
    from .train import train
    from .io import save_model, write_outputs
    if num_gpus > 1:                                        # src/utils.py:69-95
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dev_id = 0 if args.share_gpu else rank
        torch.cuda.set_device(dev_id)
        torch.distributed.init_process_group("gloo" if args.share_gpu else "nccl", init_method="env://", rank=rank, world_size=num_gpus)
    else:
        dev_id = rank
    master = rank == 0
    device = torch.device(f"cuda:{dev_id}")
    K = args.k
    Ps, Qs, model = train(args.epochs, args.batch_size, args.learning_rate, K, args.seed, data, device, num_gpus, args.hidden_size,
                          master, V, pops, args.min_k, args.max_k, args.n_components, parallelism=args.parallelism,
                          host_threads=args.threads, gmm=args.gmm, precision=args.precision,
                          unlabelled=None if pops is None else (args.unlabelled,), supervised_loss_weight=args.supervised_loss_weight,
                          **{kw: getattr(args, _DEST.get(kw, kw)) for kw in AFTER_KEYWORDS})
    if master:
        save_model(model, args.name, args.save_dir)
        write_outputs(Qs, args.name, K, args.min_k, args.max_k, args.save_dir, Ps)
        for opt in AFTER_TRAINING:
            if opt.writer is not None and getattr(args, opt.kw):
                import_module("." + opt.writer, __package__).write_results(args.save_dir, args.name, model.after_results[opt.kw])
        log.info("    Q and P matrices saved." if K is not None else "    Q and P matrices saved for all K.")
        log.info("")
        log.info(f"    Total elapsed time: {time.time() - t0:.2f} seconds.")
    if num_gpus > 1:
        torch.distributed.destroy_process_group()


_ANALYSIS_MODES = {"king": _king_main, "kinship": _kinship_main, "prune": _prune_main, "hwe": _hwe_main, "cv": _cv_main, "bootstrap": _bootstrap_main,
                   "pse": _pse_main, "qse": _qse_main, "fit": _fit_main, "pca": _pca_main, "residpca": _residpca_main, "date": _date_main, "local": _local_main}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    assert argv and argv[0] in ("train", "infer", "king", "kinship", "prune", "hwe", "cv", "bootstrap", "pse", "qse", "fit", "pca", "residpca", "date", "local"), \
        ('Please provide either the argument "train" or "infer" to choose running mode ("king" finds relatives before a run, "kinship", "prune" and "hwe" check a run\'s assumptions, '
         '"cv" helps to choose K, "bootstrap" puts standard errors on Q, "pse" on P, "qse" on Q given P, "fit" checks the fit sample by sample, "pca" gives the principal components of the genotypes, "residpca" those of the model\'s residuals, "date" dates the admixture from the decay of weighted LD, "local" gives the ancestry along each genome).')
    mode, t0 = argv[0], time.time()
    if mode in _ANALYSIS_MODES:                             # (their argument and file checks come before the GPU check)
        _ANALYSIS_MODES[mode](argv[1:])
        log.info(f"    Total elapsed time: {time.time() - t0:.2f} seconds.")
        return 0
    if mode == "train":
        args = parse_train_args(argv[1:])
        _check_after_training(args, before_gpu=True)
    _need_gpu()
    if mode == "train":
        assert args.epochs > 0 and args.batch_size > 0 and args.learning_rate > 0 and args.hidden_size > 0 and args.n_components > 0
        _check_after_training(args, before_gpu=False)
        pops = None
        if args.pops_path:                                  # src/utils.py:28-33: one population name per line
            with open(args.pops_path, "r") as fb:
                pops = [ln.strip() for ln in fb.readlines()]
            assert args.k is not None, "Supervised mode needs --k (the number of populations in --pops_path)."
        if args.k is not None:
            assert args.k > 1, "Please select K > 1."
            log.info(f"    Running on K = {args.k}.")
        elif args.min_k is not None and args.max_k is not None:
            assert args.min_k > 1 and args.max_k > args.min_k
            log.info(f"    Running from K={args.min_k} to K={args.max_k}.")
        else:
            raise ValueError("Please provide either --k or both --min_k and --max_k.")
        num_gpus = max(1, args.num_gpus if args.share_gpu else min(args.num_gpus, torch.cuda.device_count()))   # entry.py:168-173
        for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS", "NUMEXPR_NUM_THREADS"):       # entry.py:138-146
            os.environ[var] = str(args.threads)              # for child processes (the concurrent GMM fits, spawned ranks) ...
        torch.set_num_threads(max(1, args.threads))          # ... this process's pools are already up: torch here, BLAS / OpenMP
                                                             # through train(host_threads=) (threadpoolctl)
        from .svd import RSVD
        keep = _extract_keep(args.data_path, args.extract)  # before any genotype is read
        samples = _sample_keep(args)
        if pops is not None:                                # (one line per sample of the .fam)
            pops = _filter_lines(pops, samples, args.pops_path)
        data = _read(args.data_path, torch.device("cuda:0"), keep_on_device=(num_gpus == 1), keep=keep, samples=samples)   # 2-bit transpose on the GPU
        log.info("")
        log.info("    Running SVD...")
        V = RSVD(data, data.N, data.M, args.n_components, args.seed)
        if num_gpus > 1:
            data.packed.share_memory_()
            torch.multiprocessing.spawn(_train_worker, args=(args, num_gpus, data, V, pops, t0), nprocs=num_gpus)
        else:
            _train_worker(0, args, 1, data, V, pops, t0)
        return 0
    args = parse_infer_args(argv[1:])
    if args.q_se and args.refine <= 0:                     # before anything is loaded
        raise SystemExit("    --q_se needs --refine N: the encoder's Q is not a maximum of the likelihood given P, and the standard "
                         "error would not belong to it.")
    if args.q_se and not 0.0 <= args.bound < 0.5:
        raise SystemExit("    --bound must be in [0, 0.5).")
    from .model import Q_P
    from .io import write_outputs
    keep = _extract_keep(args.data_path, args.extract)      # before anything is loaded
    samples = _sample_keep(args)
    with open(f"{args.save_dir}/{args.name}_config.json") as fb:
        cfg = json.load(fb)
    Ps = None
    if args.q_se:
        _check_ks16(cfg["ks"], "--q_se", "q_se")
    if args.refine > 0:                                    # the training run's {name}.{k}.P, looked for before anything is loaded
        P_paths = find_run_files(args.save_dir, args.name, cfg["ks"], "P", "--refine")
    sd = torch.load(f"{args.save_dir}/{args.name}.pt", map_location="cpu", weights_only=True)
    if args.refine > 0:                                    # one row per SNP of the model: V is [M, num_features]
        Ps = [read_run_matrix(p, k, int(sd["V"].shape[0]), "model") for p, k in zip(P_paths, cfg["ks"])]
    model = Q_P(int(cfg["hidden_size"]), int(cfg["num_features"]), ks_list=cfg["ks"], is_train=False)
    if args.precision != "highest":
        log.info(f"    Matmul precision: {args.precision} (bf16-class products in the genotype passes).")
    model.load_state_dict(sd, device=torch.device("cuda:0"), max_batch=args.batch_size, precision=args.precision)
    data = _read(args.data_path, torch.device("cuda:0"), keep_on_device=True, keep=keep, samples=samples)
    eng = model.engine
    eng.pack_from_host(data)
    idx = torch.arange(data.N, dtype=torch.int32, device=eng.device)
    outs = [[] for _ in cfg["ks"]]
    if Ps is not None:
        for h, P_MK in enumerate(Ps):
            eng.load_P(h, P_MK)
        ll0 = ll1 = 0.0
    if args.q_se:
        from . import qse
        Pd, ses = [torch.as_tensor(P_MK, dtype=torch.float32).to(eng.device) for P_MK in Ps], [[] for _ in cfg["ks"]]
    for s, bb in row_ranges(data.N, args.batch_size):     # engine.final_q's ranges, with the projection of a batch in between
        qs = eng.infer_q(idx[s:s + bb], bb)
        if Ps is not None:                                 # projection: the encoder's Q is the start of the masked EM steps
            _, lls, _ = eng.project_q(idx[s:s + bb], bb, q0=qs, iters=0, with_loglik=True)
            ll0 += float(sum(ll.sum() for ll in lls))
            qs, lls, _ = eng.project_q(idx[s:s + bb], bb, q0=qs, iters=args.refine, tol=args.refine_tol, with_loglik=True)
            ll1 += float(sum(ll.sum() for ll in lls))
            if args.q_se:                                  # at the refined Q, given the P it was refined against
                for h, q in enumerate(qs):
                    ses[h].append(qse.q_se(eng.xp, eng.M, Pd[h], q, idx[s:s + bb], bound=args.bound))
        for h, q in enumerate(qs):
            outs[h].append(q.cpu().numpy())
    if Ps is not None:
        log.info(f"    Log-likelihood of the observed calls before refinement: {ll0:.3f}")
        log.info(f"    Log-likelihood of the observed calls after refinement:  {ll1:.3f}")
    Qs = [np.concatenate(o, axis=0) for o in outs]
    K = cfg["ks"][0] if len(cfg["ks"]) == 1 else None
    write_outputs(Qs, args.out_name, K, cfg["ks"][0], cfg["ks"][-1], args.save_dir)
    if args.q_se:
        results = [qse.concat(r) for r in ses]
        qse.log_results(results, log)
        qse.write_results(args.save_dir, args.out_name, results)
        log.info("    Standard errors of Q saved.")
    log.info(f"    Total elapsed time: {time.time() - t0:.2f} seconds.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
