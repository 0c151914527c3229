#!/bin/bash
# Build libnadm.so and libnadm_testhooks.so (gfx950 only) next to this script.  hipcc cross-compiles without a GPU.
#   build.sh [-o OUT.so] [extra compile flags, e.g. -DNADM_BF_NTW=2 ...]
# -o: ONE library, without the test hooks, at that path, its objects in a directory of their own beside it (tools/build_variant.sh).
# The extra flags reach every unit: the kernel units and the host unit of the passes must agree on the shape macros (nadm_pass_args.h).
# This file is the one list of the library's units.
set -e
out=""
if [ "$1" = "-o" ]; then out=$(realpath -m "$2"); shift 2; fi
cd "$(dirname "$0")"
here=$(pwd)
obj=${out:+$out.obj}
obj=${obj:-$here}
mkdir -p "$obj"
HOST="-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
FLAGS="--offload-arch=gfx950 $HOST"
X="$*"
# One compile line per unit, up to NADM_BUILD_JOBS at a time (16 at the most).  (xargs -L 1: no line may end in a blank.)
# Kernel units:
#   nadm_genotype_passes, nadm_small_kernels   the kernels of the step and their launchers;  nadm_step: the plan
#   nadm_gmm_dev      the decoder-init mixture fit with the sums over the samples on the device
#   nadm_calib        measurement helper: the box fingerprint of bench.py (not on the training path)
#   nadm_project      projection: Q refined against a fixed P (nadm_project_q; not on the training path)
#   nadm_project_p    the other half: P refitted against a fixed Q (nadm_project_p; not on the training path)
#   nadm_kinship      admixture-aware kinship from Q and P on the matrix pipe (nadm_kinship; not on the training path)
#   nadm_ibd          IBD-sharing sums given ancestry (k0 / k1 / k2) from Q, P and f on the matrix pipe (nadm_ibd; not on the training path)
#   nadm_king         KING-robust kinship counts from the genotypes alone on the matrix pipe (nadm_king; not on the training path)
#   nadm_ld           LD pruning: windowed r^2 on the matrix pipe, SNP counts, SNP selection (not on the training path)
#   nadm_wld          admixture dating: weighted LD summed into bins of genetic distance on the matrix pipe (nadm_wld; not on the training path)
#   nadm_snp_hwe      Hardy-Weinberg score test given ancestry, per SNP (nadm_snp_hwe; not on the training path)
#   nadm_cv           cross-validation over held-out calls: the masked copy and the held-out deviance (not on the training path)
#   nadm_snp_info     standard errors of P: per-SNP Fisher information given Q (nadm_snp_info; not on the training path)
#   nadm_sample_info  standard errors of Q given P: per-sample Fisher information (nadm_sample_info; not on the training path)
#   nadm_resid_cor    model-fit check: EM sums and the correlation of leave-one-out residuals (nadm_em_sums, nadm_resid_cor; not on the training path)
#   nadm_obs_project  standardised PCA: the two observed-calls pair products on the matrix pipe (nadm_obs_project, nadm_obs_project_t; not on the training path)
#   nadm_resid_project  residual PCA given Q and P: the two products of the standardised residuals (nadm_resid_project, nadm_resid_project_t; not on the training path)
#   nadm_local_anc    local ancestry: the linkage model's forward-backward recursion along the genome (nadm_local_anc; not on the training path)
# Host-only units, compiled as plain C++ (no device pass):
#   nadm_passes_host  the entry points, argument checks and launch rules of the genotype passes and the MLP pair
#   nadm_gmm          decoder-init mixture fit on the host
#   nadm_host_io      host packer, .bed converter, VCF parser, savetxt
#   nadm_layout       head table + flat parameter layout
#   nadm_ld_sweep     the greedy sweep of LD pruning
# The test hooks (nadm_test_force_slices / _p3_slices / _generic_mlp) are the one difference between the two libraries: nadm_hooks.cpp
# without the macro has no setter and getters that return 0; with it, the setters exist.  Every other object, the kernels included, is
# linked into both.  The tests that need a hook re-run themselves in a child process against the TEST build (tests/conftest.py: in_hook_build).
xargs -P "${NADM_BUILD_JOBS:-8}" -L 1 hipcc <<UNITS
$X $FLAGS -c nadm_genotype_passes.hip -o $obj/nadm_genotype_passes.o
$X $FLAGS -c nadm_small_kernels.hip -o $obj/nadm_small_kernels.o
$X $FLAGS -c nadm_step.hip -o $obj/nadm_step.o
$X $FLAGS -c nadm_gmm_dev.hip -o $obj/nadm_gmm_dev.o
$X $FLAGS -c nadm_calib.hip -o $obj/nadm_calib.o
$X $FLAGS -c nadm_project.hip -o $obj/nadm_project.o
$X $FLAGS -c nadm_project_p.hip -o $obj/nadm_project_p.o
$X $FLAGS -c nadm_kinship.hip -o $obj/nadm_kinship.o
$X $FLAGS -c nadm_ibd.hip -o $obj/nadm_ibd.o
$X $FLAGS -c nadm_king.hip -o $obj/nadm_king.o
$X $FLAGS -c nadm_ld.hip -o $obj/nadm_ld.o
$X $FLAGS -c nadm_wld.hip -o $obj/nadm_wld.o
$X $FLAGS -c nadm_snp_hwe.hip -o $obj/nadm_snp_hwe.o
$X $FLAGS -c nadm_cv.hip -o $obj/nadm_cv.o
$X $FLAGS -c nadm_snp_info.hip -o $obj/nadm_snp_info.o
$X $FLAGS -c nadm_sample_info.hip -o $obj/nadm_sample_info.o
$X $FLAGS -c nadm_resid_cor.hip -o $obj/nadm_resid_cor.o
$X $FLAGS -c nadm_obs_project.hip -o $obj/nadm_obs_project.o
$X $FLAGS -c nadm_resid_project.hip -o $obj/nadm_resid_project.o
$X $FLAGS -c nadm_local_anc.hip -o $obj/nadm_local_anc.o
$X $HOST -c nadm_passes_host.cpp -o $obj/nadm_passes_host.o
$X $HOST -c nadm_gmm.cpp -o $obj/nadm_gmm.o
$X $HOST -c nadm_host_io.cpp -o $obj/nadm_host_io.o
$X $HOST -c nadm_layout.cpp -o $obj/nadm_layout.o
$X $HOST -c nadm_ld_sweep.cpp -o $obj/nadm_ld_sweep.o
$X $HOST -c nadm_hooks.cpp -o $obj/nadm_hooks.o
$X $HOST -DNADM_TEST_HOOKS -c nadm_hooks.cpp -o $obj/nadm_hooks_th.o
UNITS
OBJS="nadm_genotype_passes.o nadm_small_kernels.o nadm_step.o nadm_passes_host.o nadm_gmm.o nadm_gmm_dev.o nadm_calib.o nadm_project.o nadm_project_p.o nadm_kinship.o nadm_ibd.o nadm_king.o nadm_ld.o nadm_wld.o nadm_snp_hwe.o nadm_cv.o nadm_snp_info.o nadm_sample_info.o nadm_resid_cor.o nadm_obs_project.o nadm_resid_project.o nadm_local_anc.o nadm_host_io.o nadm_layout.o nadm_ld_sweep.o"
cd "$obj"
link="hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libnadm.so"
if [ -n "$out" ]; then
    $link -o "$out" $OBJS nadm_hooks.o -lpthread -ldl
    echo "built $out"
    exit 0
fi
$link -o "$here/libnadm.so" $OBJS nadm_hooks.o -lpthread -ldl
echo "built $here/libnadm.so"
$link -o "$here/libnadm_testhooks.so" $OBJS nadm_hooks_th.o -lpthread -ldl
echo "built $here/libnadm_testhooks.so"
