#!/bin/bash
# Build libnadm.so (gfx950 only) next to this script.  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
HOST="-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
FLAGS="--offload-arch=gfx950 $HOST"
hipcc $FLAGS -c nadm_genotype_passes.hip -o nadm_genotype_passes.o "$@"
hipcc $FLAGS -c nadm_small_kernels.hip -o nadm_small_kernels.o "$@"
hipcc $FLAGS -c nadm_step.hip -o nadm_step.o "$@"
hipcc $FLAGS -c nadm_gmm_dev.hip -o nadm_gmm_dev.o "$@"         # the decoder-init mixture fit with the sums over the samples on the device
hipcc $FLAGS -c nadm_calib.hip -o nadm_calib.o "$@"             # measurement helper: the box fingerprint of bench.py (not on the training path)
hipcc $FLAGS -c nadm_project.hip -o nadm_project.o "$@"         # projection: Q refined against a fixed P (nadm_project_q; not on the training path)
hipcc $FLAGS -c nadm_project_p.hip -o nadm_project_p.o "$@"     # the other half: P refitted against a fixed Q (nadm_project_p; not on the training path)
hipcc $FLAGS -c nadm_kinship.hip -o nadm_kinship.o "$@"         # admixture-aware kinship from Q and P on the matrix pipe (nadm_kinship; not on the training path)
hipcc $FLAGS -c nadm_ld.hip -o nadm_ld.o "$@"                   # LD pruning: windowed r^2 on the matrix pipe, SNP counts, SNP selection (not on the training path)
hipcc $FLAGS -c nadm_snp_hwe.hip -o nadm_snp_hwe.o "$@"         # Hardy-Weinberg score test given ancestry, per SNP (nadm_snp_hwe; not on the training path)
hipcc $FLAGS -c nadm_cv.hip -o nadm_cv.o "$@"                   # cross-validation over held-out calls: the masked copy and the held-out deviance (not on the training path)
hipcc $FLAGS -c nadm_snp_info.hip -o nadm_snp_info.o "$@"       # standard errors of P: per-SNP Fisher information given Q (nadm_snp_info; not on the training path)
hipcc $FLAGS -c nadm_resid_cor.hip -o nadm_resid_cor.o "$@"     # model-fit check: EM sums and the correlation of leave-one-out residuals (nadm_em_sums, nadm_resid_cor; not on the training path)
hipcc $FLAGS -c nadm_obs_project.hip -o nadm_obs_project.o "$@" # standardised PCA: the two observed-calls pair products on the matrix pipe (nadm_obs_project, nadm_obs_project_t; not on the training path)
# host-only units, compiled as plain C++ (no device pass)
hipcc $HOST -c nadm_gmm.cpp -o nadm_gmm.o "$@"                  # decoder-init mixture fit on the host
hipcc $HOST -c nadm_host_io.cpp -o nadm_host_io.o "$@"          # host packer, .bed converter, VCF parser, savetxt
hipcc $HOST -c nadm_layout.cpp -o nadm_layout.o "$@"            # head table + flat parameter layout
hipcc $HOST -c nadm_ld_sweep.cpp -o nadm_ld_sweep.o "$@"        # the greedy sweep of LD pruning
# the test hooks (nadm_test_force_slices / _p3_slices / _generic_mlp) are the one difference between the two libraries: nadm_hooks.cpp
# without the macro has no setter and getters that return 0; with it, the setters exist.  Every other object, the kernels included, is
# linked into both.  The tests that need a hook re-run themselves in a child process against the TEST build (tests/conftest.py: in_hook_build).
hipcc $HOST -c nadm_hooks.cpp -o nadm_hooks.o "$@"
hipcc $HOST -DNADM_TEST_HOOKS -c nadm_hooks.cpp -o nadm_hooks_th.o "$@"
OBJS="nadm_genotype_passes.o nadm_small_kernels.o nadm_step.o nadm_gmm.o nadm_gmm_dev.o nadm_calib.o nadm_project.o nadm_project_p.o nadm_kinship.o nadm_ld.o nadm_snp_hwe.o nadm_cv.o nadm_snp_info.o nadm_resid_cor.o nadm_obs_project.o nadm_host_io.o nadm_layout.o nadm_ld_sweep.o"
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libnadm.so -o libnadm.so $OBJS nadm_hooks.o -lpthread -ldl
echo "built $(pwd)/libnadm.so"
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-soname,libnadm.so -o libnadm_testhooks.so $OBJS nadm_hooks_th.o -lpthread -ldl
echo "built $(pwd)/libnadm_testhooks.so"
