// Host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include "nadm_err.h"

namespace nadm {

inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(err_buf(), 512, "%s: launch failed: %s", what, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

// step-dependent scalars of the Adam update (bias corrections folded in): step_size = lr / (1 - b1^t), inv_bc2 = 1 / sqrt(1 - b2^t)
inline void adam_scalars(float lr, int step, float* step_size, float* inv_bc2) {
    const double bc1 = 1.0 - pow(0.9, (double)step);
    const double bc2 = 1.0 - pow(0.95, (double)step);
    *step_size = (float)((double)lr / bc1);
    *inv_bc2 = (float)(1.0 / sqrt(bc2));
}

// The test hooks (nadm_hooks.cpp): 0 = the library's own rule.  In libnadm.so they always return 0; in libnadm_testhooks.so they return
// what nadm_test_force_slices / nadm_test_force_p3_slices / nadm_test_force_generic_mlp last set.
int hook_p2_slices();
int hook_p3_slices();
int hook_generic_mlp();

// the partial sums only (the first kernel of nadm_mlp_bwd_weights): used by the variants of pass 3 that cannot host them
int mlp_bwd_weight_parts(const nadm_heads_t* hd, int32_t b, const float* Zn, const float* H, const float* dL, const float* dHpre,
                         const float* dgp, float* small_part, void* stream);

// The genotype passes as the plan's step runs them, with its matmul precision (NADM_PRECISION_*, nadm_plan_set_precision):
// "highest" calls exactly the public entry point of that form (nadm_decode_bce_sliced / _images / _step, nadm_encode_fwd / _part /
// _small); "medium" runs the same checks and launches the kernels' medium instantiations (nadm_genotype_passes.hip).
int decode_bce_prec(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, float* P, int32_t kp, const float* Q, int32_t SP,
                    float* dP, float* dqpart, float* losspart, int32_t with_loss, uint8_t* xg, const nadm_adam_t* adam, const void* qimg,
                    int32_t n_slices, float* slab, int32_t* counters, int32_t precision, void* stream);
// small_part == NULL: no side work (then total_chunks > 0 is the launch of one part of a pass, nadm_encode_fwd_part)
int encode_fwd_prec(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* V, int32_t CP, float* zpart,
                    int64_t total_chunks, const float* small_part, int32_t splits, int32_t n_small, float* grad_small, float* small,
                    const nadm_adam_t* adam, int32_t precision, void* stream);

}  // namespace nadm
