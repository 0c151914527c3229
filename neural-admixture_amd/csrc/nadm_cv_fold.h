// The cross-validation fold of a genotype call (include/nadm.h, "fold of a call"): a fixed function of (seed, matrix row, SNP),
// implemented once for both kernels of nadm_cv.hip.  The row key is uniform over a block (nadm_cv_mask) or a wave
// (nadm_cv_deviance: every thread works on the same sample), so it sits on the scalar unit; per call a kernel pays one cv_mix32
// and one multiply-high.
#pragma once
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

__host__ __device__ __forceinline__ uint32_t cv_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// i: the row's index in the WHOLE matrix (row0 + the row within the call), < 2^31
__host__ __device__ __forceinline__ uint32_t cv_row_key(const uint64_t seed, const uint32_t i) {
    return cv_mix32(cv_mix32(i ^ (uint32_t)(seed >> 32)) + (uint32_t)seed + 0x9E3779B9u);
}

// fold of SNP j of the row with key `key`, in 0 .. folds - 1
__host__ __device__ __forceinline__ uint32_t cv_fold(const uint32_t key, const uint32_t j, const uint32_t folds) {
    return (uint32_t)(((uint64_t)cv_mix32(key ^ j) * folds) >> 32);
}

// cv_fold(key, j, folds) == fold ? ~0 : 0, as arithmetic (nadm_common.h: no select on a lane condition); fold < folds <= 64
__device__ __forceinline__ uint32_t cv_held_mask(const uint32_t key, const uint32_t j, const uint32_t folds, const uint32_t fold) {
    uint32_t m = (uint32_t)((int)((cv_fold(key, j, folds) ^ fold) - 1u) >> 31);
    asm("" : "+v"(m));
    return m;
}

// the refusals both entries share: the fold function is defined for rows and SNPs below 2^31 and 2..64 folds
inline int check_cv_fold(const char* who, int64_t row0, int64_t rows, int64_t M, int32_t folds, int32_t fold) {
    if (row0 < 0 || row0 + rows > (1ll << 31)) return failf(who, "need row0 >= 0 and row0 + rows <= 2^31");
    if (M > (1ll << 31)) return failf(who, "M must be <= 2^31");
    if (folds < 2 || folds > NADM_CV_MAX_FOLDS) return failf(who, "folds must be in 2..NADM_CV_MAX_FOLDS");
    if (fold < 0 || fold >= folds) return failf(who, "fold must be in 0..folds-1");
    return 0;
}

}  // namespace nadm
