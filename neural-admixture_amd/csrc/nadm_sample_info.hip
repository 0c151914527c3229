// Standard errors of Q given P: the per-SAMPLE Fisher information of a sample's row of ancestry fractions GIVEN the allele frequencies,
// in the binomial admixture model (include/nadm.h, nadm_sample_info).  The mirror image of nadm_snp_info.hip: one pass of
// N M K^2 / 2 work over the packed matrix with the K (K + 1) / 2 running sums per sample, not per SNP.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   sample_info_accum_kernel  the lane-per-sample walk of nadm_chunk_ranges.h (sample_walk: the packed words, the staged P rows, the
//                             barriers, code 3 for whatever adds nothing) with the T = KP (KP + 1) / 2 running sums of the upper
//                             triangle (fp32) and n (int32) in registers for the whole range.  Per genotype: KP multiply-adds for pi,
//                             two clips, one multiply and one reciprocal for the weight 1 / (r u), KP multiplies for w p_a, T
//                             multiply-adds; code 3 enters every sum as exactly +0.0f / 0.  Writes the range's slab plane by plane (a
//                             wave's stores are contiguous), n as plane T.
//   sample_info_fold_kernel   one thread per sample: adds the ranges' partials in range order in float64, applies the factor 2 of the
//                             binomial(2, pi) call once (exact) and writes the pairs a <= b < K of the REAL columns, a-major.
// The float64 inverse under the constraint sum_k q_k = 1 is the caller's (neural_admixture_amd/qse.py: nadm_snp_info_se on the
// drop-one form).  At KP = 16 the kernel holds 136 sums + 16 q + 16 p + 32 packed words: a 256-thread block is one wave per SIMD, which
// may use the whole register file, so nothing spills; the narrow heads run several blocks per compute unit.  The matrix-pipe
// formulation (weights on the VALU, W (p_a p_b) on MFMA with split operands) and heads wider than 16 are not built here.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int SI_MAX_KP = 16;
constexpr int SI_TILE = 256;              // samples per block: 4 waves, a lane per sample
constexpr int SI_MAX_CHUNKS = 1024;       // chunks per range at most: no fp32 running sum covers more than 2^18 SNPs (n exact: < 2^24)
constexpr int64_t SI_BLOCKS = 1024;       // blocks wanted at least (256 CUs x 4 blocks of 4 waves), while there are chunks to split
__host__ __device__ constexpr int si_pairs(int k) { return k * (k + 1) / 2; }

template <int KP>
__global__ __launch_bounds__(SI_TILE) void sample_info_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int tiles, const int64_t chunks_per_range, const int64_t chunks, float* __restrict__ part) {
    constexpr int T = si_pairs(KP);
    __shared__ __attribute__((aligned(16))) float Ps[RANGE_CHUNK * KP];      // the chunk's P rows (16 KB at KP = 16)
    const int t = threadIdx.x;
    const int range = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - range * tiles;       // tile fastest: neighbours share a chunk of P
    const RangeRow rr = range_row(xp, ld, idx, tile * SI_TILE + t, b);
    const bool wave_live = tile * SI_TILE + (t & ~63) < b;        // wave-uniform

    float q[KP];
    load_row<KP>(Q + (int64_t)rr.posc * q_stride, q);
    float acc[T];
#pragma unroll
    for (int i = 0; i < T; ++i) acc[i] = 0.f;
    int n = 0;

    sample_walk<KP, SI_TILE>(rr, wave_live, chunk_range(range, chunks_per_range, chunks), ld, M, P, Ps, [&](const uint32_t code, const int s) {
        const uint32_t m = obs_mask(code);
        float p[KP];
        const float pi = dot_row<KP>(q, Ps + s * KP, p);
        // 1 - pi from the UNCLIPPED product, as em_terms (nadm_common.h)
        const float r = fminf(fmaxf(pi, eps), one_m_eps);
        const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
        // the expected information of pi in one call is 2 / (r u); the 2 is the fold's.  Masked: exactly +0.0f
        const float wt = keepf(__builtin_amdgcn_rcpf(r * u), m);
        n += (int)(m & 1u);
        int i = 0;
#pragma unroll
        for (int a = 0; a < KP; ++a) {
            const float wp = wt * p[a];
#pragma unroll
            for (int d = a; d < KP; ++d, ++i) acc[i] = fmaf(wp, p[d], acc[i]);
        }
    });
    // the block's slab [T + 1][256]: every lane writes (a lane past the list wrote zeros; the fold never reads it)
    float* out = part + ((int64_t)range * tiles + tile) * ((T + 1) * SI_TILE) + t;
#pragma unroll
    for (int i = 0; i < T; ++i) out[i * SI_TILE] = acc[i];
    out[T * SI_TILE] = __int_as_float(n);
}

// One thread per sample s < b: the ranges' partials in range order in float64, times 2; the pairs a <= d < k of the real columns, a-major
__global__ __launch_bounds__(256) void sample_info_fold_kernel(const float* __restrict__ part, const int ranges, const int tiles, const int b,
                                                               const int k, const int kp, double* __restrict__ info,
                                                               int32_t* __restrict__ nobs) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= b) return;
    const int T = si_pairs(kp);
    const int64_t slab = (int64_t)(T + 1) * SI_TILE, per_range = (int64_t)tiles * slab;
    const float* base = part + (s / SI_TILE) * slab + (s % SI_TILE);
    double* out = info + s * si_pairs(k);
    int i_out = 0;
    for (int a = 0; a < k; ++a) {
        const int i_row = a * kp - a * (a - 1) / 2 - a;         // plane of (a, d) = i_row + d
        for (int d = a; d < k; ++d, ++i_out) {
            const float* src = base + (int64_t)(i_row + d) * SI_TILE;
            double sum = 0.0;
            for (int r = 0; r < ranges; ++r) sum += (double)src[r * per_range];
            out[i_out] = 2.0 * sum;
        }
    }
    const float* src = base + (int64_t)T * SI_TILE;
    int n = 0;
    for (int r = 0; r < ranges; ++r) n += __float_as_int(src[r * per_range]);
    nobs[s] = n;
}

static bool si_shape_ok(int b, int64_t M) { return b > 0 && M > 0; }
static bool si_kp_ok(int kp) { return kp >= 4 && kp <= SI_MAX_KP && kp % 4 == 0; }
// the launch shape, a rule of (b, M) alone
static RangePlan si_plan(int b, int64_t M) { return range_plan(M, range_tiles(b, SI_TILE), SI_BLOCKS, SI_MAX_CHUNKS); }

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_sample_info_ranges(int32_t b, int64_t M) { return si_shape_ok(b, M) ? range_count(si_plan(b, M).ranges) : 0; }

// scratch: the partials [ranges][tiles][T + 1][256] (T fp32 sums and n as int32); 0 for a width without a kernel
extern "C" int64_t nadm_sample_info_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    return si_shape_ok(b, M) && si_kp_ok(kp) ? si_plan(b, M).blocks_bound * ((si_pairs(kp) + 1) * SI_TILE) : 0;
}

extern "C" int nadm_sample_info(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k,
                                int32_t kp, const float* Q, int32_t q_stride, float eps, double* info, int32_t* nobs, float* scratch,
                                void* stream) {
    const char* who = "nadm_sample_info";
    if (!xp || !P || !Q || !info || !nobs || !scratch) return failf(who, "null pointer");
    if (b <= 0 || M <= 0) return failf(who, "empty batch (need b > 0 and M > 0)");
    if (check_packed(who, ld, M) || check_head(who, k, kp, q_stride) || check_eps(who, eps)) return 1;
    if (kp > SI_MAX_KP) return failf(who, "K must be <= 16 (the K (K + 1) / 2 running sums of a sample live in one thread's registers)");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)Q | (uintptr_t)scratch) & 15) != 0)
        return failf(who, "xp, P, Q and scratch must be 16-byte aligned");
    if (((uintptr_t)info & 7) != 0 || (((uintptr_t)nobs | (uintptr_t)idx) & 3) != 0)
        return failf(who, "info must be 8-byte and nobs, idx 4-byte aligned");
    const RangePlan pl = si_plan(b, M);
    if (range_launch_check(who, pl)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - eps;
    if (int e = dispatch_kp(who, kp, [&](auto KP) {
            if constexpr (decltype(KP)::value <= SI_MAX_KP)
                hipLaunchKernelGGL((sample_info_accum_kernel<decltype(KP)::value>), range_grid(pl), dim3(SI_TILE), 0, st, xp, ld, idx, b, M, P,
                                   Q, q_stride, eps, ome, (int)pl.tiles, pl.cpr, pl.chunks, scratch);
        }))
        return e;
    if (int e = check_launch("sample_info (accumulate)")) return e;
    hipLaunchKernelGGL(sample_info_fold_kernel, fold_grid(b), dim3(256), 0, st, scratch, (int)pl.ranges, (int)pl.tiles, b, k, kp, info, nobs);
    return check_launch("sample_info (fold)");
}
