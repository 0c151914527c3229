// Standard errors of P: the per-SNP Fisher information of a SNP's frequency row GIVEN the ancestry fractions, in the binomial admixture
// model (include/nadm.h, nadm_snp_info).  One pass of N M K^2 / 2 work over the packed matrix.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   snp_info_accum_kernel  the SNP-owner sweep of nadm_snp_sweep.h: a thread's p row, the T = KP (KP + 1) / 2 running sums of the upper
//                          triangle (fp32) and n (int32) live in registers.  Per genotype: the Q row once from LDS into registers, KP
//                          multiply-adds for pi, two clips, one multiply and one reciprocal for the weight 1 / (r u), KP multiplies
//                          for w q_a, T multiply-adds.  Missing calls (code 3), rows >= b and SNPs >= M enter every sum as exactly
//                          +0.0f / 0.  Writes the slice's partials plane by plane (a wave's stores are contiguous), n as plane T.
//   snp_info_fold_kernel   one thread per SNP: adds the slices' partials in slice order in float64, applies the factor 2 of the
//                          binomial(2, pi) call once (exact) and writes the pairs a <= b < K of the REAL columns, a-major.
// and, as an entry of its own (nadm_snp_info_se), the float64 inverse of every SNP's free block:
//   snp_info_se_kernel     one thread per SNP: Cholesky in registers and one forward substitution per column.  torch's batched
//                          cholesky_ex / cholesky_inverse was tried first and is NOT usable on the ROCm build: over batches of 65536
//                          blocks it returned error flags for positive definite 8 x 8 blocks and wrong inverses for 7 x 7 ones.
//
// The sums are a GEMM of the pairwise products q_a q_b against the weights W, but W needs Q P^T first: that is pass 2's structure
// (nadm_genotype_passes.hip).  A matrix-pipe formulation and heads wider than 16 are not built here: at KP = 16 the 136 running sums
// still fit one thread's registers without a spill, at KP = 24 the 300 do not.
#include "nadm_snp_sweep.h"

namespace nadm {

constexpr int INFO_MAX_KP = 16;
__host__ __device__ constexpr int info_pairs(int k) { return k * (k + 1) / 2; }

template <int KP>
__global__ __launch_bounds__(SWEEP_CHUNK) void snp_info_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ part) {
    constexpr int T = info_pairs(KP);
    const SweepPos pos = sweep_pos(slices);
    float p[KP];
    sweep_load_p<KP>(P, pos.j, M, p);
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.f;
    int n = 0;

    snp_sweep<KP>(pos, xp, ld, idx, b, M, Q, q_stride, tiles_per_slice, [&](const uint32_t code, const float* qr) {
        const uint32_t m = obs_mask(code);
        float q[KP];
        float pi = 0.f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {                       // a broadcast: the row is read once, four columns at a time
            const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
            q[k] = t4.x; q[k + 1] = t4.y; q[k + 2] = t4.z; q[k + 3] = t4.w;
            pi = fmaf(t4.x, p[k], pi); pi = fmaf(t4.y, p[k + 1], pi);
            pi = fmaf(t4.z, p[k + 2], pi); pi = fmaf(t4.w, p[k + 3], pi);
        }
        // 1 - pi from the UNCLIPPED product, as em_terms (nadm_common.h).  A NaN pi (P at a SNP nobody observes) clips to eps: finite
        const float r = fminf(fmaxf(pi, eps), one_m_eps);
        const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
        // the expected information of pi in one call is 2 / (r u); the 2 is the fold's.  Masked: exactly +0.0f
        const float w = keepf(__builtin_amdgcn_rcpf(r * u), m);
        n += (int)(m & 1u);
        int t = 0;
#pragma unroll
        for (int a = 0; a < KP; ++a) {
            const float wq = w * q[a];
#pragma unroll
            for (int c = a; c < KP; ++c, ++t) acc[t] = fmaf(wq, q[c], acc[t]);
        }
    });

    float* out = part + (int64_t)pos.slice * (T + 1) * Mp + pos.j;
#pragma unroll
    for (int t = 0; t < T; ++t) out[(int64_t)t * Mp] = acc[t];
    out[(int64_t)T * Mp] = __int_as_float(n);
}

// One thread per SNP j < M: the slices' partials in slice order in float64, times 2; the pairs a <= c < k of the real columns, a-major
__global__ __launch_bounds__(256) void snp_info_fold_kernel(const float* __restrict__ part, const int slices, const int64_t Mp,
                                                            const int64_t M, const int k, const int kp, double* __restrict__ info,
                                                            int32_t* __restrict__ nobs) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int T = info_pairs(kp);
    const int64_t plane = (int64_t)(T + 1) * Mp;
    double* out = info + j * info_pairs(k);
    int t_out = 0;
    for (int a = 0; a < k; ++a) {
        const int t_row = a * kp - a * (a - 1) / 2 - a;         // plane of (a, c) = t_row + c
        for (int c = a; c < k; ++c, ++t_out) {
            const float* src = part + (int64_t)(t_row + c) * Mp + j;
            double s = 0.0;
            for (int sl = 0; sl < slices; ++sl) s += (double)src[sl * plane];
            out[t_out] = 2.0 * s;
        }
    }
    const float* src = part + (int64_t)T * Mp + j;
    int n = 0;
    for (int sl = 0; sl < slices; ++sl) n += __float_as_int(src[sl * plane]);
    nobs[j] = n;
}

// The float64 inverse, one thread per SNP j < M: the SNP's block with the rows and columns of the dropped components (drop[j][a] != 0,
// and the pad columns a >= k) replaced by those of the identity, factored as L L^T in registers (every index is a compile-time
// constant); (A^-1)_cc = |L^-1 e_c|^2 by one forward substitution per column.  A pivot that is not > 0 (a NaN included) or n = 0 makes
// every entry of the SNP NaN, as LAPACK's potrf would refuse the block.
template <int KP>
__global__ __launch_bounds__(64) void snp_info_se_kernel(const double* __restrict__ info, const uint8_t* __restrict__ drop,
                                                         const int32_t* __restrict__ nobs, const int64_t M, const int k,
                                                         double* __restrict__ se) {
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= M) return;
    constexpr int T = info_pairs(KP);
    const double* src = info + j * info_pairs(k);
    bool fr[KP];
#pragma unroll
    for (int a = 0; a < KP; ++a) fr[a] = a < k && drop[j * k + (a < k ? a : 0)] == 0;
    double L[T];                                                // the lower triangle by rows: (i, c), c <= i, at i (i + 1) / 2 + c
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int c = 0; c <= i; ++c) {
            double v = i == c ? 1.0 : 0.0;
            if (fr[i] && fr[c]) v = src[c * k - c * (c - 1) / 2 + (i - c)];        // the pair (c, i), c <= i, of the a-major real columns
            L[i * (i + 1) / 2 + c] = v;
        }
    bool bad = nobs[j] == 0;
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int c = 0; c <= i; ++c) {
            double s = L[i * (i + 1) / 2 + c];
#pragma unroll
            for (int m = 0; m < c; ++m) s = fma(-L[i * (i + 1) / 2 + m], L[c * (c + 1) / 2 + m], s);
            if (c == i) {
                bad = bad || !(s > 0.0);
                L[i * (i + 1) / 2 + i] = sqrt(s);
            } else {
                L[i * (i + 1) / 2 + c] = s / L[c * (c + 1) / 2 + c];
            }
        }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        double y[KP];
        y[c] = 1.0 / L[c * (c + 1) / 2 + c];
        double var = y[c] * y[c];
#pragma unroll
        for (int i = c + 1; i < KP; ++i) {
            double s = 0.0;
#pragma unroll
            for (int m = c; m < i; ++m) s = fma(L[i * (i + 1) / 2 + m], y[m], s);
            y[i] = -s / L[i * (i + 1) / 2 + i];
            var = fma(y[i], y[i], var);
        }
        if (c < k) se[j * k + c] = (fr[c] && !bad && var > 0.0) ? sqrt(var) : nan;
    }
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_snp_info_slices(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_slices(b, M); }

// scratch: the partials [slices, T + 1, Mp] (T fp32 sums and n as int32), Mp = 256 chunks; 0 for a width without a kernel
extern "C" int64_t nadm_snp_info_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    if (b <= 0 || M <= 0 || kp < 4 || kp > INFO_MAX_KP || kp % 4 != 0) return 0;
    return sweep_rows_bound(b, M) * (info_pairs(kp) + 1);
}

extern "C" int nadm_snp_info(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                             int32_t k, int32_t kp, const float* P, float eps, double* info, int32_t* nobs, float* scratch,
                             void* stream) {
    if (!xp || !Q || !P || !info || !nobs || !scratch) return fail("nadm_snp_info: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_snp_info: empty block (need b > 0 and M > 0)");
    if (check_packed("nadm_snp_info", ld, M) || check_head("nadm_snp_info", k, kp, q_stride) || check_eps("nadm_snp_info", eps)) return 1;
    if (kp > INFO_MAX_KP) return fail("nadm_snp_info: K must be <= 16 (the K (K + 1) / 2 running sums of a SNP live in one thread's registers)");
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)P | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_snp_info: xp, Q, P and scratch must be 16-byte aligned");
    if (((uintptr_t)info & 7) != 0 || (((uintptr_t)nobs | (uintptr_t)idx) & 3) != 0)
        return fail("nadm_snp_info: info must be 8-byte and nobs, idx 4-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll) return fail("nadm_snp_info: too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps;
    if (int e = dispatch_kp("nadm_snp_info", kp, [&](auto KP) {
            if constexpr (decltype(KP)::value <= INFO_MAX_KP)
                hipLaunchKernelGGL((snp_info_accum_kernel<decltype(KP)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld, idx, b, M, P,
                                   Q, q_stride, eps, ome, slices, tps, Mp, scratch);
        }))
        return e;
    if (int e = check_launch("snp_info (accumulate)")) return e;
    hipLaunchKernelGGL(snp_info_fold_kernel, dim3((unsigned)chunks), dim3(256), 0, st, scratch, slices, Mp, M, k, kp, info, nobs);
    return check_launch("snp_info (fold)");
}

extern "C" int nadm_snp_info_se(const double* info, const uint8_t* drop, const int32_t* nobs, int64_t M, int32_t k, double* se,
                                void* stream) {
    if (!info || !drop || !nobs || !se) return fail("nadm_snp_info_se: null pointer");
    if (M <= 0) return fail("nadm_snp_info_se: empty block (need M > 0)");
    if (k < 1 || k > INFO_MAX_KP) return fail("nadm_snp_info_se: K must be in 1..16");
    if ((((uintptr_t)info | (uintptr_t)se) & 7) != 0 || ((uintptr_t)nobs & 3) != 0)
        return fail("nadm_snp_info_se: info and se must be 8-byte and nobs 4-byte aligned");
    const int64_t blocks = (M + 63) / 64;
    if (blocks > 0x7FFFFFFFll) return fail("nadm_snp_info_se: too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (int e = dispatch_kp("nadm_snp_info_se", nadm_pad_k(k), [&](auto KP) {
            if constexpr (decltype(KP)::value <= INFO_MAX_KP)
                hipLaunchKernelGGL((snp_info_se_kernel<decltype(KP)::value>), dim3((unsigned)blocks), dim3(64), 0, st, info, drop, nobs, M, k,
                                   se);
        }))
        return e;
    return check_launch("snp_info_se");
}
