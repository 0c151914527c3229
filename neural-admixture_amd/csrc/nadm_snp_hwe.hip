// Hardy-Weinberg proportions GIVEN ANCESTRY: the per-SNP score test of an inbreeding coefficient F at F = 0 in the binomial admixture
// model (include/nadm.h, nadm_snp_hwe).  One pass of N M K work over the packed matrix.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   snp_hwe_accum_kernel  the SNP-owner sweep of nadm_snp_sweep.h: a thread's p row and four running sums (U and Hexp in fp32, n and
//                         Hobs in int32) live in registers.  Per genotype: KP multiply-adds, one reciprocal.  Missing calls (code 3),
//                         rows >= b, SNPs >= M and a masked pi enter every sum as exactly +0.0f / 0.  Writes the slice's partials, 16
//                         bytes per SNP.
//   snp_hwe_fold_kernel   one thread per SNP: adds the slices' partials in slice order, U and Hexp in float64, n and Hobs as integers.
#include "nadm_snp_sweep.h"

namespace nadm {

template <int KP>
__global__ __launch_bounds__(SWEEP_CHUNK) void snp_hwe_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const float pimin, const float one_m_pimin, const int slices, const int tiles_per_slice, const int64_t Mp,
    u32x4_t* __restrict__ part) {
    const SweepPos pos = sweep_pos(slices);
    float p[KP];
    sweep_load_p<KP>(P, pos.j, M, p);
    float U = 0.f, H = 0.f;
    int n = 0, hobs = 0;

    snp_sweep<KP>(pos, xp, ld, idx, b, M, Q, q_stride, tiles_per_slice, [&](const uint32_t code, const float* qr) {
        // observed, g == 0 ? ~0 : 0 and g == 1 ? ~0 : 0 as arithmetic on the code, applied with v_and / v_bfi (nadm_common.h: no
        // select on a lane condition)
        uint32_t m = obs_mask(code);
        uint32_t m0 = (uint32_t)((int)(code - 1u) >> 31);
        uint32_t m1 = (uint32_t)((int)((code ^ 1u) - 1u) >> 31);
        asm("" : "+v"(m0));
        asm("" : "+v"(m1));
        float pi = 0.f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {                       // a broadcast; wide heads take the row the same way, four columns at a time
            const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
            pi = fmaf(t4.x, p[k], pi); pi = fmaf(t4.y, p[k + 1], pi);
            pi = fmaf(t4.z, p[k + 2], pi); pi = fmaf(t4.w, p[k + 3], pi);
        }
        m &= ge0_mask(pi - pimin) & ge0_mask(one_m_pimin - pi);
        // 1 - pi from the UNCLIPPED product, as em_terms (nadm_common.h)
        const float r = fminf(fmaxf(pi, eps), one_m_eps);
        const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
        // g = 0: r / u, g = 2: u / r, g = 1: -1
        const float num = __uint_as_float(blend(__float_as_uint(r), __float_as_uint(u), m0));
        const float den = __uint_as_float(blend(__float_as_uint(u), __float_as_uint(r), m0));
        const float ratio = num * __builtin_amdgcn_rcpf(den);
        const float tt = __uint_as_float(blend(0xBF800000u, __float_as_uint(ratio), m1));
        U += keepf(tt, m);                                      // masked: exactly +0.0f
        H += keepf((pi + pi) * (1.f - pi), m);
        n += (int)(m & 1u);
        hobs += (int)(m & m1 & 1u);
    });

    part[(int64_t)pos.slice * Mp + pos.j] = (u32x4_t){__float_as_uint(U), __float_as_uint(H), (uint32_t)n, (uint32_t)hobs};
}

// One thread per SNP j < M: the slices' partials in slice order, U and Hexp in float64, n and Hobs as integers
__global__ __launch_bounds__(256) void snp_hwe_fold_kernel(const u32x4_t* __restrict__ part, const int slices, const int64_t Mp,
                                                           const int64_t M, double* __restrict__ U, double* __restrict__ Hexp,
                                                           int32_t* __restrict__ nobs, int32_t* __restrict__ Hobs) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double us = 0.0, hs = 0.0;
    int n = 0, ho = 0;
    for (int s = 0; s < slices; ++s) {
        const u32x4_t v = part[(int64_t)s * Mp + j];
        us += (double)__uint_as_float(v[0]);
        hs += (double)__uint_as_float(v[1]);
        n += (int)v[2];
        ho += (int)v[3];
    }
    U[j] = us;
    nobs[j] = n;
    if (Hexp) Hexp[j] = hs;
    if (Hobs) Hobs[j] = ho;
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_snp_hwe_slices(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_slices(b, M); }

// scratch: the partials [slices, Mp] x { U, Hexp (fp32), n, Hobs (int32) }, Mp = 256 chunks
extern "C" int64_t nadm_snp_hwe_scratch_floats(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_rows_bound(b, M) * 4; }

extern "C" int nadm_snp_hwe(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                            int32_t k, int32_t kp, const float* P, float eps, float pimin, double* U, double* Hexp, int32_t* nobs,
                            int32_t* Hobs, float* scratch, void* stream) {
    if (!xp || !Q || !P || !U || !nobs || !scratch) return fail("nadm_snp_hwe: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_snp_hwe: empty block (need b > 0 and M > 0)");
    if (check_packed("nadm_snp_hwe", ld, M) || check_head("nadm_snp_hwe", k, kp, q_stride) || check_eps("nadm_snp_hwe", eps)) return 1;
    if (!(pimin >= 0.f && pimin < 0.5f)) return fail("nadm_snp_hwe: pimin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)P | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_snp_hwe: xp, Q, P and scratch must be 16-byte aligned");
    if ((((uintptr_t)U | (uintptr_t)Hexp) & 7) != 0 || (((uintptr_t)nobs | (uintptr_t)Hobs | (uintptr_t)idx) & 3) != 0)
        return fail("nadm_snp_hwe: U, Hexp must be 8-byte and nobs, Hobs, idx 4-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll) return fail("nadm_snp_hwe: too many blocks for one launch");
    u32x4_t* part = reinterpret_cast<u32x4_t*>(scratch);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps, omp = 1.f - pimin;
    if (int e = dispatch_kp("nadm_snp_hwe", kp, [&](auto KP) {
            hipLaunchKernelGGL((snp_hwe_accum_kernel<decltype(KP)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld, idx, b, M, P, Q,
                               q_stride, eps, ome, pimin, omp, slices, tps, Mp, part);
        }))
        return e;
    if (int e = check_launch("snp_hwe (accumulate)")) return e;
    hipLaunchKernelGGL(snp_hwe_fold_kernel, dim3((unsigned)chunks), dim3(256), 0, st, part, slices, Mp, M, U, Hexp, nobs, Hobs);
    return check_launch("snp_hwe (fold)");
}
