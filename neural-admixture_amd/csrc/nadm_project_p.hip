// The P half of the block EM over observed calls: refit one head's P against a FIXED Q with a masked EM step of the binomial admixture
// model (include/nadm.h, nadm_project_p).  The transpose of nadm_project.hip: there a lane owns a sample and P is broadcast from LDS,
// here a thread owns a SNP and Q is broadcast from LDS.
//
// Two launches per step, no floating-point atomics (two launches on the same inputs give the same bits):
//   project_p_accum_kernel  the SNP-owner sweep of nadm_snp_sweep.h: a thread's p, B and C rows live in registers.  Missing calls (code
//                           3), rows >= b and SNPs >= M enter every sum as exactly +0.0f.  Writes the slice's partials of B, C (fp32)
//                           and n (int32).  The body is em_sums_accumulate (nadm_em_accum.h), shared with nadm_em_sums.
//   project_p_fold_kernel   one thread per (SNP, column): adds the slices' partials in slice order in float64 and applies
//                           p' = clip(pB / (pB + (1 - p)C), pmin, 1 - pmin); den == 0 returns p as it came.
#include "nadm_em_accum.h"

namespace nadm {

template <int KP>
__global__ __launch_bounds__(SWEEP_CHUNK) void project_p_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ bcpart, int32_t* __restrict__ npart) {
    em_sums_accumulate<KP>(xp, ld, idx, b, M, P, Q, q_stride, eps, one_m_eps, slices, tiles_per_slice, Mp, bcpart, npart);
}

// One thread per (SNP j < M, column c < kp): the slices' partials in slice order, in float64; rows >= M of Pout are never written.
__global__ __launch_bounds__(256) void project_p_fold_kernel(const float* __restrict__ bcpart, const int32_t* __restrict__ npart,
                                                             const int slices, const int64_t Mp, const int64_t M, const int k, const int kp,
                                                             const float* Pin, float* Pout,   /* may alias */
                                                             const float pmin, int32_t* __restrict__ nobs_snp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * kp) return;
    const int64_t j = e / kp;
    const int c = (int)(e - j * kp);
    double Bs = 0.0, Cs = 0.0;
    for (int s = 0; s < slices; ++s) {
        const float* row = bcpart + ((int64_t)s * Mp + j) * (2 * kp);
        Bs += (double)row[c];
        Cs += (double)row[kp + c];
    }
    const float pi = Pin[e];
    float out = 0.f;                                             // pad columns are written 0
    if (c < k) {
        const double num = (double)pi * Bs;
        const double den = num + (1.0 - (double)pi) * Cs;
        out = pi;                                                // den == 0 (nobody observes the SNP): the bits as they came
        if (den > 0.0) {
            double v = num / den;
            const double lo = (double)pmin, hi = 1.0 - (double)pmin;
            v = v < lo ? lo : (v > hi ? hi : v);
            out = (float)v;
        }
    }
    Pout[e] = out;
    if (nobs_snp && c == 0) {
        int n = 0;
        for (int s = 0; s < slices; ++s) n += npart[(int64_t)s * Mp + j];
        nobs_snp[j] = n;
    }
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_project_p_slices(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_slices(b, M); }

// scratch: B | C partials [slices, Mp, 2 kp] float | n partials [slices, Mp] int32, Mp = 256 chunks
extern "C" int64_t nadm_project_p_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    return (b <= 0 || M <= 0 || kp <= 0 || kp > NADM_MAX_K) ? 0 : sweep_rows_bound(b, M) * (2 * (int64_t)kp + 1);
}

extern "C" int nadm_project_p(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                              int32_t k, int32_t kp, const float* Pin, float* Pout, float eps, float pmin, int32_t* nobs_snp,
                              float* scratch, void* stream) {
    if (!xp || !Q || !Pin || !Pout || !scratch) return fail("nadm_project_p: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_project_p: empty batch (need b > 0 and M > 0)");
    if (check_packed("nadm_project_p", ld, M) || check_head("nadm_project_p", k, kp, q_stride) || check_eps("nadm_project_p", eps)) return 1;
    if (!(pmin >= 0.f && pmin < 0.5f)) return fail("nadm_project_p: pmin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)Pin | (uintptr_t)Pout | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_project_p: xp, Q, Pin, Pout and scratch must be 16-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll || (M * kp + 255) / 256 > 0x7FFFFFFFll)
        return fail("nadm_project_p: too many blocks for one launch");
    float* bcpart = scratch;
    int32_t* npart = reinterpret_cast<int32_t*>(scratch + (int64_t)slices * Mp * 2 * kp);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps;
    if (int e = dispatch_kp("nadm_project_p", kp, [&](auto KP) {
            hipLaunchKernelGGL((project_p_accum_kernel<decltype(KP)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld, idx, b, M, Pin, Q,
                               q_stride, eps, ome, slices, tps, Mp, bcpart, npart);
        }))
        return e;
    if (int e = check_launch("project_p (accumulate)")) return e;
    hipLaunchKernelGGL(project_p_fold_kernel, dim3((unsigned)((M * kp + 255) / 256)), dim3(256), 0, st, bcpart, npart, slices, Mp, M, k, kp,
                       Pin, Pout, pmin, nobs_snp);
    return check_launch("project_p (fold)");
}
