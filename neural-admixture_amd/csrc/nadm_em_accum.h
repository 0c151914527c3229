// The accumulation of the EM sums B and C of one head's P against a fixed Q (include/nadm.h, nadm_project_p and nadm_em_sums), shared by
// the two units that form them: nadm_project_p.hip folds them into the refitted P, nadm_resid_cor.hip keeps them.  One body, hence the
// same operations in the same order and the same bits in both.
//
// The SNP-owner sweep of nadm_snp_sweep.h: a thread's p, B and C rows live in registers.  Missing calls (code 3), rows >= b and SNPs >= M
// enter every sum as exactly +0.0f.  Writes the slice's partials of B, C (fp32, row slice * Mp + j of bcpart, 2 KP floats) and n (int32).
#pragma once
#include "nadm_snp_sweep.h"

namespace nadm {

template <int KP>
__device__ __forceinline__ void em_sums_accumulate(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ bcpart, int32_t* __restrict__ npart) {
    const SweepPos pos = sweep_pos(slices);
    float p[KP], B[KP], Cc[KP];
    sweep_load_p<KP>(P, pos.j, M, p);
#pragma unroll
    for (int k = 0; k < KP; ++k) B[k] = Cc[k] = 0.f;
    int n = 0;

    snp_sweep<KP>(pos, xp, ld, idx, b, M, Q, q_stride, tiles_per_slice, [&](const uint32_t code, const float* qr) {
        const uint32_t m = obs_mask(code);
        float rr = 0.f;
        float q[KP <= 16 ? KP : 4];
        if constexpr (KP <= 16) {
#pragma unroll
            for (int k = 0; k < KP; k += 4) {
                const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                q[k] = t4.x; q[k + 1] = t4.y; q[k + 2] = t4.z; q[k + 3] = t4.w;
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) rr = fmaf(q[k], p[k], rr);
        } else {                                                // wide heads: the row is read twice, four columns at a time
#pragma unroll
            for (int k = 0; k < KP; k += 4) {
                const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                rr = fmaf(t4.x, p[k], rr); rr = fmaf(t4.y, p[k + 1], rr);
                rr = fmaf(t4.z, p[k + 2], rr); rr = fmaf(t4.w, p[k + 3], rr);
            }
        }
        const EmTerms e = em_terms(rr, code, m, eps, one_m_eps);
        if constexpr (KP <= 16) {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                B[k] = fmaf(q[k], e.t1, B[k]);
                Cc[k] = fmaf(q[k], e.t0, Cc[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < KP; k += 4) {
                const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                q[0] = t4.x; q[1] = t4.y; q[2] = t4.z; q[3] = t4.w;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    B[k + c] = fmaf(q[c], e.t1, B[k + c]);
                    Cc[k + c] = fmaf(q[c], e.t0, Cc[k + c]);
                }
            }
        }
        n += (int)(m & 1u);
    });

    const int64_t o = (int64_t)pos.slice * Mp + pos.j;
    float* out = bcpart + o * (2 * KP);
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        *reinterpret_cast<float4*>(out + k) = make_float4(B[k], B[k + 1], B[k + 2], B[k + 3]);
        *reinterpret_cast<float4*>(out + KP + k) = make_float4(Cc[k], Cc[k + 1], Cc[k + 2], Cc[k + 3]);
    }
    npart[o] = n;
}

}  // namespace nadm
