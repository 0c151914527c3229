// Model-fit check: the pairwise correlation of leave-one-out residuals (evalAdmix, Garcia-Erill & Albrechtsen 2020) of one block of
// ordered sample pairs, and the EM sums it is taken against (include/nadm.h, nadm_em_sums and nadm_resid_cor).
//
// nadm_em_sums: two launches, no floating-point atomics:
//   em_sums_accum_kernel    em_sums_accumulate (nadm_em_accum.h): the body nadm_project_p's accumulation runs, hence its bits.
//   em_sums_fold_kernel     one thread per (SNP, column): the slices' partials in slice order in float64, rounded to fp32 once.
//
// nadm_resid_cor: two launches, no floating-point atomics (two calls on the same inputs give the same bits):
//   resid_cor_accum_kernel  one 256-thread block per (256 samples a, group of GB left-out samples b, contiguous range of 256-SNP
//                           chunks).  A lane owns a sample a: its q row, its 64 bytes of the chunk (four 16-byte loads, decoded in
//                           registers) and four fp32 running sums per b of the group (S, Ta, Tb, n) live in registers across the
//                           whole range, so the partials are written once.  Per chunk the block first builds, cooperatively, what
//                           depends on (b, j) alone: thread t takes SNP t of the chunk, reads its rows of P, B and C once and, for
//                           every b of the group, forms the refitted frequencies f^{-b}_j. (KP divisions, amortised over the 256
//                           samples a), pi^{-b}_bj, d_bj and o_bj into LDS.  Then every lane walks the chunk's SNPs: the f row and
//                           (d_b, o_b) are read from LDS at the same address in every lane (a broadcast); per (a, b, j) that is KP
//                           multiply-adds for pi^{-b}_aj and seven more operations.  a's word is decoded once per SNP for the
//                           whole group.  Missing calls (code 3) and SNPs >= M enter every sum as exactly +0.0f.
//   resid_cor_fold_kernel   one thread per pair: the ranges' partials in range order in float64; n is a sum of ones below 2^24 per
//                           range (a range never covers more than 2^18 SNPs) and added as an integer.
//
// The product [64 a x KP] . [KP x 256 j] is matrix shaped, but KP <= 16 and the elementwise tail (the residual, its mask and four
// sums) is as long as the product: it stays on the vector pipe in plain fp32.
//
// The chunk split is that of nadm_chunk_ranges.h.  Its row lookup and piece load are not used here: a lane without a sample (a >= ba)
// loads nothing at all and a piece past the row's end is skipped rather than clamped, and the group's rows are kept as row numbers (their
// single bytes are addressed per chunk): with range_row's pointers the kernel measured 0.25 % slower.
#include "nadm_chunk_ranges.h"
#include "nadm_em_accum.h"

namespace nadm {

constexpr int RC_CHUNK = RANGE_CHUNK;     // = threads per block
constexpr int RC_ROWS = 256;              // samples a per block: four waves, a lane per sample
constexpr int RC_MAX_CHUNKS = 1024;       // chunks per range at most: no fp32 running sum covers more than 2^18 SNPs (n exact: < 2^24)
constexpr int64_t RC_BLOCKS = 512;        // blocks wanted at least (256 CUs x 2 blocks of 4 waves), while there are chunks to split
constexpr int RC_MAX_KP = 16;
// left-out samples per group: their f rows take GB x 256 x KP floats of LDS, 48 KB at most, so that two blocks stay resident on a CU
__host__ __device__ constexpr int rc_group(int kp) { return kp >= 16 ? 3 : 4; }

template <int KP>
__global__ __launch_bounds__(SWEEP_CHUNK) void em_sums_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ bcpart, int32_t* __restrict__ npart) {
    em_sums_accumulate<KP>(xp, ld, idx, b, M, P, Q, q_stride, eps, one_m_eps, slices, tiles_per_slice, Mp, bcpart, npart);
}

// One thread per (SNP j < M, column c < kp): the slices' partials in slice order in float64, rounded to fp32 once; pad columns 0
__global__ __launch_bounds__(256) void em_sums_fold_kernel(const float* __restrict__ bcpart, const int32_t* __restrict__ npart,
                                                           const int slices, const int64_t Mp, const int64_t M, const int k, const int kp,
                                                           float* __restrict__ Bout, float* __restrict__ Cout,
                                                           int32_t* __restrict__ nobs_snp) {
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
    Bout[e] = c < k ? (float)Bs : 0.f;
    Cout[e] = c < k ? (float)Cs : 0.f;
    if (nobs_snp && c == 0) {
        int n = 0;
        for (int s = 0; s < slices; ++s) n += npart[(int64_t)s * Mp + j];
        nobs_snp[j] = n;
    }
}

template <int KP>
__global__ __launch_bounds__(RC_ROWS, 2) void resid_cor_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idxA, const int ba, const int32_t* __restrict__ idxB,
    const int bb, const int64_t M, const float* __restrict__ P, const float* __restrict__ Bsum, const float* __restrict__ Csum,
    const float* __restrict__ QA, const float* __restrict__ QB, const int q_stride, const float eps, const float one_m_eps,
    const int tiles_a, const int groups_b, const int cpr, const int64_t chunks, float* __restrict__ part) {
    constexpr int GB = rc_group(KP);
    __shared__ __attribute__((aligned(16))) float Fs[GB * RC_CHUNK * KP];       // f^{-b}_j. of the chunk, per b of the group
    __shared__ __attribute__((aligned(16))) float Ds[GB * RC_CHUNK * 2];        // (d_bj, o_bj)
    __shared__ __attribute__((aligned(16))) float Qbs[GB * KP];                 // the group's q rows
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int gb = (int)(blockIdx.x % groups_b);
    const int rest = (int)(blockIdx.x / groups_b);
    const int ta = rest % tiles_a, r = rest / tiles_a;
    const auto [c_lo, c_hi] = chunk_range(r, cpr, chunks);

    const int a = ta * RC_ROWS + wave * 64 + lane;
    const bool live = a < ba;
    const bool wave_live = ta * RC_ROWS + wave * 64 < ba;       // wave-uniform: a wave without a sample only helps to build
    const int64_t rowA = live ? (idxA ? (int64_t)idxA[a] : (int64_t)a) : 0;
    float q[KP];
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = *reinterpret_cast<const float4*>(QA + (int64_t)a * q_stride + k);
        q[k] = v.x; q[k + 1] = v.y; q[k + 2] = v.z; q[k + 3] = v.w;
    }
    // the group's samples, clamped to the block: a b >= bb repeats the last one and is never written
    int64_t rowB[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int bs = min(gb * GB + g, bb - 1);
        rowB[g] = idxB ? (int64_t)idxB[bs] : (int64_t)bs;
    }
    if (t < GB * KP) Qbs[t] = QB[(int64_t)min(gb * GB + t / KP, bb - 1) * q_stride + t % KP];       // visible after the first barrier

    float S[GB], Ta[GB], Tb[GB], Nn[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) S[g] = Ta[g] = Tb[g] = Nn[g] = 0.f;

#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        const int64_t j0 = c * RC_CHUNK;
        // this lane's row: the chunk's 64 bytes, in flight under the build (16-byte pieces past the row's end read as zeros; their
        // SNPs are >= M anyway)
        uint32_t w[16];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (live && c * (RC_CHUNK / 4) + 16 * (v + 1) <= ld) u = *reinterpret_cast<const uint4*>(xp + rowA * ld + c * (RC_CHUNK / 4) + 16 * v);
            w[4 * v] = u.x; w[4 * v + 1] = u.y; w[4 * v + 2] = u.z; w[4 * v + 3] = u.w;
        }
        __syncthreads();                                        // the previous chunk's rows have been read by every wave

        // ---- build: thread t owns SNP j0 + t (a SNP >= M reads row M - 1 and becomes code 3)
        {
            const int64_t j = j0 + t;
            const int64_t jc = j < M ? j : M - 1;
            const uint32_t past_m = 3u & ~lt_mask64(j, M);
            float p[KP], Bv[KP], Cv[KP], den[KP];
#pragma unroll
            for (int k = 0; k < KP; k += 4) {
                const float4 pv = *reinterpret_cast<const float4*>(P + jc * KP + k);
                const float4 bv = *reinterpret_cast<const float4*>(Bsum + jc * KP + k);
                const float4 cv = *reinterpret_cast<const float4*>(Csum + jc * KP + k);
                p[k] = pv.x; p[k + 1] = pv.y; p[k + 2] = pv.z; p[k + 3] = pv.w;
                Bv[k] = bv.x; Bv[k + 1] = bv.y; Bv[k + 2] = bv.z; Bv[k + 3] = bv.w;
                Cv[k] = cv.x; Cv[k + 1] = cv.y; Cv[k + 2] = cv.z; Cv[k + 3] = cv.w;
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) den[k] = p[k] * Bv[k] + (1.f - p[k]) * Cv[k];
            const int64_t boff = min(c * (RC_CHUNK / 4) + (t >> 2), ld - 1);     // a byte past the row's end holds SNPs >= M only
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const uint32_t code = (((uint32_t)xp[rowB[g] * ld + boff] >> (2 * (t & 3))) | past_m) & 3u;
                const uint32_t m = obs_mask(code);
                const float* qb = Qbs + g * KP;
                float rr = 0.f;
#pragma unroll
                for (int k = 0; k < KP; ++k) rr = fmaf(qb[k], p[k], rr);
                const EmTerms e = em_terms(rr, code, m, eps, one_m_eps);       // b's own terms of B and C, as they entered the sums
                float f[KP];
                float pib = 0.f;
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const float nb = fmaxf(Bv[k] - qb[k] * e.t1, 0.f);
                    const float nc = fmaxf(Cv[k] - qb[k] * e.t0, 0.f);
                    const float numn = p[k] * nb;
                    const float denn = numn + (1.f - p[k]) * nc;
                    // the branch, decided in fp32 on these values (include/nadm.h); a NaN compares false and keeps p
                    const bool take = denn >= NADM_LOO_MIN_SHARE * den[k] && den[k] > 0.f && denn > 0.f;
                    f[k] = take ? numn / denn : p[k];
                    pib = fmaf(qb[k], f[k], pib);
                }
                float* fr = Fs + (g * RC_CHUNK + t) * KP;
#pragma unroll
                for (int k = 0; k < KP; k += 4) *reinterpret_cast<float4*>(fr + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
                *reinterpret_cast<float2*>(Ds + (g * RC_CHUNK + t) * 2) = make_float2(keepf(fmaf(-2.f, pib, e.g), m), keepf(1.f, m));
            }
        }
        __syncthreads();
        if (!wave_live) continue;

        // ---- this lane's sample against the group, SNP by SNP
#pragma unroll 1
        for (int wi = 0; wi < 16; ++wi) {                       // one 32-bit word = 16 SNPs
            const int64_t left = M - (j0 + 16 * wi);
            if (left <= 0) break;                               // (wave-uniform) nothing but SNPs >= M from here on
            uint32_t bits = w[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) bits = (wi == i) ? w[i] : bits;       // (w stays in registers: no dynamic index)
            if (left < 16) bits |= 0xFFFFFFFFu << (2 * (int)left);             // SNPs >= M become code 3, once per word
#pragma unroll 2
            for (int i = 0; i < 16; ++i) {
                const uint32_t code = (bits >> (2 * i)) & 3u;
                const uint32_t m = obs_mask(code);
                const float gf = (float)code;
                const float oa = keepf(1.f, m);
                const int s = wi * 16 + i;
#pragma unroll
                for (int g = 0; g < GB; ++g) {
                    const float* fr = Fs + (g * RC_CHUNK + s) * KP;             // the same address in every lane: a broadcast
                    float pi = 0.f;
#pragma unroll
                    for (int k = 0; k < KP; k += 4) {
                        const float4 f4 = *reinterpret_cast<const float4*>(fr + k);
                        pi = fmaf(q[k], f4.x, pi); pi = fmaf(q[k + 1], f4.y, pi);
                        pi = fmaf(q[k + 2], f4.z, pi); pi = fmaf(q[k + 3], f4.w, pi);
                    }
                    const float2 dv = *reinterpret_cast<const float2*>(Ds + (g * RC_CHUNK + s) * 2);
                    const float da = keepf(fmaf(-2.f, pi, gf), m);
                    S[g] = fmaf(da, dv.x, S[g]);
                    Ta[g] = fmaf(da * da, dv.y, Ta[g]);
                    Tb[g] = fmaf(dv.x * dv.x, oa, Tb[g]);
                    Nn[g] = fmaf(oa, dv.y, Nn[g]);
                }
            }
        }
    }
    if (!live) return;
    float* out = part + ((int64_t)blockIdx.x * RC_ROWS + wave * 64 + lane) * (GB * 4);
#pragma unroll
    for (int g = 0; g < GB; ++g) *reinterpret_cast<float4*>(out + 4 * g) = make_float4(S[g], Ta[g], Tb[g], Nn[g]);
}

// One thread per pair (a < ba, b < bb): the ranges' partials in range order, in float64
__global__ __launch_bounds__(256) void resid_cor_fold_kernel(const float* __restrict__ part, const int ranges, const int tiles_a,
                                                             const int groups_b, const int GB, const int ba, const int bb,
                                                             double* __restrict__ S, double* __restrict__ Ta, double* __restrict__ Tb,
                                                             int32_t* __restrict__ nobs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)ba * bb) return;
    const int a = (int)(e / bb), b = (int)(e - (int64_t)a * bb);
    const int ta = a / RC_ROWS, al = a % RC_ROWS, gb = b / GB, g = b % GB;
    double s = 0.0, va = 0.0, vb = 0.0;
    int n = 0;
    for (int r = 0; r < ranges; ++r) {
        const float* p = part + ((((int64_t)r * tiles_a + ta) * groups_b + gb) * RC_ROWS + al) * (GB * 4) + 4 * g;
        s += (double)p[0];
        va += (double)p[1];
        vb += (double)p[2];
        n += (int)p[3];
    }
    S[e] = s;
    Ta[e] = va;
    Tb[e] = vb;
    if (nobs) nobs[e] = n;
}

// the launch shape, a rule of (ba, bb, M, kp) alone: a "tile" is 256 samples a x one group of b
static RangePlan rc_plan(int ba, int bb, int64_t M, int kp) { return range_plan(M, range_tiles(ba, RC_ROWS, bb, rc_group(kp)), RC_BLOCKS, RC_MAX_CHUNKS); }
static bool rc_shape_ok(int ba, int bb, int64_t M, int kp) {
    return pair_block_ok(ba, bb, M, NADM_RESID_COR_MAX_ROWS) && kp >= 4 && kp <= RC_MAX_KP && kp % 4 == 0;
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_em_sums_slices(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_slices(b, M); }

// scratch: B | C partials [slices, Mp, 2 kp] float | n partials [slices, Mp] int32, Mp = 256 chunks (nadm_project_p's)
extern "C" int64_t nadm_em_sums_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    return (b <= 0 || M <= 0 || kp <= 0 || kp > NADM_MAX_K) ? 0 : sweep_rows_bound(b, M) * (2 * (int64_t)kp + 1);
}

extern "C" int nadm_em_sums(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                            int32_t k, int32_t kp, const float* P, float eps, float* B, float* C, int32_t* nobs_snp, float* scratch,
                            void* stream) {
    if (!xp || !Q || !P || !B || !C || !scratch) return fail("nadm_em_sums: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_em_sums: empty batch (need b > 0 and M > 0)");
    if (check_packed("nadm_em_sums", ld, M) || check_head("nadm_em_sums", k, kp, q_stride) || check_eps("nadm_em_sums", eps)) return 1;
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)P | (uintptr_t)B | (uintptr_t)C | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_em_sums: xp, Q, P, B, C and scratch must be 16-byte aligned");
    if ((((uintptr_t)nobs_snp | (uintptr_t)idx) & 3) != 0) return fail("nadm_em_sums: nobs_snp and idx must be 4-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll || (M * kp + 255) / 256 > 0x7FFFFFFFll) return fail("nadm_em_sums: too many blocks for one launch");
    float* bcpart = scratch;
    int32_t* npart = reinterpret_cast<int32_t*>(scratch + (int64_t)slices * Mp * 2 * kp);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps;
    if (int e = dispatch_kp("nadm_em_sums", kp, [&](auto KP) {
            hipLaunchKernelGGL((em_sums_accum_kernel<decltype(KP)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld, idx, b, M, P, Q,
                               q_stride, eps, ome, slices, tps, Mp, bcpart, npart);
        }))
        return e;
    if (int e = check_launch("em_sums (accumulate)")) return e;
    hipLaunchKernelGGL(em_sums_fold_kernel, dim3((unsigned)((M * kp + 255) / 256)), dim3(256), 0, st, bcpart, npart, slices, Mp, M, k, kp, B, C,
                       nobs_snp);
    return check_launch("em_sums (fold)");
}

extern "C" int32_t nadm_resid_cor_ranges(int32_t ba, int32_t bb, int64_t M, int32_t kp) {
    return rc_shape_ok(ba, bb, M, kp) ? range_count(rc_plan(ba, bb, M, kp).ranges) : 0;
}

// scratch: [ranges][256-sample tiles of a][groups of b][256][GB][S | Ta | Tb | n] float: bounded by ranges x ba x bb, never per chunk
extern "C" int64_t nadm_resid_cor_scratch_floats(int32_t ba, int32_t bb, int64_t M, int32_t kp) {
    return rc_shape_ok(ba, bb, M, kp) ? rc_plan(ba, bb, M, kp).blocks_bound * (RC_ROWS * rc_group(kp) * 4) : 0;
}

extern "C" int nadm_resid_cor(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                              const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride, const float* B,
                              const float* C, float eps, double* S, double* Ta, double* Tb, int32_t* nobs, float* scratch, void* stream) {
    if (!xp || !P || !QA || !QB || !B || !C || !S || !Ta || !Tb || !scratch) return fail("nadm_resid_cor: null pointer");
    if (check_pair_block("nadm_resid_cor", ba, bb, M, PAIR_MAX_ROWS(NADM_RESID_COR_MAX_ROWS))) return 1;
    if (check_packed("nadm_resid_cor", ld, M) || check_head("nadm_resid_cor", k, kp, q_stride) || check_eps("nadm_resid_cor", eps)) return 1;
    if (kp > RC_MAX_KP)
        return fail("nadm_resid_cor: K must be <= 16 (a sample's Q row and the refitted frequencies of a chunk live in registers and LDS)");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)QA | (uintptr_t)QB | (uintptr_t)B | (uintptr_t)C | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_resid_cor: xp, P, QA, QB, B, C and scratch must be 16-byte aligned");
    if ((((uintptr_t)S | (uintptr_t)Ta | (uintptr_t)Tb) & 7) != 0 || (((uintptr_t)nobs | (uintptr_t)idxA | (uintptr_t)idxB) & 3) != 0)
        return fail("nadm_resid_cor: S, Ta, Tb must be 8-byte and nobs, idxA, idxB 4-byte aligned");
    const int GB = rc_group(kp);
    const RangePlan pl = rc_plan(ba, bb, M, kp);
    if (range_launch_check("nadm_resid_cor", pl)) return 1;
    const int tiles_a = (ba + RC_ROWS - 1) / RC_ROWS, groups_b = (bb + GB - 1) / GB;
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - eps;
    if (int e = dispatch_kp("nadm_resid_cor", kp, [&](auto KP) {
            if constexpr (decltype(KP)::value <= RC_MAX_KP)
                hipLaunchKernelGGL((resid_cor_accum_kernel<decltype(KP)::value>), range_grid(pl), dim3(RC_ROWS), 0, st, xp, ld, idxA, ba, idxB, bb,
                                   M, P, B, C, QA, QB, q_stride, eps, ome, tiles_a, groups_b, (int)pl.cpr, pl.chunks, scratch);
        }))
        return e;
    if (int e = check_launch("resid_cor (accumulate)")) return e;
    hipLaunchKernelGGL(resid_cor_fold_kernel, fold_grid((int64_t)ba * bb), dim3(256), 0, st, scratch, (int)pl.ranges, tiles_a, groups_b, GB, ba,
                       bb, S, Ta, Tb, nobs);
    return check_launch("resid_cor (fold)");
}
