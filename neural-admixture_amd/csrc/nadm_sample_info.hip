// Standard errors of Q given P: the per-SAMPLE Fisher information of a sample's row of ancestry fractions GIVEN the allele frequencies,
// in the binomial admixture model (include/nadm.h, nadm_sample_info).  The mirror image of nadm_snp_info.hip: one pass of
// N M K^2 / 2 work over the packed matrix with the K (K + 1) / 2 running sums per sample, not per SNP.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   sample_info_accum_kernel  a sample-owning kernel on the chunk-range plan of nadm_chunk_ranges.h: one 256-thread block per (tile of 256
//                             rows of the list, range of consecutive 256-SNP chunks), a lane per sample.  The lane's q row, the chunk's
//                             16 packed words (the next chunk's are loaded under the current chunk's work), the T = KP (KP + 1) / 2
//                             running sums of the upper triangle (fp32) and n (int32) live in registers for the whole range.  The chunk's
//                             P rows sit in LDS once per block and every lane reads the SAME row (a broadcast: project_accum_kernel's
//                             arrangement).  Per genotype: KP multiply-adds for pi, two clips, one multiply and one reciprocal for the
//                             weight 1 / (r u), KP multiplies for w p_a, T multiply-adds.  Missing calls (code 3), rows past the list and
//                             SNPs >= M are code 3 before the decode and enter every sum as exactly +0.0f / 0.  A wave whose 64 rows are
//                             all past the list stages and waits with the block and skips the arithmetic.  Writes the range's slab
//                             plane by plane (a wave's stores are contiguous), n as plane T.
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
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);
    const RangeRow rr = range_row(xp, ld, idx, tile * SI_TILE + t, b);
    const uint32_t inval = ~rr.valid;                             // a row past the list: every call missing
    const bool wave_live = tile * SI_TILE + (t & ~63) < b;        // wave-uniform

    float q[KP];
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(Q + (int64_t)rr.posc * q_stride + k);
        q[k] = t4.x; q[k + 1] = t4.y; q[k + 2] = t4.z; q[k + 3] = t4.w;
    }
    float acc[T];
#pragma unroll
    for (int i = 0; i < T; ++i) acc[i] = 0.f;
    int n = 0;

    u32x4_t nxt[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, c_lo, v, ld);

#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        const int64_t j0 = c * RANGE_CHUNK;
        if (c > c_lo) __syncthreads();                            // the previous chunk's rows have been read
        {
            // the chunk's P rows into LDS (rows >= M as zeros): RANGE_CHUNK * KP / 4 float4, coalesced
            const float4* src = reinterpret_cast<const float4*>(P + j0 * KP);
            const int64_t lim = (M - j0) * (KP / 4);              // float4 of the chunk that exist
#pragma unroll
            for (int e = t; e < RANGE_CHUNK * KP / 4; e += SI_TILE)
                reinterpret_cast<float4*>(Ps)[e] = e < lim ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        uint32_t w[16];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            w[4 * v] = nxt[v][0] | inval; w[4 * v + 1] = nxt[v][1] | inval;
            w[4 * v + 2] = nxt[v][2] | inval; w[4 * v + 3] = nxt[v][3] | inval;
        }
        {
            const int64_t cn = min(c + 1, c_hi - 1);              // the next chunk's words, in flight under this chunk's arithmetic
#pragma unroll
            for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cn, v, ld);
        }
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll 1
        for (int wi = 0; wi < 16; ++wi) {                         // one 32-bit word = 16 SNPs
            uint32_t bits = w[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) bits = (wi == i) ? w[i] : bits;     // (w stays in registers: no dynamic index)
            // SNPs >= M become code 3 here, once per word (wave-uniform): with them the pad bits of the row's last byte and what lies behind
            const int64_t left = M - (j0 + 16 * wi);
            if (left < 16) bits |= left <= 0 ? 0xFFFFFFFFu : (0xFFFFFFFFu << (2 * (int)left));
#pragma unroll 4
            for (int e = 0; e < 16; ++e) {
                const uint32_t m = obs_mask((bits >> (2 * e)) & 3u);
                const float* pr = Ps + (wi * 16 + e) * KP;
                float p[KP];
                float pi = 0.f;
#pragma unroll
                for (int k = 0; k < KP; k += 4) {                 // a broadcast: the row is read once, four columns at a time
                    const float4 t4 = *reinterpret_cast<const float4*>(pr + k);
                    p[k] = t4.x; p[k + 1] = t4.y; p[k + 2] = t4.z; p[k + 3] = t4.w;
                    pi = fmaf(q[k], t4.x, pi); pi = fmaf(q[k + 1], t4.y, pi);
                    pi = fmaf(q[k + 2], t4.z, pi); pi = fmaf(q[k + 3], t4.w, pi);
                }
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
            }
        }
    }
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
