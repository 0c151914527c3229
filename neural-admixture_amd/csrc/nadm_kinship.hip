// Admixture-aware kinship (REAP, Thornton et al. 2012) of one block of sample pairs from the packed matrix, Q and one head's P
// (include/nadm.h, nadm_kinship): two Gram products over the SNP axis and a count, on v_mfma_f32_16x16x32_bf16.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   kinship_accum_kernel  one 256-thread block per (64 x 64 tile of A samples x B samples, range of 256-SNP chunks), on PairBuilder of
//                         nadm_chunk_ranges.h: the builder role, the chunk walk in eight steps of 32 SNPs, pi and the mask are its.
//                         BUILD: from pi and m, d = m (g - 2 pi) and s = m sqrt(pi (1 - pi)), each split into two RNE bf16 pieces;
//                         the five 16-byte operand fragments (d_hi, d_lo, s_hi, s_lo, m) of (sample, group) -- exactly what one lane
//                         of the instruction takes -- go into the LDS image [piece][group][sample]: consecutive lanes write and read
//                         consecutive 16 bytes.  MULTIPLY: wave w owns A rows 16 w .. 16 w + 15 against the four 16-sample B tiles:
//                         7 instructions per tile (lo.hi + hi.lo + hi.hi for num and for den, one for n) into fp32 accumulators
//                         that live for the whole range.  The operand image never leaves LDS.  Missing calls, SNPs >= M, rows past
//                         the list and masked pi enter as exactly +0.0f.
//   pair_fold_kernel      (with KinshipSum) one thread per pair: the ranges' partials in range order in float64; n as int32.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int KIN_CHUNK = RANGE_CHUNK;
constexpr int KIN_TILE = PAIR_TILE;       // samples per tile side
constexpr int KIN_MAX_CHUNKS = 1024;      // chunks per range at most: no fp32 accumulator covers more than 2^18 SNPs (n exact: < 2^24)
constexpr int64_t KIN_BLOCKS = 512;       // blocks wanted at least (256 CUs x 2 blocks of 4 waves), while there are chunks to split
constexpr int KIN_PIECES = 5;             // d_hi, d_lo, s_hi, s_lo, m
constexpr int KIN_SLOT = 4 * 2 * KIN_TILE;        // fragments of one piece: [group 0..3][sample 0..127]

template <int KP>
__global__ __launch_bounds__(256, KP <= 16 ? 2 : 1) void kinship_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idxA, const int ba, const int32_t* __restrict__ idxB,
    const int bb, const int64_t M, const float* __restrict__ P, const float* __restrict__ QA, const float* __restrict__ QB,
    const int q_stride, const float pimin, const float one_m_pimin, const int tiles_b, const int ranges, const int chunks_per_range,
    const int64_t chunks, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Ps[KIN_CHUNK * KP];
    __shared__ __attribute__((aligned(16))) u32x4_t Img[KIN_PIECES * KIN_SLOT];                // [piece][group][sample 0..127]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tile = (int)blockIdx.x / ranges, range = (int)blockIdx.x - tile * ranges;
    const PairBuilder<KP> bld(xp, ld, idxA, ba, idxB, bb, QA, QB, q_stride, tile / tiles_b, tile % tiles_b);

    f32x4_t acc[3][4];                                            // num, den, n
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[0][i] = acc[1][i] = acc[2][i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    bld.walk(chunk_range(range, chunks_per_range, chunks), ld, M, P, Ps, [&](const int st, const uint32_t (&cw)[16], const int left) {
        // ---- build: two (sample, group) operand fragments per thread
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const PairGroup gr = bld.group(st, it, cw, left);
            float pi[8];
            bld.pi8(Ps, gr.jl, pi);
            float dv[8], sv[8];
            uint32_t mv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t code = (gr.bits >> (2 * e)) & 3u;
                const uint32_t m = bld.mask(code, e, gr.rem, pi[e], pimin, one_m_pimin);
                mv[e] = m;
                dv[e] = keepf((float)code - 2.f * pi[e], m);
                sv[e] = keepf(__builtin_amdgcn_sqrtf(fmaxf(pi[e] * (1.f - pi[e]), 0.f)), m);
            }
            u32x4_t dh, dl, shi, slo;
            split8(dv, dh, dl);
            split8(sv, shi, slo);
            u32x4_t* o = Img + gr.g * (2 * KIN_TILE) + bld.s;
            o[0 * KIN_SLOT] = dh;
            o[1 * KIN_SLOT] = dl;
            o[2 * KIN_SLOT] = shi;
            o[3 * KIN_SLOT] = slo;
            o[4 * KIN_SLOT] = ones8(mv);
        }
        __syncthreads();
        // ---- multiply: lane l is row / column l & 15 and group l >> 4 of both operands
        const u32x4_t* ia = Img + (lane >> 4) * (2 * KIN_TILE) + 16 * w + (lane & 15);
        bf16x8_t a[KIN_PIECES];
#pragma unroll
        for (int p = 0; p < KIN_PIECES; ++p) a[p] = frag(ia[p * KIN_SLOT]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4_t* ib = Img + (lane >> 4) * (2 * KIN_TILE) + KIN_TILE + 16 * j + (lane & 15);
            bf16x8_t b[KIN_PIECES];
#pragma unroll
            for (int p = 0; p < KIN_PIECES; ++p) b[p] = frag(ib[p * KIN_SLOT]);
            acc[0][j] = mfma_split(acc[0][j], a[0], a[1], b[0], b[1]);
            acc[1][j] = mfma_split(acc[1][j], a[2], a[3], b[2], b[3]);
            acc[2][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[4], b[4], acc[2][j], 0, 0, 0);
        }
        __syncthreads();
    });
    pair_slab_store<3>(part, range, ranges, tile, acc);
}

// pair_fold_kernel's sums: num and den in float64 (each fp32 partial cast before the add), n as an integer
struct KinshipSum {
    struct Out { double *num, *den; int32_t* nobs; } out;
    double ns = 0.0, ds = 0.0;
    int n = 0;
    __device__ __forceinline__ void add(const int plane, const float v) {
        if (plane == 0) ns += (double)v; else if (plane == 1) ds += (double)v; else n += (int)v;
    }
    __device__ __forceinline__ void store(const int64_t e, int64_t) const {
        out.num[e] = ns; out.den[e] = ds;
        if (out.nobs) out.nobs[e] = n;
    }
};

// the launch shape, a rule of (ba, bb, M) alone
static RangePlan kin_plan(int ba, int bb, int64_t M) { return range_plan(M, range_tiles(ba, KIN_TILE, bb, KIN_TILE), KIN_BLOCKS, KIN_MAX_CHUNKS); }
static bool kin_shape_ok(int ba, int bb, int64_t M) { return pair_block_ok(ba, bb, M, NADM_KINSHIP_MAX_ROWS); }

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_kinship_ranges(int32_t ba, int32_t bb, int64_t M) { return kin_shape_ok(ba, bb, M) ? range_count(kin_plan(ba, bb, M).ranges) : 0; }

// scratch: [ranges][tiles][num | den | n][64 x 64] float
extern "C" int64_t nadm_kinship_scratch_floats(int32_t ba, int32_t bb, int64_t M) {
    return kin_shape_ok(ba, bb, M) ? kin_plan(ba, bb, M).blocks_bound * (3 * KIN_TILE * KIN_TILE) : 0;
}

extern "C" int nadm_kinship(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                            const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride, float pimin,
                            double* num, double* den, int32_t* nobs, float* scratch, void* stream) {
    if (!xp || !P || !QA || !QB || !num || !den || !scratch) return fail("nadm_kinship: null pointer");
    if (check_pair_block("nadm_kinship", ba, bb, M, PAIR_MAX_ROWS(NADM_KINSHIP_MAX_ROWS))) return 1;
    if (check_packed("nadm_kinship", ld, M) || check_head("nadm_kinship", k, kp, q_stride)) return 1;
    if (!(pimin >= 0.f && pimin < 0.5f)) return fail("nadm_kinship: pimin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)QA | (uintptr_t)QB | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_kinship: xp, P, QA, QB and scratch must be 16-byte aligned");
    if ((((uintptr_t)num | (uintptr_t)den) & 7) != 0 || ((uintptr_t)nobs & 3) != 0)
        return fail("nadm_kinship: num, den must be 8-byte and nobs 4-byte aligned");
    const RangePlan pl = kin_plan(ba, bb, M);
    if (range_launch_check("nadm_kinship", pl)) return 1;
    const int tiles_b = (bb + KIN_TILE - 1) / KIN_TILE;
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - pimin;
    if (int e = dispatch_kp("nadm_kinship", kp, [&](auto KP) {
            hipLaunchKernelGGL((kinship_accum_kernel<decltype(KP)::value>), range_grid(pl), dim3(256), 0, st, xp, ld, idxA, ba, idxB, bb, M, P, QA,
                               QB, q_stride, pimin, ome, tiles_b, (int)pl.ranges, (int)pl.cpr, pl.chunks, scratch);
        }))
        return e;
    if (int e = check_launch("kinship (accumulate)")) return e;
    launch_pair_fold<float, 3, KinshipSum>(scratch, pl, ba, bb, {num, den, nobs}, st);
    return check_launch("kinship (fold)");
}
