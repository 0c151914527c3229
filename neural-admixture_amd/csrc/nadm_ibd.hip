// IBD-sharing sums given ancestry (PC-Relate's k2 and k0 estimators, Conomos et al. 2016, with the admixture model's individual-specific
// frequencies) of one block of sample pairs from the packed matrix, Q, one head's P and the samples' inbreeding coefficients
// (include/nadm.h, nadm_ibd): four Gram products over the SNP axis on v_mfma_f32_16x16x32_bf16.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   ibd_accum_kernel   one 256-thread block per (64 x 64 tile of A samples x B samples, range of 256-SNP chunks), on PairBuilder of
//                      nadm_chunk_ranges.h as kinship_accum_kernel is: the builder role, the chunk walk in eight steps of 32 SNPs, pi
//                      and the mask are its.  BUILD: from pi and m the six operands e, vm, u, w, z0, z2 of the header, the first four
//                      split into two RNE bf16 pieces each: TEN 16-byte fragments for each of the thread's two (sample, group)
//                      pairs.  The operand image [slot][group][sample] in
//                      LDS has room for SIX pieces (48 KB), and a step goes through it in two halves:
//                        half 1   slots 0..3 = e_hi, e_lo, vm_hi, vm_lo (slots 4, 5 = z0, z2 are written with them)
//                                 -> 6 instructions per 16 x 16 tile (hi.hi + hi.lo + lo.hi of e.e and of vm.vm)
//                        half 2   slots 0..3 = u_hi, u_lo, w_hi, w_lo, which waited in 32 registers
//                                 -> 8 instructions per tile (the three of u.w and the three of w.u into ONE accumulator; z0.z2 and
//                                    z2.z0 into one)
//                      All ten pieces at once would be 80 KB of image, 96 KB with P at kp = 16: one block per compute unit.  In halves a
//                      block takes 52 .. 64 KB and two blocks share a compute unit as in nadm_kinship, so that one block's build (vector
//                      ALU) runs under the other's multiply (matrix pipe); the price is two more barriers per step.  Wave w owns A rows
//                      16 w .. 16 w + 15 against the four 16-sample B tiles; the 16 fp32 accumulators of a lane live for the whole range.
//                      Missing calls, SNPs >= M, rows past the list and masked pi enter as exactly +0.0f through bit masks, whatever f is.
//   pair_fold_kernel   (with IbdSum) one thread per pair: the ranges' partials in range order in float64; ibs0 as int32.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int IBD_CHUNK = RANGE_CHUNK;
constexpr int IBD_TILE = PAIR_TILE;       // samples per tile side
constexpr int IBD_MAX_CHUNKS = 1024;      // chunks per range at most: no fp32 accumulator covers more than 2^18 SNPs (ibs0 exact: < 2^24)
constexpr int64_t IBD_BLOCKS = 512;       // blocks wanted at least (256 CUs x 2 blocks of 4 waves), while there are chunks to split
constexpr int IBD_MAX_KP = 16;
constexpr int IBD_SLOTS = 6;              // pieces the LDS image holds at a time (half 2 of a step)
constexpr int IBD_SLOT = 4 * 2 * IBD_TILE;        // fragments of one piece: [group 0..3][sample 0..127]
constexpr int IBD_PLANES = 4;             // k2num, k2den, ibs0, exp0

// x == 0 ? ~0 : 0 for x in 0..3, as arithmetic (opaque: see lt_mask)
__device__ __forceinline__ uint32_t ibd_eq0_mask(uint32_t x) {
    uint32_t m = (uint32_t)((int)(x - 1u) >> 31);
    asm("" : "+v"(m));
    return m;
}

template <int KP>
__global__ __launch_bounds__(256, 2) void ibd_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idxA, const int ba, const int32_t* __restrict__ idxB,
    const int bb, const int64_t M, const float* __restrict__ P, const float* __restrict__ QA, const float* __restrict__ QB,
    const int q_stride, const float* __restrict__ fA, const float* __restrict__ fB, const float pimin, const float one_m_pimin,
    const int tiles_b, const int ranges, const int chunks_per_range, const int64_t chunks, float* __restrict__ part) {
    static_assert(KP <= IBD_MAX_KP && KP % 4 == 0, "a sample's Q row lives in registers");
    __shared__ __attribute__((aligned(16))) float Ps[IBD_CHUNK * KP];
    __shared__ __attribute__((aligned(16))) u32x4_t Img[IBD_SLOTS * IBD_SLOT];                 // [slot][group][sample 0..127]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tile = (int)blockIdx.x / ranges, range = (int)blockIdx.x - tile * ranges;
    const PairBuilder<KP> bld(xp, ld, idxA, ba, idxB, bb, QA, QB, q_stride, tile / tiles_b, tile % tiles_b);
    const float opf = 1.f + (bld.isA ? fA : fB)[bld.rr.posc];     // 1 + f of the sample (any value: a masked call is cleared by bits)

    enum { N = 0, D = 1, I = 2, X = 3 };                          // the slab's planes: k2num, k2den, ibs0, exp0
    f32x4_t acc[IBD_PLANES][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[N][i] = acc[D][i] = acc[I][i] = acc[X][i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    bld.walk(chunk_range(range, chunks_per_range, chunks), ld, M, P, Ps, [&](const int st, const uint32_t (&cw)[16], const int left) {
        // ---- build: the ten operand fragments of two (sample, group) pairs per thread
        u32x4_t fr[2][4];                                         // u_hi, u_lo, w_hi, w_lo of the two pairs
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const PairGroup gr = bld.group(st, it, cw, left);
            float pi[8];
            bld.pi8(Ps, gr.jl, pi);
            float ev[8], vv[8], uv[8], wv[8];
            uint32_t m0[8], m2[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t code = (gr.bits >> (2 * e)) & 3u;
                const uint32_t m = bld.mask(code, e, gr.rem, pi[e], pimin, one_m_pimin);
                const uint32_t is0 = ibd_eq0_mask(code), is2 = ibd_eq0_mask(code ^ 2u);
                const float omp = 1.f - pi[e];
                const float v = pi[e] * omp;
                // dominance coding gD: pi at g = 0, 0 at g = 1, 1 - pi at g = 2 (the two masks are disjoint)
                const float gd = __uint_as_float((__float_as_uint(pi[e]) & is0) | (__float_as_uint(omp) & is2));
                ev[e] = keepf(fmaf(-v, opf, gd), m);
                vv[e] = keepf(v, m);
                uv[e] = keepf(pi[e] * pi[e], m);
                wv[e] = keepf(omp * omp, m);
                m0[e] = m & is0;
                m2[e] = m & is2;
            }
            // half 1's pieces and the indicators go straight into the image (the previous step's half 2 ended with a barrier, and
            // half 1 does not read slots 4 and 5); u and w wait in registers for half 2
            u32x4_t eh, el, vh, vl;
            split8(ev, eh, el);
            split8(vv, vh, vl);
            split8(uv, fr[it][0], fr[it][1]);
            split8(wv, fr[it][2], fr[it][3]);
            u32x4_t* o = Img + gr.g * (2 * IBD_TILE) + bld.s;
            o[0 * IBD_SLOT] = eh;
            o[1 * IBD_SLOT] = el;
            o[2 * IBD_SLOT] = vh;
            o[3 * IBD_SLOT] = vl;
            o[4 * IBD_SLOT] = ones8(m0);
            o[5 * IBD_SLOT] = ones8(m2);
        }
        // lane l is row / column l & 15 and group l >> 4 of both operands
        const u32x4_t* ia = Img + (lane >> 4) * (2 * IBD_TILE) + 16 * w + (lane & 15);
        const u32x4_t* ib = Img + (lane >> 4) * (2 * IBD_TILE) + IBD_TILE + (lane & 15);
        __syncthreads();
        // ---- half 1: e.e and vm.vm
        {
            bf16x8_t a[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) a[p] = frag(ia[p * IBD_SLOT]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x8_t b[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) b[p] = frag(ib[p * IBD_SLOT + 16 * j]);
                acc[N][j] = mfma_split(acc[N][j], a[0], a[1], b[0], b[1]);
                acc[D][j] = mfma_split(acc[D][j], a[2], a[3], b[2], b[3]);
            }
        }
        __syncthreads();
        // ---- half 2: u and w over e and vm; u.w + w.u and the two indicator products
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            u32x4_t* o = Img + (bld.g0 + 2 * it) * (2 * IBD_TILE) + bld.s;
#pragma unroll
            for (int p = 0; p < 4; ++p) o[p * IBD_SLOT] = fr[it][p];
        }
        __syncthreads();
        {
            bf16x8_t a[6];                                        // u_hi, u_lo, w_hi, w_lo, z0, z2
#pragma unroll
            for (int p = 0; p < 6; ++p) a[p] = frag(ia[p * IBD_SLOT]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x8_t b[6];
#pragma unroll
                for (int p = 0; p < 6; ++p) b[p] = frag(ib[p * IBD_SLOT + 16 * j]);
                // the two split products interleaved into ONE accumulator: this order is the sum's bits
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[2], acc[X][j], 0, 0, 0);      // u_a w_b: lo.hi
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[3], b[0], acc[X][j], 0, 0, 0);      // w_a u_b: lo.hi
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[3], acc[X][j], 0, 0, 0);      // u_a w_b: hi.lo
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[1], acc[X][j], 0, 0, 0);      // w_a u_b: hi.lo
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc[X][j], 0, 0, 0);      // u_a w_b: hi.hi
                acc[X][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc[X][j], 0, 0, 0);      // w_a u_b: hi.hi
                acc[I][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[4], b[5], acc[I][j], 0, 0, 0);      // z0_a z2_b
                acc[I][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[5], b[4], acc[I][j], 0, 0, 0);      // z2_a z0_b
            }
        }
        __syncthreads();
    });
    pair_slab_store<IBD_PLANES>(part, range, ranges, tile, acc);
}

// pair_fold_kernel's sums: k2num, k2den and exp0 in float64 (each fp32 partial cast before the add), ibs0 as an integer
struct IbdSum {
    struct Out { double *k2num, *k2den; int32_t* ibs0; double* exp0; } out;
    double ns = 0.0, ds = 0.0, xs = 0.0;
    int n = 0;
    __device__ __forceinline__ void add(const int plane, const float v) {
        if (plane == 0) ns += (double)v; else if (plane == 1) ds += (double)v; else if (plane == 2) n += (int)v; else xs += (double)v;
    }
    __device__ __forceinline__ void store(const int64_t e, int64_t) const {
        out.k2num[e] = ns; out.k2den[e] = ds; out.ibs0[e] = n; out.exp0[e] = xs;
    }
};

// the launch shape, a rule of (ba, bb, M) alone
static RangePlan ibd_plan(int ba, int bb, int64_t M) { return range_plan(M, range_tiles(ba, IBD_TILE, bb, IBD_TILE), IBD_BLOCKS, IBD_MAX_CHUNKS); }
static bool ibd_shape_ok(int ba, int bb, int64_t M) { return pair_block_ok(ba, bb, M, NADM_IBD_MAX_ROWS); }

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_ibd_ranges(int32_t ba, int32_t bb, int64_t M) { return ibd_shape_ok(ba, bb, M) ? range_count(ibd_plan(ba, bb, M).ranges) : 0; }

// scratch: [ranges][tiles][k2num | k2den | ibs0 | exp0][64 x 64] float
extern "C" int64_t nadm_ibd_scratch_floats(int32_t ba, int32_t bb, int64_t M) {
    return ibd_shape_ok(ba, bb, M) ? ibd_plan(ba, bb, M).blocks_bound * (IBD_PLANES * IBD_TILE * IBD_TILE) : 0;
}

extern "C" int nadm_ibd(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                        const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride, const float* fA,
                        const float* fB, float pimin, double* k2num, double* k2den, int32_t* ibs0, double* exp0, float* scratch,
                        void* stream) {
    const char* who = "nadm_ibd";
    if (!xp || !P || !QA || !QB || !fA || !fB || !k2num || !k2den || !ibs0 || !exp0 || !scratch) return failf(who, "null pointer");
    if (check_pair_block(who, ba, bb, M, PAIR_MAX_ROWS(NADM_IBD_MAX_ROWS))) return 1;
    if (check_packed(who, ld, M) || check_head(who, k, kp, q_stride)) return 1;
    if (kp > IBD_MAX_KP)
        return failf(who, "K must be <= 16 (a sample's Q row lives in its builder thread's registers and the staged P beside the operand "
                          "image lets two blocks share a compute unit only up to kp = 16)");
    if (!(pimin >= 0.f && pimin < 0.5f)) return failf(who, "pimin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)QA | (uintptr_t)QB | (uintptr_t)scratch) & 15) != 0)
        return failf(who, "xp, P, QA, QB and scratch must be 16-byte aligned");
    if ((((uintptr_t)k2num | (uintptr_t)k2den | (uintptr_t)exp0) & 7) != 0 ||
        (((uintptr_t)ibs0 | (uintptr_t)fA | (uintptr_t)fB | (uintptr_t)idxA | (uintptr_t)idxB) & 3) != 0)
        return failf(who, "k2num, k2den, exp0 must be 8-byte and ibs0, fA, fB, idxA, idxB 4-byte aligned");
    const RangePlan pl = ibd_plan(ba, bb, M);
    if (range_launch_check(who, pl)) return 1;
    const int tiles_b = (bb + IBD_TILE - 1) / IBD_TILE;
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - pimin;
    if (int e = dispatch_kp(who, kp, [&](auto KP) {
            if constexpr (decltype(KP)::value <= IBD_MAX_KP)
                hipLaunchKernelGGL((ibd_accum_kernel<decltype(KP)::value>), range_grid(pl), dim3(256), 0, st, xp, ld, idxA, ba, idxB, bb, M, P,
                                   QA, QB, q_stride, fA, fB, pimin, ome, tiles_b, (int)pl.ranges, (int)pl.cpr, pl.chunks, scratch);
        }))
        return e;
    if (int e = check_launch("ibd (accumulate)")) return e;
    launch_pair_fold<float, IBD_PLANES, IbdSum>(scratch, pl, ba, bb, {k2num, k2den, ibs0, exp0}, st);
    return check_launch("ibd (fold)");
}
