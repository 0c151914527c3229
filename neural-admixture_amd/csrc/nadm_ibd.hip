// IBD-sharing sums given ancestry (PC-Relate's k2 and k0 estimators, Conomos et al. 2016, with the admixture model's individual-specific
// frequencies) of one block of sample pairs from the packed matrix, Q, one head's P and the samples' inbreeding coefficients
// (include/nadm.h, nadm_ibd): four Gram products over the SNP axis on v_mfma_f32_16x16x32_bf16.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   ibd_accum_kernel   the shape of kinship_accum_kernel (nadm_kinship.hip): one 256-thread block per (64 x 64 tile of A samples x B
//                      samples, range of 256-SNP chunks); per chunk the chunk's P rows are staged in LDS and every thread keeps its
//                      sample's 64 packed bytes in registers (the next chunk's are loaded under the current chunk's work); a chunk is
//                      worked off in eight steps of 32 SNPs = one K of the instruction.  BUILD: thread t owns sample t & 127 of the 128
//                      (64 A then 64 B) and two of the step's four 8-SNP groups.  It decodes, forms pi (fp32, k in order), the mask m and
//                      the six operands e, vm, u, w, z0, z2 of the header, splits the first four into two RNE bf16 pieces each and so
//                      has the TEN 16-byte fragments of each of its two (sample, group) pairs.  The operand image [slot][group][sample] in
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
// The chunk split, the row lookup, the clamped piece load and the fold are those of nadm_chunk_ranges.h.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int IBD_CHUNK = RANGE_CHUNK;
constexpr int IBD_TILE = PAIR_TILE;       // samples per tile side
constexpr int IBD_STEP = 32;              // SNPs per build / multiply step = K of the instruction
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
// eight fp32 values -> their round-to-nearest bf16 pieces hi and lo = rne(v - hi), element e in half e & 1 of dword e >> 1
__device__ __forceinline__ void ibd_split(const float (&v)[8], u32x4_t& hi, u32x4_t& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
        lo[i] = pk_bf16(v[2 * i] - __uint_as_float(hi[i] << 16), v[2 * i + 1] - __uint_as_float(hi[i] & 0xFFFF0000u));
    }
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
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = (int)blockIdx.x / ranges, range = (int)blockIdx.x - tile * ranges;
    const int ta = tile / tiles_b, tb = tile - ta * tiles_b;
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);

    // builder role: sample s of the 128 (A rows of the tile, then B rows), groups g0 and g0 + 2 of every step
    const int s = t & 127, g0 = t >> 7;
    const bool isA = s < IBD_TILE;
    const int pos = (isA ? ta : tb) * IBD_TILE + (s & (IBD_TILE - 1));      // position in the list
    const RangeRow rr = range_row(xp, ld, isA ? idxA : idxB, pos, isA ? ba : bb);      // (a row past the list: every call missing)
    const float* qrow = (isA ? QA : QB) + (int64_t)rr.posc * q_stride;
    float q[KP];
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(qrow + k);
        q[k] = v.x; q[k + 1] = v.y; q[k + 2] = v.z; q[k + 3] = v.w;
    }
    const float opf = 1.f + (isA ? fA : fB)[rr.posc];             // 1 + f of the sample (any value: a masked call is cleared by bits)
    const int sh = 16 * g0;

    f32x4_t accN[4], accD[4], accX[4], accI[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) accN[i] = accD[i] = accX[i] = accI[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    auto load_chunk = [&](const int64_t c, u32x4_t (&xv)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = range_piece(rr.x, c, i, ld);
    };
    u32x4_t nxt[4];
    load_chunk(c_lo, nxt);

#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        uint32_t cw[16];                                          // the chunk's 16 dwords; every step consumes the first two
#pragma unroll
        for (int i = 0; i < 16; ++i) cw[i] = nxt[i >> 2][i & 3];
        // the chunk's P rows (a row >= M reads row M - 1; its SNP is masked below).  The previous chunk's last step ended with a barrier
#pragma unroll
        for (int v = 0; v < KP / 4; ++v) {
            const int e = t + 256 * v;
            const int64_t j = min(c * IBD_CHUNK + e / (KP / 4), M - 1);
            reinterpret_cast<f32x4_t*>(Ps)[e] = *reinterpret_cast<const f32x4_t*>(P + j * KP + 4 * (e % (KP / 4)));
        }
        load_chunk(min(c + 1, c_hi - 1), nxt);
        const int left = (int)min(M - c * IBD_CHUNK, (int64_t)(2 * IBD_CHUNK));       // SNPs < M from the chunk's first on (>= 1)
        __syncthreads();
#pragma unroll 1
        for (int st = 0; st < IBD_CHUNK / IBD_STEP; ++st) {
            // ---- build: the ten operand fragments of two (sample, group) pairs per thread
            u32x4_t fr[2][4];                                     // u_hi, u_lo, w_hi, w_lo of the two pairs
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int g = g0 + 2 * it;                        // dword `it` of the step holds its groups 2 it and 2 it + 1
                const uint32_t bits = cw[it] >> sh;
                const int jl = st * IBD_STEP + g * 8;             // first SNP of the group within the chunk
                const int rem = left - jl;                        // element e of the group is a SNP < M iff e < rem
                float pi[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) pi[e] = 0.f;
#pragma unroll
                for (int k = 0; k < KP; k += 4) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float4 p4 = *reinterpret_cast<const float4*>(&Ps[(jl + e) * KP + k]);       // a broadcast
                        pi[e] = fmaf(q[k], p4.x, pi[e]); pi[e] = fmaf(q[k + 1], p4.y, pi[e]);
                        pi[e] = fmaf(q[k + 2], p4.z, pi[e]); pi[e] = fmaf(q[k + 3], p4.w, pi[e]);
                    }
                }
                float ev[8], vv[8], uv[8], wv[8];
                uint32_t m0[8], m2[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t code = (bits >> (2 * e)) & 3u;
                    uint32_t m = obs_mask(code);
                    m &= rr.valid & lt_mask(e, rem) & ge0_mask(pi[e] - pimin) & ge0_mask(one_m_pimin - pi[e]);
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
                u32x4_t eh, el, vh, vl, z0, z2;
                ibd_split(ev, eh, el);
                ibd_split(vv, vh, vl);
                ibd_split(uv, fr[it][0], fr[it][1]);
                ibd_split(wv, fr[it][2], fr[it][3]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {                     // bf16 1.0 or 0
                    z0[i] = (m0[2 * i] & 0x3F80u) | (m0[2 * i + 1] & 0x3F800000u);
                    z2[i] = (m2[2 * i] & 0x3F80u) | (m2[2 * i + 1] & 0x3F800000u);
                }
                u32x4_t* o = Img + g * (2 * IBD_TILE) + s;
                o[0 * IBD_SLOT] = eh;
                o[1 * IBD_SLOT] = el;
                o[2 * IBD_SLOT] = vh;
                o[3 * IBD_SLOT] = vl;
                o[4 * IBD_SLOT] = z0;
                o[5 * IBD_SLOT] = z2;
            }
#pragma unroll
            for (int i = 0; i < 14; ++i) cw[i] = cw[i + 2];
            // lane l is row / column l & 15 and group l >> 4 of both operands
            const u32x4_t* ia = Img + (lane >> 4) * (2 * IBD_TILE) + 16 * w + (lane & 15);
            const u32x4_t* ib = Img + (lane >> 4) * (2 * IBD_TILE) + IBD_TILE + (lane & 15);
            __syncthreads();
            // ---- half 1: e.e and vm.vm
            {
                bf16x8_t a[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) a[p] = __builtin_bit_cast(bf16x8_t, ia[p * IBD_SLOT]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf16x8_t b[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) b[p] = __builtin_bit_cast(bf16x8_t, ib[p * IBD_SLOT + 16 * j]);
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], accN[j], 0, 0, 0);      // lo.hi
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], accN[j], 0, 0, 0);      // hi.lo
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], accN[j], 0, 0, 0);      // hi.hi
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[3], b[2], accD[j], 0, 0, 0);
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[3], accD[j], 0, 0, 0);
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[2], accD[j], 0, 0, 0);
                }
            }
            __syncthreads();
            // ---- half 2: u and w over e and vm; u.w + w.u and the two indicator products
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                u32x4_t* o = Img + (g0 + 2 * it) * (2 * IBD_TILE) + s;
#pragma unroll
                for (int p = 0; p < 4; ++p) o[p * IBD_SLOT] = fr[it][p];
            }
            __syncthreads();
            {
                bf16x8_t a[6];                                    // u_hi, u_lo, w_hi, w_lo, z0, z2
#pragma unroll
                for (int p = 0; p < 6; ++p) a[p] = __builtin_bit_cast(bf16x8_t, ia[p * IBD_SLOT]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf16x8_t b[6];
#pragma unroll
                    for (int p = 0; p < 6; ++p) b[p] = __builtin_bit_cast(bf16x8_t, ib[p * IBD_SLOT + 16 * j]);
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[2], accX[j], 0, 0, 0);      // u_a w_b: lo.hi
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[3], b[0], accX[j], 0, 0, 0);      // w_a u_b: lo.hi
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[3], accX[j], 0, 0, 0);      // u_a w_b: hi.lo
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[1], accX[j], 0, 0, 0);      // w_a u_b: hi.lo
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], accX[j], 0, 0, 0);      // u_a w_b: hi.hi
                    accX[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], accX[j], 0, 0, 0);      // w_a u_b: hi.hi
                    accI[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[4], b[5], accI[j], 0, 0, 0);      // z0_a z2_b
                    accI[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[5], b[4], accI[j], 0, 0, 0);      // z2_a z0_b
                }
            }
            __syncthreads();
        }
    }
    // D: column = lane & 15 (B sample 16 j + column), rows 4 (lane >> 4) + i (A sample 16 w + row).  Every block writes its whole slab
    float* out = part + ((int64_t)range * (gridDim.x / ranges) + tile) * (IBD_PLANES * IBD_TILE * IBD_TILE);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (16 * w + 4 * (lane >> 4) + i) * IBD_TILE + 16 * j + (lane & 15);
            out[o] = accN[j][i];
            out[IBD_TILE * IBD_TILE + o] = accD[j][i];
            out[2 * IBD_TILE * IBD_TILE + o] = accI[j][i];
            out[3 * IBD_TILE * IBD_TILE + o] = accX[j][i];
        }
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
static bool ibd_shape_ok(int ba, int bb, int64_t M) { return ba > 0 && bb > 0 && ba <= NADM_IBD_MAX_ROWS && bb <= NADM_IBD_MAX_ROWS && M > 0; }

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
    if (ba <= 0 || bb <= 0 || M <= 0) return failf(who, "empty block (need ba > 0, bb > 0 and M > 0)");
    if (ba > NADM_IBD_MAX_ROWS || bb > NADM_IBD_MAX_ROWS) return failf(who, "ba and bb must be <= NADM_IBD_MAX_ROWS");
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
