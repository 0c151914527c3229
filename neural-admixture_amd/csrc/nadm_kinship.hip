// Admixture-aware kinship (REAP, Thornton et al. 2012) of one block of sample pairs from the packed matrix, Q and one head's P
// (include/nadm.h, nadm_kinship): two Gram products over the SNP axis and a count, on v_mfma_f32_16x16x32_bf16.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   kinship_accum_kernel  one 256-thread block per (64 x 64 tile of A samples x B samples, range of 256-SNP chunks).  Per chunk the
//                         block stages the chunk's P rows in LDS and every thread keeps its sample's 64 packed bytes in registers
//                         (the next chunk's are loaded under the current chunk's work).  A chunk is worked off in eight steps of 32
//                         SNPs = one K of the instruction.  BUILD: thread t owns sample t & 127 of the 128 (64 A then 64 B) and two
//                         of the step's four 8-SNP groups; the group is the same in all lanes of a wave, so the P rows are LDS
//                         broadcasts.  It decodes, forms pi (fp32, k in order), the mask m, d = m (g - 2 pi) and s = m sqrt(pi (1 -
//                         pi)), splits d and s into two RNE bf16 pieces each and writes the five 16-byte operand fragments (d_hi,
//                         d_lo, s_hi, s_lo, m) of (sample, group) -- exactly what one lane of the instruction takes -- into the LDS
//                         image [piece][group][sample]: consecutive lanes write and read consecutive 16 bytes.  MULTIPLY: wave w owns
//                         A rows 16 w .. 16 w + 15 against the four 16-sample B tiles: 7 instructions per tile (hi.hi + hi.lo + lo.hi
//                         for num and for den, one for n) into fp32 accumulators that live for the whole range.  The operand image
//                         never leaves LDS.  Missing calls, SNPs >= M, rows past the list and masked pi enter as exactly +0.0f.
//   pair_fold_kernel      (with KinshipSum) one thread per pair: the ranges' partials in range order in float64; n as int32.
// The chunk split, the row lookup, the clamped piece load and the fold are those of nadm_chunk_ranges.h.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int KIN_CHUNK = RANGE_CHUNK;
constexpr int KIN_TILE = PAIR_TILE;       // samples per tile side
constexpr int KIN_STEP = 32;              // SNPs per build / multiply step = K of the instruction
constexpr int KIN_MAX_CHUNKS = 1024;      // chunks per range at most: no fp32 accumulator covers more than 2^18 SNPs (n exact: < 2^24)
constexpr int64_t KIN_BLOCKS = 512;       // blocks wanted at least (256 CUs x 2 blocks of 4 waves), while there are chunks to split
constexpr int KIN_PIECES = 5;             // d_hi, d_lo, s_hi, s_lo, m

template <int KP>
__global__ __launch_bounds__(256, KP <= 16 ? 2 : 1) void kinship_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idxA, const int ba, const int32_t* __restrict__ idxB,
    const int bb, const int64_t M, const float* __restrict__ P, const float* __restrict__ QA, const float* __restrict__ QB,
    const int q_stride, const float pimin, const float one_m_pimin, const int tiles_b, const int ranges, const int chunks_per_range,
    const int64_t chunks, float* __restrict__ part) {
    constexpr bool WIDE = KP > 16;                                // wide heads: Q is re-read (L1 / L2) four columns at a time
    __shared__ __attribute__((aligned(16))) float Ps[KIN_CHUNK * KP];
    __shared__ __attribute__((aligned(16))) u32x4_t Img[KIN_PIECES * 4 * 2 * KIN_TILE];       // [piece][group][sample 0..127]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = (int)blockIdx.x / ranges, range = (int)blockIdx.x - tile * ranges;
    const int ta = tile / tiles_b, tb = tile - ta * tiles_b;
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);

    // builder role: sample s of the 128 (A rows of the tile, then B rows), groups g0 and g0 + 2 of every step
    const int s = t & 127, g0 = t >> 7;
    const bool isA = s < KIN_TILE;
    const int pos = (isA ? ta : tb) * KIN_TILE + (s & (KIN_TILE - 1));      // position in the list
    const RangeRow rr = range_row(xp, ld, isA ? idxA : idxB, pos, isA ? ba : bb);      // (a row past the list: every call missing)
    const float* qrow = (isA ? QA : QB) + (int64_t)rr.posc * q_stride;
    float q[WIDE ? 4 : KP];
    if constexpr (!WIDE) {
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(qrow + k);
            q[k] = v.x; q[k + 1] = v.y; q[k + 2] = v.z; q[k + 3] = v.w;
        }
    }
    const int sh = 16 * g0;

    f32x4_t accN[4], accD[4], accC[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) accN[i] = accD[i] = accC[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

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
            const int64_t j = min(c * KIN_CHUNK + e / (KP / 4), M - 1);
            reinterpret_cast<f32x4_t*>(Ps)[e] = *reinterpret_cast<const f32x4_t*>(P + j * KP + 4 * (e % (KP / 4)));
        }
        load_chunk(min(c + 1, c_hi - 1), nxt);
        const int left = (int)min(M - c * KIN_CHUNK, (int64_t)(2 * KIN_CHUNK));       // SNPs < M from the chunk's first on (>= 1)
        __syncthreads();
#pragma unroll 1
        for (int st = 0; st < KIN_CHUNK / KIN_STEP; ++st) {
            // ---- build: two (sample, group) operand fragments per thread
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int g = g0 + 2 * it;                        // dword `it` of the step holds its groups 2 it and 2 it + 1
                const uint32_t bits = cw[it] >> sh;
                const int jl = st * KIN_STEP + g * 8;             // first SNP of the group within the chunk
                const int rem = left - jl;                        // element e of the group is a SNP < M iff e < rem
                float pi[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) pi[e] = 0.f;
#pragma unroll
                for (int k = 0; k < KP; k += 4) {
                    if constexpr (WIDE) {
                        const float4 v = *reinterpret_cast<const float4*>(qrow + k);
                        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float4 p4 = *reinterpret_cast<const float4*>(&Ps[(jl + e) * KP + k]);       // a broadcast
                        const int kq = WIDE ? 0 : k;
                        pi[e] = fmaf(q[kq], p4.x, pi[e]); pi[e] = fmaf(q[kq + 1], p4.y, pi[e]);
                        pi[e] = fmaf(q[kq + 2], p4.z, pi[e]); pi[e] = fmaf(q[kq + 3], p4.w, pi[e]);
                    }
                }
                float dv[8], sv[8];
                uint32_t mv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t code = (bits >> (2 * e)) & 3u;
                    uint32_t m = obs_mask(code);
                    m &= rr.valid & lt_mask(e, rem) & ge0_mask(pi[e] - pimin) & ge0_mask(one_m_pimin - pi[e]);
                    mv[e] = m;
                    dv[e] = keepf((float)code - 2.f * pi[e], m);
                    sv[e] = keepf(__builtin_amdgcn_sqrtf(fmaxf(pi[e] * (1.f - pi[e]), 0.f)), m);
                }
                u32x4_t dh, dl, shi, slo, mm;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dh[i] = pk_bf16(dv[2 * i], dv[2 * i + 1]);
                    dl[i] = pk_bf16(dv[2 * i] - __uint_as_float(dh[i] << 16), dv[2 * i + 1] - __uint_as_float(dh[i] & 0xFFFF0000u));
                    shi[i] = pk_bf16(sv[2 * i], sv[2 * i + 1]);
                    slo[i] = pk_bf16(sv[2 * i] - __uint_as_float(shi[i] << 16), sv[2 * i + 1] - __uint_as_float(shi[i] & 0xFFFF0000u));
                    mm[i] = (mv[2 * i] & 0x3F80u) | (mv[2 * i + 1] & 0x3F800000u);            // bf16 1.0 or 0
                }
                u32x4_t* o = Img + g * (2 * KIN_TILE) + s;
                o[0 * 4 * 2 * KIN_TILE] = dh;
                o[1 * 4 * 2 * KIN_TILE] = dl;
                o[2 * 4 * 2 * KIN_TILE] = shi;
                o[3 * 4 * 2 * KIN_TILE] = slo;
                o[4 * 4 * 2 * KIN_TILE] = mm;
            }
#pragma unroll
            for (int i = 0; i < 14; ++i) cw[i] = cw[i + 2];
            __syncthreads();
            // ---- multiply: lane l is row / column l & 15 and group l >> 4 of both operands
            {
                const u32x4_t* ia = Img + (lane >> 4) * (2 * KIN_TILE) + 16 * w + (lane & 15);
                bf16x8_t a[KIN_PIECES];
#pragma unroll
                for (int p = 0; p < KIN_PIECES; ++p) a[p] = __builtin_bit_cast(bf16x8_t, ia[p * 4 * 2 * KIN_TILE]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x4_t* ib = Img + (lane >> 4) * (2 * KIN_TILE) + KIN_TILE + 16 * j + (lane & 15);
                    bf16x8_t b[KIN_PIECES];
#pragma unroll
                    for (int p = 0; p < KIN_PIECES; ++p) b[p] = __builtin_bit_cast(bf16x8_t, ib[p * 4 * 2 * KIN_TILE]);
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], accN[j], 0, 0, 0);      // lo.hi
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], accN[j], 0, 0, 0);      // hi.lo
                    accN[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], accN[j], 0, 0, 0);      // hi.hi
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[3], b[2], accD[j], 0, 0, 0);
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[3], accD[j], 0, 0, 0);
                    accD[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[2], accD[j], 0, 0, 0);
                    accC[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[4], b[4], accC[j], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }
    // D: column = lane & 15 (B sample 16 j + column), rows 4 (lane >> 4) + i (A sample 16 w + row).  Every block writes its whole slab
    float* out = part + ((int64_t)range * (gridDim.x / ranges) + tile) * (3 * KIN_TILE * KIN_TILE);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (16 * w + 4 * (lane >> 4) + i) * KIN_TILE + 16 * j + (lane & 15);
            out[o] = accN[j][i];
            out[KIN_TILE * KIN_TILE + o] = accD[j][i];
            out[2 * KIN_TILE * KIN_TILE + o] = accC[j][i];
        }
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
static bool kin_shape_ok(int ba, int bb, int64_t M) {
    return ba > 0 && bb > 0 && ba <= NADM_KINSHIP_MAX_ROWS && bb <= NADM_KINSHIP_MAX_ROWS && M > 0;
}

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
    if (ba <= 0 || bb <= 0 || M <= 0) return fail("nadm_kinship: empty block (need ba > 0, bb > 0 and M > 0)");
    if (ba > NADM_KINSHIP_MAX_ROWS || bb > NADM_KINSHIP_MAX_ROWS) return fail("nadm_kinship: ba and bb must be <= NADM_KINSHIP_MAX_ROWS");
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
