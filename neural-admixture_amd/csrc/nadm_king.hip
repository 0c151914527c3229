// KING-robust kinship counts (Manichaikul et al. 2010) of one block of sample pairs from the packed matrix alone (include/nadm.h,
// nadm_king): five integer counts per pair, summed over the SNP axis on v_mfma_i32_16x16x64_i8 with int32 accumulators.  Exact.
//
// Two launches per call, no atomics, no floating point:
//   king_accum_kernel  one 256-thread block per (64 x 64 tile of A samples x B samples, range of 256-SNP chunks: the scaffolding of
//                      nadm_chunk_ranges.h, as nadm_kinship uses it).  Wave w owns the 32 x 32 quarter (w >> 1, w & 1) of
//                      the tile: two 16-sample A tiles against two 16-sample B tiles.  The matrix is sample-major and the SNP axis
//                      is the instruction's k, so nothing is transposed: lane l is sample l & 15 of each of its four 16-sample
//                      tiles and k-group q = l >> 4 of the instruction, for the A and for the B operand alike (the lane -> (row, k)
//                      rule of nadm_ld.hip's header; D: column = lane & 15 = B sample, rows 4 (lane >> 4) + i = A sample).
//                      LOAD    per chunk a lane loads ONE 16-byte piece per sample: bytes 16 q .. 16 q + 15 of the chunk's 64 (the
//                              next chunk's under the current chunk's work).  A wave's load covers 16 rows x 64 contiguous bytes.
//                      STEP    a chunk is four steps of 64 SNPs = one K of the instruction.  In step s a lane's operand is dword s
//                              of its piece: the 16 consecutive SNPs 64 q + 16 s .. + 15 of its own sample's row.  (Deviation from
//                              "step s = SNPs 64 s .. 64 s + 63": a step here is the SNPs {64 q + 16 s + e}.  The instruction sums
//                              over k and both operands follow the same rule, so which 64 SNPs of the chunk share a step does not
//                              matter; one dwordx4 load per sample and chunk replaces four dword loads.)
//                      EXPAND  the dword x -> bit-planes lo = x & 0x5555.., hi = (x >> 1) & 0x5555.. -> the four indicator planes
//                              h = lo & ~hi (code 1), z2 = hi & ~lo, o = ~(lo & hi), z0 = ~(lo | hi), one bit per 2-bit field; plane
//                              p -> operand dword i = (p >> 2 i) & 0x01010101: byte b of dword i is field 4 b + i.  (The same
//                              permutation of k on both sides.)  No per-field loop: 9 + 4 x 7 bit operations per sample and step.
//                      MULTIPLY six products per 16 x 16 tile and step into five accumulators: o.o (n), h.h (hethet), z0.z2 + z2.z0
//                              (ibs0), h.o (het_a), o.h (het_b): 24 instructions per wave and step, i32x4 accumulators that live for
//                              the whole range.
//                      B fragments are REBUILT IN REGISTERS by every wave, there is no LDS image and no barrier: an image as in
//                      nadm_kinship would be read back as 4 pieces x 16 bytes per lane, sample and step (16 KB per wave and step
//                      through the LDS port all four waves share) to save ~37 bit operations per sample and step that run on the
//                      wave's own SIMD beside its 24 matrix instructions; with the 2 x 2 tile layout a wave expands four samples
//                      per step instead of the five of a 1 x 4 layout.
//                      SNPs >= M, the pad fields of a row's last byte, the bytes behind it and rows past the list are overwritten
//                      with the missing code (all ones) BEFORE the expansion: they contribute exactly 0 to every count.
//   pair_fold_kernel   (nadm_chunk_ranges.h, with KingSum) one thread per pair: the ranges' int32 partials in range order.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int KING_CHUNK = RANGE_CHUNK;
constexpr int KING_TILE = PAIR_TILE;             // samples per tile side
constexpr int64_t KING_MAX_CHUNKS = 1ll << 23;   // chunks per range at most: an int32 count covers 2^31 SNPs
constexpr int64_t KING_BLOCKS = 512;             // blocks wanted at least, while there are chunks to split (as nadm_kinship)
constexpr int KING_COUNTS = 5;                   // n, hethet, ibs0, het_a, het_b
constexpr int KING_SLAB = KING_COUNTS * KING_TILE * KING_TILE;

struct KingFrag {
    i32x4_t h, z0, z2, o;
};

// the 16 fields of x (one bit per field at the even positions of a plane) -> 16 int8 of 0 / 1: dword i holds the fields i, 4 + i, 8 + i, 12 + i
__device__ __forceinline__ i32x4_t king_spread(const uint32_t plane) {
    return (i32x4_t){(int)(plane & 0x01010101u), (int)((plane >> 2) & 0x01010101u), (int)((plane >> 4) & 0x01010101u),
                     (int)((plane >> 6) & 0x01010101u)};
}
__device__ __forceinline__ KingFrag king_expand(const uint32_t x) {
    const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
    KingFrag f;
    f.h = king_spread(lo & ~hi);
    f.z2 = king_spread(hi & ~lo);
    f.o = king_spread((lo & hi) ^ 0x55555555u);
    f.z0 = king_spread((lo | hi) ^ 0x55555555u);
    return f;
}

__global__ __launch_bounds__(256, 2) void king_accum_kernel(const uint8_t* __restrict__ xp, const int64_t ld,
                                                            const int32_t* __restrict__ idxA, const int ba,
                                                            const int32_t* __restrict__ idxB, const int bb, const int64_t M,
                                                            const int tiles_b, const int ranges, const int64_t chunks_per_range,
                                                            const int64_t chunks, int32_t* __restrict__ part) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int tile = (int)blockIdx.x / ranges, range = (int)blockIdx.x - tile * ranges;
    const int ta = tile / tiles_b, tb = tile - ta * tiles_b;
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);

    // the lane's four samples: A tiles 0, 1 then B tiles 0, 1 of the wave's quarter
    const uint8_t* xrow[4];
    uint32_t gone[4];                                             // a row past the list: every call missing
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool isA = i < 2;
        const int pos = (isA ? ta : tb) * KING_TILE + 32 * (isA ? (w >> 1) : (w & 1)) + 16 * (i & 1) + r;
        const RangeRow rr = range_row(xp, ld, isA ? idxA : idxB, pos, isA ? ba : bb);
        xrow[i] = rr.x;
        gone[i] = ~rr.valid;
    }
    // (a clamped piece holds SNPs >= M only: every field of it is overwritten below)
    auto load_chunk = [&](const int64_t c, u32x4_t (&xv)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = range_piece(xrow[i], c, q, ld);
    };

    i32x4_t acc[2][2][KING_COUNTS];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < KING_COUNTS; ++k) acc[i][j][k] = (i32x4_t){0, 0, 0, 0};

    u32x4_t nxt[4];
    load_chunk(c_lo, nxt);
#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        u32x4_t cur[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i] | gone[i];
        load_chunk(min(c + 1, c_hi - 1), nxt);
        const int64_t left = M - (c * KING_CHUNK + 64 * q);       // SNPs < M from the piece's first on (may be <= 0)
        if (c * KING_CHUNK + KING_CHUNK > M) {                    // the last chunk of the matrix (the same in every lane)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t l = left - 16 * s;                  // ones in the fields of SNPs >= M
                const uint32_t tail = l >= 16 ? 0u : (l <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (2 * (int)l));
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[i][s] |= tail;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const KingFrag a0 = king_expand(cur[0][s]), a1 = king_expand(cur[1][s]);
            const KingFrag b0 = king_expand(cur[2][s]), b1 = king_expand(cur[3][s]);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const KingFrag& a = i ? a1 : a0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const KingFrag& b = j ? b1 : b0;
                    acc[i][j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.o, b.o, acc[i][j][0], 0, 0, 0);        // n
                    acc[i][j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.h, b.h, acc[i][j][1], 0, 0, 0);        // hethet
                    acc[i][j][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.z0, b.z2, acc[i][j][2], 0, 0, 0);      // ibs0
                    acc[i][j][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.z2, b.z0, acc[i][j][2], 0, 0, 0);
                    acc[i][j][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.h, b.o, acc[i][j][3], 0, 0, 0);        // het_a
                    acc[i][j][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.o, b.h, acc[i][j][4], 0, 0, 0);        // het_b
                }
            }
        }
    }
    // D: column = lane & 15 (B sample), rows 4 (lane >> 4) + e (A sample).  Every block writes its whole slab [count][64][64]
    int32_t* out = part + ((int64_t)range * (gridDim.x / ranges) + tile) * KING_SLAB;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = (32 * (w >> 1) + 16 * i + 4 * q + e) * KING_TILE + 32 * (w & 1) + 16 * j + r;
#pragma unroll
                for (int k = 0; k < KING_COUNTS; ++k) out[k * KING_TILE * KING_TILE + o] = acc[i][j][k][e];
            }
}

// pair_fold_kernel's sums: the five counts, int32
struct KingSum {
    using Out = int32_t*;
    Out counts;
    int s[KING_COUNTS] = {};
    __device__ __forceinline__ void add(const int plane, const int32_t v) { s[plane] += v; }
    __device__ __forceinline__ void store(const int64_t e, const int64_t pairs) const {
#pragma unroll
        for (int k = 0; k < KING_COUNTS; ++k) counts[k * pairs + e] = s[k];
    }
};

// the launch shape, a rule of (ba, bb, M) alone
static RangePlan king_plan(int ba, int bb, int64_t M) { return range_plan(M, range_tiles(ba, KING_TILE, bb, KING_TILE), KING_BLOCKS, KING_MAX_CHUNKS); }
static bool king_shape_ok(int ba, int bb, int64_t M) { return pair_block_ok(ba, bb, M, NADM_KING_MAX_ROWS) && M < (1ll << 31); }

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_king_ranges(int32_t ba, int32_t bb, int64_t M) { return king_shape_ok(ba, bb, M) ? range_count(king_plan(ba, bb, M).ranges) : 0; }

// scratch: [ranges][tiles][n | hethet | ibs0 | het_a | het_b][64 x 64] int32
extern "C" int64_t nadm_king_scratch_ints(int32_t ba, int32_t bb, int64_t M) {
    return king_shape_ok(ba, bb, M) ? king_plan(ba, bb, M).blocks_bound * KING_SLAB : 0;
}

extern "C" int nadm_king(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                         int32_t* counts, int32_t* scratch, void* stream) {
    if (!xp || !counts || !scratch) return fail("nadm_king: null pointer");
    if (check_pair_block("nadm_king", ba, bb, M, PAIR_MAX_ROWS(NADM_KING_MAX_ROWS))) return 1;
    if (M >= (1ll << 31)) return fail("nadm_king: M must be < 2^31 (the counts are int32)");
    if (check_packed("nadm_king", ld, M)) return 1;
    if ((((uintptr_t)xp | (uintptr_t)scratch) & 15) != 0) return fail("nadm_king: xp and scratch must be 16-byte aligned");
    if ((((uintptr_t)idxA | (uintptr_t)idxB | (uintptr_t)counts) & 3) != 0)
        return fail("nadm_king: idxA, idxB and counts must be 4-byte aligned");
    const RangePlan pl = king_plan(ba, bb, M);
    if (range_launch_check("nadm_king", pl)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(king_accum_kernel, range_grid(pl), dim3(256), 0, st, xp, ld, idxA, ba, idxB, bb, M, (bb + KING_TILE - 1) / KING_TILE,
                       (int)pl.ranges, pl.cpr, pl.chunks, scratch);
    if (int e = check_launch("king (accumulate)")) return e;
    launch_pair_fold<int32_t, KING_COUNTS, KingSum>(scratch, pl, ba, bb, counts, st);
    return check_launch("king (fold)");
}
