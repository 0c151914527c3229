// The chunk-range scaffolding shared by the kernels that work a block of sample rows over the SNP axis of the packed matrix: the
// counterpart of nadm_snp_sweep.h for the kernels that own samples, not SNPs.
//
// One 256-thread block per (tile of the block's rows, range of consecutive 256-SNP chunks).  The block keeps its running sums in
// registers for the whole range and writes its slab of partials once; a second launch folds the ranges' slabs in range order (no
// floating-point atomics: the same inputs give the same bits).  The chunk axis is cut by the split rule of nadm_host_rules.h, a rule
// of the shape alone: as many ranges as it takes to put BLOCKS blocks on the chip given the tile count, while there are chunks to
// split, and never more than MAX_CHUNKS chunks in one range (what one running sum may cover).
//
// Every unit supplies its tile count, BLOCKS and MAX_CHUNKS (-> range_plan), its blockIdx -> (tile, range) order (which decides the
// blocks that share L2 lines: range fastest in kinship, ibd and king, tile fastest in sample_info, resid_project and obs_project, group
// fastest in resid_cor) and its slab layout.  Between the prologue and the slab store there are two shared walks:
//
//   sample_walk   a lane per sample, 256 rows per tile (sample_info_accum_kernel in nadm_sample_info.hip).  The walk holds the row's 16
//                 packed words with the next chunk's in flight, stages the chunk's P rows in LDS (zeros past M), keeps the two barriers
//                 and the skip of a wave without rows, and hands every call to the body as a code: missing, SNP >= M and row past the
//                 list all arrive as code 3.  A kernel is its prologue (range_row, load_row of q, its sums zeroed), the walk with its
//                 arithmetic for one genotype as the body (dot_row for pi), and its slab store.
//   PairBuilder   64 x 64 tiles of sample pairs on the matrix pipe (kinship_accum_kernel in nadm_kinship.hip, ibd_accum_kernel in
//                 nadm_ibd.hip).  Thread t builds the operand fragments of sample t & 127 of the 128 (A rows, then B rows) for two of
//                 the four 8-SNP groups of every 32-SNP step.  The builder holds the row, its q, the chunk's 16 words with the next
//                 chunk's in flight and the chunk's P rows in LDS (clamped to M - 1), and gives the eight pi of a group and the mask
//                 of a call.  A kernel supplies its operands, its LDS image and barriers within a step, its multiplies (split8, ones8,
//                 mfma_split) and the Sum of its fold; pair_slab_store and pair_fold_kernel are shared.
//
// king_accum_kernel (nadm_king.hip: fragments rebuilt in registers, no P) and obs_project_kernel (nadm_obs_project.hip) use the plan,
// range_row and range_piece alone; resid_cor_accum_kernel (nadm_resid_cor.hip), which skips what the others clamp, keeps its own loads;
// project_accum_kernel (nadm_project.hip: one wave per (chunk, tile), no ranges) takes dot_row and chunk_word.  resid_project_kernel
// (nadm_resid_project.hip) is the walk's loop written out, on the same pieces (load_row, stage_rows, chunk_word, dot_row): as the walk's
// body, with W staged and the chunk's sum of squares closed through hooks, the compiler issued the W reads of the hot loop one at a
// time, each behind a wait, and the forward product took 117 ms where it takes 90 (profiles/range_walks.txt).  The
// [ranges][tiles][PLANES][64 x 64] slabs of kinship, ibd and king share pair_fold_kernel; the others keep folds of their own: index
// arithmetic is all there is to them.
#pragma once
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int RANGE_CHUNK = 256;         // SNPs per chunk = 64 bytes of a packed row
constexpr int PAIR_TILE = 64;            // samples per side of a tile of pair_fold_kernel's slabs

// ---- host: the launch shape
struct RangePlan {
    int64_t chunks, tiles, cpr, ranges;  // 256-SNP chunks of M, tiles of rows, chunks per range, ranges = ceil(chunks / cpr)
    int64_t blocks_bound;                // a bound of ranges x tiles that grows with M and with the tiles: sizes the partials
};
inline int64_t range_tiles(int ba, int rows_a, int bb = 1, int rows_b = 1) {
    return (int64_t)((ba + rows_a - 1) / rows_a) * ((bb + rows_b - 1) / rows_b);
}
inline RangePlan range_plan(int64_t M, int64_t tiles, int64_t want_blocks, int64_t max_chunks) {
    const int64_t chunks = (M + RANGE_CHUNK - 1) / RANGE_CHUNK, cpr = split_per_part(chunks, tiles, want_blocks, max_chunks);
    return {chunks, tiles, cpr, (chunks + cpr - 1) / cpr, split_blocks_bound(chunks, tiles, want_blocks, max_chunks)};
}
// what a *_ranges / *_chunks query returns: the count, 0 where it does not fit the launch
inline int32_t range_count(int64_t n) { return n > 0x7FFFFFFFll ? 0 : (int32_t)n; }
// the grid (tiles x ranges) and the kernels' int arguments must fit; range_grid is the accumulate launch's grid once they do
inline int range_launch_check(const char* who, const RangePlan& p) {
    return (p.tiles * p.ranges > 0x7FFFFFFFll || p.cpr > 0x7FFFFFFFll) ? failf(who, "too many blocks for one launch") : 0;
}
inline dim3 range_grid(const RangePlan& p) { return dim3((unsigned)(p.tiles * p.ranges)); }
inline dim3 fold_grid(int64_t outputs) { return dim3((unsigned)((outputs + 255) / 256)); }       // one thread per output

// ---- device
struct ChunkRange { int64_t lo, hi; };
__device__ __forceinline__ ChunkRange chunk_range(const int range, const int64_t cpr, const int64_t chunks) {
    const int64_t lo = (int64_t)range * cpr;                      // < chunks: ranges = ceil(chunks / cpr)
    return {lo, min(lo + cpr, chunks)};
}
// position `pos` of a list of nb rows (idx: the gather list, or none) -> the row's packed bytes, pos < nb ? 0xFFFFFFFF : 0, and
// min(pos, nb - 1): a position past the list reads the list's last row, and the kernel turns every call of it into a missing one
struct RangeRow { const uint8_t* x; uint32_t valid; int posc; };
__device__ __forceinline__ RangeRow range_row(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                              const int pos, const int nb) {
    const uint32_t valid = lt_mask(pos, nb);
    const int posc = min(pos, nb - 1);
    const int64_t row = idx ? idx[posc] : posc;
    return {xp + row * ld, valid, posc};
}
// 16-byte piece `piece` (0..3) of chunk c of a row.  A piece past the row's end holds SNPs >= M only (4 ld >= M, and ld is a multiple
// of 16): its offset is clamped to the row's last piece and the load is unconditional; the kernel masks SNPs >= M anyway
__device__ __forceinline__ u32x4_t range_piece(const uint8_t* xrow, const int64_t c, const int piece, const int64_t ld) {
    return *reinterpret_cast<const u32x4_t*>(xrow + min(c * (RANGE_CHUNK / 4) + 16 * piece, ld - 16));
}

// ---- device: rows of fp32 in registers and LDS
// a row of KP floats (16-byte aligned) into registers, four columns per load
template <int KP>
__device__ __forceinline__ void load_row(const float* row, float (&v)[KP]) {
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(row + k);
        v[k] = t4.x; v[k + 1] = t4.y; v[k + 2] = t4.z; v[k + 3] = t4.w;
    }
}
// pi = q . row as multiply-adds with k ascending from +0.0f (the order the float64 tests rest on); the row is read once, four columns
// at a time (in LDS, the same address in every lane: a broadcast), and stays in p for the caller that goes on with it
template <int KP>
__device__ __forceinline__ float dot_row(const float (&q)[KP], const float* row, float (&p)[KP]) {
    load_row<KP>(row, p);
    float pi = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) pi = fmaf(q[k], p[k], pi);
    return pi;
}
template <int KP>
__device__ __forceinline__ float dot_row(const float (&q)[KP], const float* row) {
    float p[KP];
    return dot_row<KP>(q, row, p);
}
// rows j0 .. j0 + ROWS - 1 of an [M][W] matrix into LDS (rows >= M as zeros: never read from memory), float4 by float4, coalesced
template <int ROWS, int W, int THREADS>
__device__ __forceinline__ void stage_rows(const float* __restrict__ A, const int64_t j0, const int64_t M, float* S) {
    const float4* src = reinterpret_cast<const float4*>(A + j0 * W);
    const int64_t lim = (M - j0) * (W / 4);                       // float4 of the rows that exist
#pragma unroll
    for (int e = threadIdx.x; e < ROWS * W / 4; e += THREADS)
        reinterpret_cast<float4*>(S)[e] = e < lim ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
}
// word wi (16 SNPs) of a chunk's 16 packed words, `left` = M - (the word's first SNP).  (w stays in registers: no dynamic index.)
// SNPs >= M become code 3 here, once per word (wave-uniform): with them the pad bits of the row's last byte and what lies behind
__device__ __forceinline__ uint32_t chunk_word(const uint32_t (&w)[16], const int wi, const int64_t left) {
    uint32_t bits = w[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
        const uint32_t wv = w[i];                                 // read whatever wi is: a select, never a branch around a load
        bits = (wi == i) ? wv : bits;
    }
    if (left < 16) bits |= left <= 0 ? 0xFFFFFFFFu : (0xFFFFFFFFu << (2 * (int)left));
    return bits;
}

// ---- device: the lane-per-sample walk.  Calls body(code, s) once per SNP s = 0 .. 255 of every chunk of the range, in order, for the
// lane's row rr: code is the 2-bit call, 3 where it is missing, the SNP is >= M or the row is past the list (nothing to add).  The P rows
// of the chunk are in Ps ([256][KP], zeros past M) while the body runs, the same for every lane.  A wave with no row of the list
// (wave_live false, wave-uniform) stages and waits with the block and skips the body.  THREADS = the block's thread count
template <int KP, int THREADS, class Body>
__device__ __forceinline__ void sample_walk(const RangeRow rr, const bool wave_live, const ChunkRange cr, const int64_t ld, const int64_t M,
                                            const float* __restrict__ P, float* Ps, Body&& body) {
    const uint32_t inval = ~rr.valid;                             // a row past the list: every call missing
    u32x4_t nxt[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cr.lo, v, ld);
#pragma unroll 1
    for (int64_t c = cr.lo; c < cr.hi; ++c) {
        const int64_t j0 = c * RANGE_CHUNK;
        if (c > cr.lo) __syncthreads();                           // the previous chunk's rows have been read
        stage_rows<RANGE_CHUNK, KP, THREADS>(P, j0, M, Ps);
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = nxt[i >> 2][i & 3] | inval;
        {
            const int64_t cn = min(c + 1, cr.hi - 1);             // the next chunk's words, in flight under this chunk's arithmetic
#pragma unroll
            for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cn, v, ld);
        }
        __syncthreads();
        if (!wave_live) continue;
#pragma unroll 1
        for (int wi = 0; wi < 16; ++wi) {                         // one 32-bit word = 16 SNPs
            const uint32_t bits = chunk_word(w, wi, M - (j0 + 16 * wi));
#pragma unroll 4
            for (int e = 0; e < 16; ++e) body((bits >> (2 * e)) & 3u, wi * 16 + e);
        }
    }
}

// ---- device: the operand builder of the 64 x 64 pair tiles.  A chunk is worked off in PAIR_STEPS steps of 32 SNPs = one K of
// v_mfma_f32_16x16x32_bf16; a step's four 8-SNP groups are the four 16-byte fragments a lane quartet of the instruction takes
constexpr int PAIR_STEP = 32, PAIR_STEPS = RANGE_CHUNK / PAIR_STEP;
// eight fp32 values -> their round-to-nearest bf16 pieces hi and lo = rne(v - hi), element e in half e & 1 of dword e >> 1
__device__ __forceinline__ void split8(const float (&v)[8], u32x4_t& hi, u32x4_t& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
        lo[i] = pk_bf16(v[2 * i] - __uint_as_float(hi[i] << 16), v[2 * i + 1] - __uint_as_float(hi[i] & 0xFFFF0000u));
    }
}
// eight masks (all ones or zero) -> bf16 1.0 or 0, laid out as split8's pieces
__device__ __forceinline__ u32x4_t ones8(const uint32_t (&m)[8]) {
    u32x4_t z;
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (m[2 * i] & 0x3F80u) | (m[2 * i + 1] & 0x3F800000u);
    return z;
}
__device__ __forceinline__ bf16x8_t frag(const u32x4_t v) { return __builtin_bit_cast(bf16x8_t, v); }
// acc += a b with both operands split: lo.hi, hi.lo, hi.hi, in this order (lo.lo is below the fp32 accumulator's last bit)
__device__ __forceinline__ f32x4_t mfma_split(f32x4_t acc, const bf16x8_t a_hi, const bf16x8_t a_lo, const bf16x8_t b_hi, const bf16x8_t b_lo) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi, acc, 0, 0, 0);
}

// one (sample, group) of a step: the group's 16 bits of the row, its first SNP within the chunk, and rem: element e is a SNP < M iff e < rem
struct PairGroup { int g; uint32_t bits; int jl, rem; };

// The builder role of thread t = threadIdx.x of a 256-thread block on tile (ta, tb): sample s = t & 127 of the 128 (the tile's A rows,
// then its B rows; a row past the list: every call masked), groups g0 and g0 + 2 of every step.  KP <= 16 keeps the q row in
// registers; wider heads (WIDE) re-read it (L1 / L2) four columns at a time
template <int KP, bool WIDE = (KP > 16)>
struct PairBuilder {
    int s, g0, sh;
    bool isA;
    RangeRow rr;
    const float* qrow;
    float q[WIDE ? 1 : KP];

    __device__ __forceinline__ PairBuilder(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idxA, const int ba,
                                           const int32_t* __restrict__ idxB, const int bb, const float* __restrict__ QA,
                                           const float* __restrict__ QB, const int q_stride, const int ta, const int tb) {
        const int t = threadIdx.x;
        s = t & 127, g0 = t >> 7, sh = 16 * g0;
        isA = s < PAIR_TILE;
        const int pos = (isA ? ta : tb) * PAIR_TILE + (s & (PAIR_TILE - 1));           // position in the list
        rr = range_row(xp, ld, isA ? idxA : idxB, pos, isA ? ba : bb);
        qrow = (isA ? QA : QB) + (int64_t)rr.posc * q_stride;
        if constexpr (!WIDE) load_row<KP>(qrow, q);
    }

    // calls step(st, cw, left) for the PAIR_STEPS steps of every chunk of the range: cw[0], cw[1] are the row's two dwords of step st
    // (group(st, it, cw, left) takes them apart), left the SNPs < M from the chunk's first on (>= 1).  The chunk's P rows are in Ps
    // ([256][KP]; a row >= M holds row M - 1, and mask() clears its SNP).  A step must END with a barrier: the next chunk's rows are
    // staged behind the last one
    template <class Step>
    __device__ __forceinline__ void walk(const ChunkRange cr, const int64_t ld, const int64_t M, const float* __restrict__ P, float* Ps,
                                         Step&& step) const {
        const int t = threadIdx.x;
        u32x4_t nxt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nxt[i] = range_piece(rr.x, cr.lo, i, ld);
#pragma unroll 1
        for (int64_t c = cr.lo; c < cr.hi; ++c) {
            uint32_t cw[16];                                      // the chunk's 16 dwords; every step consumes the first two
#pragma unroll
            for (int i = 0; i < 16; ++i) cw[i] = nxt[i >> 2][i & 3];
#pragma unroll
            for (int v = 0; v < KP / 4; ++v) {
                const int e = t + 256 * v;
                const int64_t j = min(c * RANGE_CHUNK + e / (KP / 4), M - 1);
                reinterpret_cast<f32x4_t*>(Ps)[e] = *reinterpret_cast<const f32x4_t*>(P + j * KP + 4 * (e % (KP / 4)));
            }
            {
                const int64_t cn = min(c + 1, cr.hi - 1);         // the next chunk's words, in flight under this chunk's work
#pragma unroll
                for (int i = 0; i < 4; ++i) nxt[i] = range_piece(rr.x, cn, i, ld);
            }
            const int left = (int)min(M - c * RANGE_CHUNK, (int64_t)(2 * RANGE_CHUNK));
            __syncthreads();
#pragma unroll 1
            for (int st = 0; st < PAIR_STEPS; ++st) {
                step(st, cw, left);
#pragma unroll
                for (int i = 0; i < 14; ++i) cw[i] = cw[i + 2];
            }
        }
    }
    // this thread's group `it` (0, 1) of step st: dword `it` of the step holds its groups 2 it and 2 it + 1
    __device__ __forceinline__ PairGroup group(const int st, const int it, const uint32_t (&cw)[16], const int left) const {
        const int g = g0 + 2 * it, jl = st * PAIR_STEP + g * 8;
        return {g, cw[it] >> sh, jl, left - jl};
    }
    // pi of the eight SNPs jl .. jl + 7 of the chunk: fp32 multiply-adds, k ascending from +0.0f; the P rows are LDS broadcasts (a group
    // is the same in all lanes of a wave)
    __device__ __forceinline__ void pi8(const float* Ps, const int jl, float (&pi)[8]) const {
#pragma unroll
        for (int e = 0; e < 8; ++e) pi[e] = 0.f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            float qk[4];
            if constexpr (WIDE) load_row<4>(qrow + k, qk);
            else { qk[0] = q[k]; qk[1] = q[k + 1]; qk[2] = q[k + 2]; qk[3] = q[k + 3]; }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float4 p4 = *reinterpret_cast<const float4*>(&Ps[(jl + e) * KP + k]);
                pi[e] = fmaf(qk[0], p4.x, pi[e]); pi[e] = fmaf(qk[1], p4.y, pi[e]);
                pi[e] = fmaf(qk[2], p4.z, pi[e]); pi[e] = fmaf(qk[3], p4.w, pi[e]);
            }
        }
    }
    // all ones where element e of a group enters the sums: the call observed, the row inside the list, the SNP < M, pimin <= pi <= 1 - pimin
    __device__ __forceinline__ uint32_t mask(const uint32_t code, const int e, const int rem, const float pi, const float pimin,
                                             const float one_m_pimin) const {
        return obs_mask(code) & rr.valid & lt_mask(e, rem) & ge0_mask(pi - pimin) & ge0_mask(one_m_pimin - pi);
    }
};

// the block's slab [PLANES][64 x 64] of its accumulators in the D layout of the instruction: wave w owns A rows 16 w .. 16 w + 15,
// acc[p][j] the B tile 16 j .. 16 j + 15; column = lane & 15, rows 4 (lane >> 4) + i.  Every block writes its whole slab
template <int PLANES>
__device__ __forceinline__ void pair_slab_store(float* __restrict__ part, const int range, const int ranges, const int tile,
                                                const f32x4_t (&acc)[PLANES][4]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* out = part + ((int64_t)range * (gridDim.x / ranges) + tile) * (PLANES * PAIR_TILE * PAIR_TILE);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (16 * w + 4 * (lane >> 4) + i) * PAIR_TILE + 16 * j + (lane & 15);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) out[p * PAIR_TILE * PAIR_TILE + o] = acc[p][j][i];
        }
}

// The fold of a [ranges][tiles][PLANES][64 x 64] slab of T: one thread per pair (a < ba, b < bb) walks the ranges in order and hands
// plane k's partial to sum.add(k, value) (k a constant after unrolling), then sum.store(e, pairs) writes pair e = a bb + b.  Sum is an
// aggregate of its output pointers (Sum::Out, its first member) and its running sums, zero by their initialisers; it decides the type
// each plane is summed in
template <class T, int PLANES, class Sum>
__global__ __launch_bounds__(256) void pair_fold_kernel(const T* __restrict__ part, const int ranges, const int tiles, const int tiles_b,
                                                        const int ba, const int bb, const typename Sum::Out out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pairs = (int64_t)ba * bb;
    if (e >= pairs) return;
    Sum sum{out};
    const int a = (int)(e / bb), b = (int)(e - (int64_t)a * bb);
    const int tile = (a / PAIR_TILE) * tiles_b + b / PAIR_TILE;
    const int o = (a % PAIR_TILE) * PAIR_TILE + b % PAIR_TILE;
#pragma clang loop vectorize(disable) interleave(disable)        // (a handful of ranges: one copy of the loop)
    for (int r = 0; r < ranges; ++r) {
        const T* p = part + ((int64_t)r * tiles + tile) * (PLANES * PAIR_TILE * PAIR_TILE) + o;
#pragma unroll
        for (int k = 0; k < PLANES; ++k) sum.add(k, p[k * PAIR_TILE * PAIR_TILE]);
    }
    sum.store(e, pairs);
}
template <class T, int PLANES, class Sum>
inline void launch_pair_fold(const T* part, const RangePlan& p, const int ba, const int bb, const typename Sum::Out out, hipStream_t st) {
    hipLaunchKernelGGL((pair_fold_kernel<T, PLANES, Sum>), fold_grid((int64_t)ba * bb), dim3(256), 0, st, part, (int)p.ranges, (int)p.tiles,
                       (bb + PAIR_TILE - 1) / PAIR_TILE, ba, bb, out);
}

}  // namespace nadm
