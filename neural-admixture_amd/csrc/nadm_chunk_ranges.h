// The chunk-range scaffolding shared by the kernels that work a block of sample rows over the SNP axis of the packed matrix
// (kinship_accum_kernel in nadm_kinship.hip, king_accum_kernel in nadm_king.hip, resid_cor_accum_kernel in nadm_resid_cor.hip,
// obs_project_kernel in nadm_obs_project.hip): the counterpart of nadm_snp_sweep.h for the kernels that own samples, not SNPs.
//
// One 256-thread block per (tile of the block's rows, range of consecutive 256-SNP chunks).  The block keeps its running sums in
// registers for the whole range and writes its slab of partials once; a second launch folds the ranges' slabs in range order (no
// floating-point atomics: the same inputs give the same bits).  The chunk axis is cut by the split rule of nadm_host_rules.h, a rule
// of the shape alone: as many ranges as it takes to put BLOCKS blocks on the chip given the tile count, while there are chunks to
// split, and never more than MAX_CHUNKS chunks in one range (what one running sum may cover).
//
// A unit supplies: its tile count, BLOCKS and MAX_CHUNKS (-> range_plan), its blockIdx -> (tile, range) order (which decides the blocks
// that share L2 lines: range fastest in kinship and king, tile fastest in obs_project, group fastest in resid_cor), the list positions
// of the rows its threads own (-> range_row, range_piece; resid_cor, which skips what the others clamp, keeps its own loads), its
// arithmetic per chunk, and its slab layout.  The [ranges][tiles][PLANES][64 x 64] slabs of kinship and king share pair_fold_kernel;
// resid_cor ([..][256][GB][4]) and obs_project ([ranges][rows][CP], rounded to fp32) keep folds of their own: index arithmetic is all
// there is to them.
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
