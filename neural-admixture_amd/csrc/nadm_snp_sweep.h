// The SNP-owner sweep over the packed matrix, shared by the kernels that keep per-SNP sums over a batch of samples
// (project_p_accum_kernel in nadm_project_p.hip, snp_hwe_accum_kernel in nadm_snp_hwe.hip): a thread owns a SNP, Q is broadcast from LDS.
//
// One 256-thread block per (256-SNP chunk, slice of the batch's 64-sample tiles).  A thread owns one SNP: its row of P and its running
// sums live in the kernel's registers.  A tile's 64 rows x 64 bytes of the chunk arrive as ONE 16-byte load per thread (row index and
// byte offset clamped: unconditional) and go to LDS, double-buffered, together with the tile's Q rows; the next tile's loads are issued
// before the current tile's arithmetic.  Every thread reads the SAME Q row (a broadcast) and its own byte of row i.  Missing calls come
// as code 3; rows >= b and SNPs >= M are turned into code 3 here, so that a body masks on the code alone.
//
// A kernel is three parts: its prologue (sweep_pos, sweep_load_p, its sums zeroed), snp_sweep with a lambda that holds its arithmetic
// for one genotype, and its epilogue store to row slice * Mp + j of the slice's slab (rows M..Mp hold zeros and are never read).
#pragma once
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int SWEEP_CHUNK = 256;         // SNPs per chunk = threads per block = 64 bytes of a packed row
constexpr int SWEEP_TILE = 64;           // samples per tile: 64 rows x 64 bytes = one 16-byte load per thread
constexpr int SWEEP_MAX_TILES = 64;      // tiles per slice at most: no fp32 running sum covers more than 4096 samples
constexpr int64_t SWEEP_BLOCKS = 1024;   // blocks wanted at least (256 CUs x 4 blocks of 4 waves), while there are tiles to split

// ---- host: the launch shape, a rule of (b, M) alone (nadm_host.h: split_per_part, split_blocks_bound)
inline int64_t sweep_chunks(int64_t M) { return (M + SWEEP_CHUNK - 1) / SWEEP_CHUNK; }
inline int sweep_tiles(int b) { return (b + SWEEP_TILE - 1) / SWEEP_TILE; }
inline int sweep_tiles_per_slice(int b, int64_t M) {
    return (int)split_per_part(sweep_tiles(b), sweep_chunks(M), SWEEP_BLOCKS, SWEEP_MAX_TILES);
}
inline int sweep_slices(int b, int64_t M) {
    const int tps = sweep_tiles_per_slice(b, M);
    return (sweep_tiles(b) + tps - 1) / tps;
}
// (slice, SNP) rows of partials a scratch buffer must hold: a bound of slices x 256 chunks that grows with b and with M
inline int64_t sweep_rows_bound(int b, int64_t M) {
    return split_blocks_bound(sweep_tiles(b), sweep_chunks(M), SWEEP_BLOCKS, SWEEP_MAX_TILES) * SWEEP_CHUNK;
}

// ---- device
struct SweepPos {
    int64_t chunk;
    int slice;
    int64_t j;                           // this thread's SNP; may be >= M in the last chunk
};
__device__ __forceinline__ SweepPos sweep_pos(const int slices) {
    SweepPos s;
    s.chunk = blockIdx.x / slices;
    s.slice = (int)(blockIdx.x - s.chunk * slices);
    s.j = s.chunk * SWEEP_CHUNK + threadIdx.x;
    return s;
}

// this thread's row of P (a SNP >= M reads row M - 1; the sweep turns its calls into code 3)
template <int KP>
__device__ __forceinline__ void sweep_load_p(const float* __restrict__ P, const int64_t j, const int64_t M, float (&p)[KP]) {
    const float* pr = P + (j < M ? j : M - 1) * KP;
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(pr + k);
        p[k] = v.x; p[k + 1] = v.y; p[k + 2] = v.z; p[k + 3] = v.w;
    }
}

// calls body(code, qrow) once per (sample of the slice, this thread's SNP), samples in order: code is the 2-bit call (3 = nothing to
// add), qrow the sample's KP floats of Q in LDS, the same address in every thread
template <int KP, class Body>
__device__ __forceinline__ void snp_sweep(const SweepPos pos, const uint8_t* __restrict__ xp, const int64_t ld,
                                          const int32_t* __restrict__ idx, const int b, const int64_t M, const float* __restrict__ Q,
                                          const int q_stride, const int tiles_per_slice, Body&& body) {
    constexpr int QF4 = SWEEP_TILE * KP / 4;                    // float4 of a tile's Q rows
    constexpr int QV = (QF4 + SWEEP_CHUNK - 1) / SWEEP_CHUNK;   // of them per thread
    __shared__ __attribute__((aligned(16))) uint8_t Xs[2][SWEEP_TILE * 64];
    __shared__ __attribute__((aligned(16))) float Qs[2][SWEEP_TILE * KP];
    const int t = threadIdx.x;
    const int tiles = (b + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_lo = pos.slice * tiles_per_slice;               // < tiles: slices = ceil(tiles / tiles_per_slice)
    const int t_hi = min(t_lo + tiles_per_slice, tiles);
    const uint32_t past_m = 3u & ~lt_mask64(pos.j, M);
    const int sh = 2 * (t & 3);

    // loader role: row t / 4 of the tile, 16-byte piece t % 4 of the chunk's 64 bytes.  A piece past the row's end holds SNPs >= M
    // only (4 ld >= M), so its offset is clamped to the row's last piece and the load is unconditional
    const int lrow = t >> 2;
    const int64_t boff = min(pos.chunk * (SWEEP_CHUNK / 4) + 16 * (t & 3), ld - 16);
    auto row_of = [&](const int tile) {                         // matrix row of this thread's row of `tile`, clamped to the batch
        const int sc = min(tile * SWEEP_TILE + lrow, b - 1);
        return idx ? idx[sc] : sc;
    };
    int row = row_of(t_lo);
    u32x4_t xv = {0u, 0u, 0u, 0u};
    f32x4_t qv[QV];
#pragma unroll
    for (int v = 0; v < QV; ++v) qv[v] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // one iteration ahead of the arithmetic: iteration `tile` stores tile's rows (fetched by the iteration before) to LDS, issues
    // the loads of tile + 1 and then works on tile, so that the loads are in flight under the arithmetic
#pragma unroll 1
    for (int tile = t_lo - 1; tile < t_hi; ++tile) {
        const bool work = tile >= t_lo;
        const int buf = (tile - t_lo) & 1;
        if (work) {
            // the other buffer was read in the previous iteration, which every thread left before it passed this iteration's
            // barrier: one barrier per tile.  A row >= b becomes "every call missing" here, not at the load: nothing may consume
            // a load before the arithmetic it is meant to run under
            *reinterpret_cast<u32x4_t*>(&Xs[buf][lrow * 64 + 16 * (t & 3)]) = xv | ~lt_mask(tile * SWEEP_TILE + lrow, b);
#pragma unroll
            for (int v = 0; v < QV; ++v) {
                const int e = t + SWEEP_CHUNK * v;
                if (e < QF4) reinterpret_cast<f32x4_t*>(Qs[buf])[e] = qv[v];
            }
        }
        __syncthreads();
        {
            const int nt = min(tile + 1, t_hi - 1);
            xv = *reinterpret_cast<const u32x4_t*>(xp + (int64_t)row * ld + boff);
            row = row_of(min(tile + 2, t_hi - 1));              // (the gather list one tile further ahead: no load waits on a load)
#pragma unroll
            for (int v = 0; v < QV; ++v) {
                const int e = t + SWEEP_CHUNK * v;
                if (e < QF4) {
                    const int qs = min(nt * SWEEP_TILE + e / (KP / 4), b - 1);
                    qv[v] = *reinterpret_cast<const f32x4_t*>(Q + (int64_t)qs * q_stride + 4 * (e % (KP / 4)));
                }
            }
        }
        if (!work) continue;
        const uint8_t* xb = &Xs[buf][t >> 2];                   // this thread's byte of row i: lanes 4c..4c+3 share it
        const float* qb = Qs[buf];
#pragma unroll 4
        for (int i = 0; i < SWEEP_TILE; ++i) body((((uint32_t)xb[i * 64] >> sh) | past_m) & 3u, qb + i * KP);
    }
}

}  // namespace nadm
