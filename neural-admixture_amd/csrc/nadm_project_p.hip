// The P half of the block EM over observed calls: refit one head's P against a FIXED Q with a masked EM step of the binomial admixture
// model (include/nadm.h, nadm_project_p).  The transpose of nadm_project.hip: there a lane owns a sample and P is broadcast from LDS,
// here a thread owns a SNP and Q is broadcast from LDS.
//
// Two launches per step, no floating-point atomics (two launches on the same inputs give the same bits):
//   project_p_accum_kernel  one 256-thread block per (256-SNP chunk, slice of the batch's 64-sample tiles).  A thread owns one SNP: its
//                           p, B and C rows live in registers.  A tile's 64 rows x 64 bytes of the chunk arrive as ONE 16-byte load per
//                           thread (row index and byte offset clamped: unconditional) and go to LDS, double-buffered, together with the
//                           tile's Q rows; the next tile's loads are issued before the current tile's arithmetic.  Every thread reads
//                           the SAME Q row (a broadcast) and its own byte of row i.  Missing calls (code 3), rows >= b and SNPs >= M
//                           enter every sum as exactly +0.0f.  Writes the slice's partials of B, C (fp32) and n (int32).
//   project_p_fold_kernel   one thread per (SNP, column): adds the slices' partials in slice order in float64 and applies
//                           p' = clip(pB / (pB + (1 - p)C), pmin, 1 - pmin); den == 0 returns p as it came.
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int PP_CHUNK = 256;            // SNPs per chunk = threads per block = 64 bytes of a packed row
constexpr int PP_TILE = 64;              // samples per tile: 64 rows x 64 bytes = one 16-byte load per thread
constexpr int PP_MAX_TILES = 64;         // tiles per slice at most: no fp32 running sum covers more than 4096 samples
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int64_t PP_BLOCKS = 1024;      // blocks wanted at least (256 CUs x 4 blocks of 4 waves), while there are tiles to split

template <int KP>
__global__ __launch_bounds__(PP_CHUNK) void project_p_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ bcpart, int32_t* __restrict__ npart) {
    constexpr int QF4 = PP_TILE * KP / 4;                       // float4 of a tile's Q rows
    constexpr int QV = (QF4 + PP_CHUNK - 1) / PP_CHUNK;         // of them per thread
    __shared__ __attribute__((aligned(16))) uint8_t Xs[2][PP_TILE * 64];
    __shared__ __attribute__((aligned(16))) float Qs[2][PP_TILE * KP];
    const int t = threadIdx.x;
    const int64_t chunk = blockIdx.x / slices;
    const int slice = (int)(blockIdx.x - chunk * slices);
    const int tiles = (b + PP_TILE - 1) / PP_TILE;
    const int t_lo = slice * tiles_per_slice;                   // < tiles: slices = ceil(tiles / tiles_per_slice)
    const int t_hi = min(t_lo + tiles_per_slice, tiles);
    const int64_t j = chunk * PP_CHUNK + t;

    // this thread's SNP (a SNP >= M reads row M - 1 and is turned into code 3 below, once)
    float p[KP], B[KP], Cc[KP];
    {
        const float* pr = P + (j < M ? j : M - 1) * KP;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(pr + k);
            p[k] = v.x; p[k + 1] = v.y; p[k + 2] = v.z; p[k + 3] = v.w;
            B[k] = B[k + 1] = B[k + 2] = B[k + 3] = 0.f;
            Cc[k] = Cc[k + 1] = Cc[k + 2] = Cc[k + 3] = 0.f;
        }
    }
    const uint32_t past_m = 3u & ~lt_mask64(j, M);
    const int sh = 2 * (t & 3);
    int n = 0;

    // loader role: row t / 4 of the tile, 16-byte piece t % 4 of the chunk's 64 bytes.  A piece past the row's end holds SNPs >= M
    // only (4 ld >= M), so its offset is clamped to the row's last piece and the load is unconditional
    const int lrow = t >> 2;
    const int64_t boff = min(chunk * (PP_CHUNK / 4) + 16 * (t & 3), ld - 16);
    auto row_of = [&](const int tile) {                         // matrix row of this thread's row of `tile`, clamped to the batch
        const int sc = min(tile * PP_TILE + lrow, b - 1);
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
            *reinterpret_cast<u32x4_t*>(&Xs[buf][lrow * 64 + 16 * (t & 3)]) = xv | ~lt_mask(tile * PP_TILE + lrow, b);
#pragma unroll
            for (int v = 0; v < QV; ++v) {
                const int e = t + PP_CHUNK * v;
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
                const int e = t + PP_CHUNK * v;
                if (e < QF4) {
                    const int qs = min(nt * PP_TILE + e / (KP / 4), b - 1);
                    qv[v] = *reinterpret_cast<const f32x4_t*>(Q + (int64_t)qs * q_stride + 4 * (e % (KP / 4)));
                }
            }
        }
        if (!work) continue;
        const uint8_t* xb = &Xs[buf][t >> 2];                   // this thread's byte of row i: lanes 4c..4c+3 share it
        const float* qb = Qs[buf];
#pragma unroll 4
        for (int i = 0; i < PP_TILE; ++i) {
            const uint32_t code = (((uint32_t)xb[i * 64] >> sh) | past_m) & 3u;
            // observed ? ~0 : 0 as arithmetic on the code, applied with v_and (nadm_common.h: no select on a lane condition)
            uint32_t m = ((code + 1u) >> 2) - 1u;
            asm("" : "+v"(m));
            const float* qr = qb + i * KP;
            float rr = 0.f;
            float q[KP <= 16 ? KP : 4];
            if constexpr (KP <= 16) {
#pragma unroll
                for (int k = 0; k < KP; k += 4) {
                    const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                    q[k] = t4.x; q[k + 1] = t4.y; q[k + 2] = t4.z; q[k + 3] = t4.w;
                }
#pragma unroll
                for (int k = 0; k < KP; ++k) rr = fmaf(q[k], p[k], rr);
            } else {                                            // wide heads: the row is read twice, four columns at a time
#pragma unroll
                for (int k = 0; k < KP; k += 4) {
                    const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                    rr = fmaf(t4.x, p[k], rr); rr = fmaf(t4.y, p[k + 1], rr);
                    rr = fmaf(t4.z, p[k + 2], rr); rr = fmaf(t4.w, p[k + 3], rr);
                }
            }
            // 1 - r from the UNCLIPPED product, as project_accum_kernel
            const float r = fminf(fmaxf(rr, eps), one_m_eps);
            const float u = fminf(fmaxf(1.f - rr, eps), one_m_eps);
            const float g = (float)code, h = 2.f - g;
            const float t1 = keepf(g * __builtin_amdgcn_rcpf(r), m);          // masked: exactly +0.0f
            const float t0 = keepf(h * __builtin_amdgcn_rcpf(u), m);
            if constexpr (KP <= 16) {
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    B[k] = fmaf(q[k], t1, B[k]);
                    Cc[k] = fmaf(q[k], t0, Cc[k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < KP; k += 4) {
                    const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                    q[0] = t4.x; q[1] = t4.y; q[2] = t4.z; q[3] = t4.w;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        B[k + c] = fmaf(q[c], t1, B[k + c]);
                        Cc[k + c] = fmaf(q[c], t0, Cc[k + c]);
                    }
                }
            }
            n += (int)(m & 1u);
        }
    }
    // every thread of the block writes its row of the slice's slab (rows M..Mp hold zeros and are never read)
    const int64_t o = (int64_t)slice * Mp + j;
    float* out = bcpart + o * (2 * KP);
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        *reinterpret_cast<float4*>(out + k) = make_float4(B[k], B[k + 1], B[k + 2], B[k + 3]);
        *reinterpret_cast<float4*>(out + KP + k) = make_float4(Cc[k], Cc[k + 1], Cc[k + 2], Cc[k + 3]);
    }
    npart[o] = n;
}

// One thread per (SNP j < M, column c < kp): the slices' partials in slice order, in float64; rows >= M of Pout are never written.
__global__ __launch_bounds__(256) void project_p_fold_kernel(const float* __restrict__ bcpart, const int32_t* __restrict__ npart,
                                                             const int slices, const int64_t Mp, const int64_t M, const int k, const int kp,
                                                             const float* Pin, float* Pout,   /* may alias */
                                                             const float pmin, int32_t* __restrict__ nobs_snp) {
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
    const float pi = Pin[e];
    float out = 0.f;                                             // pad columns are written 0
    if (c < k) {
        const double num = (double)pi * Bs;
        const double den = num + (1.0 - (double)pi) * Cs;
        out = pi;                                                // den == 0 (nobody observes the SNP): the bits as they came
        if (den > 0.0) {
            double v = num / den;
            const double lo = (double)pmin, hi = 1.0 - (double)pmin;
            v = v < lo ? lo : (v > hi ? hi : v);
            out = (float)v;
        }
    }
    Pout[e] = out;
    if (nobs_snp && c == 0) {
        int n = 0;
        for (int s = 0; s < slices; ++s) n += npart[(int64_t)s * Mp + j];
        nobs_snp[j] = n;
    }
}

static int64_t pp_chunks(int64_t M) { return (M + PP_CHUNK - 1) / PP_CHUNK; }
static int pp_tiles(int b) { return (b + PP_TILE - 1) / PP_TILE; }

// tiles per slice, a rule of (b, M) alone: as many slices as it takes to put PP_BLOCKS blocks on the chip while there are tiles to
// split, and never more than PP_MAX_TILES tiles in one slice
static int pp_tiles_per_slice(int b, int64_t M) {
    const int64_t tiles = pp_tiles(b), chunks = pp_chunks(M);
    int64_t want = (PP_BLOCKS + chunks - 1) / chunks;
    if (want > tiles) want = tiles;
    const int64_t least = (tiles + PP_MAX_TILES - 1) / PP_MAX_TILES;
    if (want < least) want = least;
    return (int)((tiles + want - 1) / want);
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_project_p_slices(int32_t b, int64_t M) {
    if (b <= 0 || M <= 0) return 0;
    const int tps = pp_tiles_per_slice(b, M);
    return (pp_tiles(b) + tps - 1) / tps;
}

// scratch: B | C partials [slices, Mp, 2 kp] float | n partials [slices, Mp] int32, Mp = 256 chunks.  Sized by a bound of
// slices x chunks that grows with b and with M (the product itself does not: ceil(1024 / chunks) chunks wobbles with chunks)
extern "C" int64_t nadm_project_p_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    if (b <= 0 || M <= 0 || kp <= 0 || kp > NADM_MAX_K) return 0;
    const int64_t tiles = pp_tiles(b), chunks = pp_chunks(M);
    const int64_t least = (tiles + PP_MAX_TILES - 1) / PP_MAX_TILES;
    int64_t blocks = chunks * tiles < PP_BLOCKS - 1 + chunks ? chunks * tiles : PP_BLOCKS - 1 + chunks;
    if (blocks < chunks * least) blocks = chunks * least;
    return blocks * PP_CHUNK * (2 * (int64_t)kp + 1);
}

extern "C" int nadm_project_p(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                              int32_t k, int32_t kp, const float* Pin, float* Pout, float eps, float pmin, int32_t* nobs_snp,
                              float* scratch, void* stream) {
    if (!xp || !Q || !Pin || !Pout || !scratch) return fail("nadm_project_p: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_project_p: empty batch (need b > 0 and M > 0)");
    if (ld * 4 < M) return fail("nadm_project_p: ld < ceil(M/4)");
    if (ld % 16 != 0 || ld >= (1ll << 32)) return fail("nadm_project_p: ld must be a multiple of 16 and < 2^32");
    if (k < 1 || k > NADM_MAX_K) return fail("nadm_project_p: K must be in 1..NADM_MAX_K");
    if (kp != nadm_pad_k(k)) return fail("nadm_project_p: kp must be nadm_pad_k(k)");
    if (q_stride < kp) return fail("nadm_project_p: q_stride < kp");
    if (q_stride % 4 != 0) return fail("nadm_project_p: q_stride must be a multiple of 4");
    if (!(eps >= 1e-9f && eps < 0.5f)) return fail("nadm_project_p: eps must be in [1e-9, 0.5)");
    if (!(pmin >= 0.f && pmin < 0.5f)) return fail("nadm_project_p: pmin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)Pin | (uintptr_t)Pout | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_project_p: xp, Q, Pin, Pout and scratch must be 16-byte aligned");
    const int64_t chunks = pp_chunks(M), Mp = chunks * PP_CHUNK;
    const int tps = pp_tiles_per_slice(b, M);
    const int slices = (pp_tiles(b) + tps - 1) / tps;
    if (chunks * slices > 0x7FFFFFFFll || (M * kp + 255) / 256 > 0x7FFFFFFFll)
        return fail("nadm_project_p: too many blocks for one launch");
    float* bcpart = scratch;
    int32_t* npart = reinterpret_cast<int32_t*>(scratch + (int64_t)slices * Mp * 2 * kp);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps;
#define NADM_PP_CASE(KP)                                                                                                                 \
    case KP:                                                                                                                             \
        hipLaunchKernelGGL((project_p_accum_kernel<KP>), dim3(grid), dim3(PP_CHUNK), 0, st, xp, ld, idx, b, M, Pin, Q, q_stride, eps, ome, \
                           slices, tps, Mp, bcpart, npart);                                                                              \
        break;
    switch (kp) {
        NADM_PP_CASE(4) NADM_PP_CASE(8) NADM_PP_CASE(12) NADM_PP_CASE(16)
        NADM_PP_CASE(24) NADM_PP_CASE(32) NADM_PP_CASE(48) NADM_PP_CASE(64)
        default: return fail("nadm_project_p: unsupported padded K (use nadm_pad_k)");
    }
#undef NADM_PP_CASE
    if (int e = check_launch("project_p (accumulate)")) return e;
    hipLaunchKernelGGL(project_p_fold_kernel, dim3((unsigned)((M * kp + 255) / 256)), dim3(256), 0, st, bcpart, npart, slices, Mp, M, k, kp,
                       Pin, Pout, pmin, nobs_snp);
    return check_launch("project_p (fold)");
}
