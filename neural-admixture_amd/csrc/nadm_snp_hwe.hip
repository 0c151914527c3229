// Hardy-Weinberg proportions GIVEN ANCESTRY: the per-SNP score test of an inbreeding coefficient F at F = 0 in the binomial admixture
// model (include/nadm.h, nadm_snp_hwe).  One pass of N M K work over the packed matrix in the shape of nadm_project_p.hip: a thread owns
// a SNP, Q is broadcast from LDS.
//
// Two launches per call, no floating-point atomics (two launches on the same inputs give the same bits):
//   snp_hwe_accum_kernel  one 256-thread block per (256-SNP chunk, slice of the batch's 64-sample tiles).  A thread owns one SNP: its
//                         p row and four running sums (U and Hexp in fp32, n and Hobs in int32) live in registers.  A tile's 64 rows
//                         x 64 bytes of the chunk arrive as ONE 16-byte load per thread (row index and byte offset clamped:
//                         unconditional) and go to LDS, double-buffered, together with the tile's Q rows; the next tile's loads are
//                         issued before the current tile's arithmetic.  Every thread reads the SAME Q row (a broadcast) and its own
//                         byte of row i.  Per genotype: KP multiply-adds, one reciprocal.  Missing calls (code 3), rows >= b, SNPs
//                         >= M and a masked pi enter every sum as exactly +0.0f / 0.  Writes the slice's partials, 16 bytes per SNP.
//   snp_hwe_fold_kernel   one thread per SNP: adds the slices' partials in slice order, U and Hexp in float64, n and Hobs as integers.
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int HW_CHUNK = 256;            // SNPs per chunk = threads per block = 64 bytes of a packed row
constexpr int HW_TILE = 64;              // samples per tile: 64 rows x 64 bytes = one 16-byte load per thread
constexpr int HW_MAX_TILES = 64;         // tiles per slice at most: no fp32 running sum covers more than 4096 samples
constexpr int64_t HW_BLOCKS = 1024;      // blocks wanted at least (256 CUs x 4 blocks of 4 waves), while there are tiles to split
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// x >= 0 ? ~0 : 0 from the sign bit (a NaN or -0.0f goes by its sign bit; x = a - b of finite a != b is never -0.0f, a == b gives +0.0f)
__device__ __forceinline__ uint32_t ge0_mask(float x) {
    uint32_t m = ~(uint32_t)((int)__float_as_uint(x) >> 31);
    asm("" : "+v"(m));
    return m;
}

template <int KP>
__global__ __launch_bounds__(HW_CHUNK) void snp_hwe_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const float pimin, const float one_m_pimin, const int slices, const int tiles_per_slice, const int64_t Mp,
    u32x4_t* __restrict__ part) {
    constexpr int QF4 = HW_TILE * KP / 4;                       // float4 of a tile's Q rows
    constexpr int QV = (QF4 + HW_CHUNK - 1) / HW_CHUNK;         // of them per thread
    __shared__ __attribute__((aligned(16))) uint8_t Xs[2][HW_TILE * 64];
    __shared__ __attribute__((aligned(16))) float Qs[2][HW_TILE * KP];
    const int t = threadIdx.x;
    const int64_t chunk = blockIdx.x / slices;
    const int slice = (int)(blockIdx.x - chunk * slices);
    const int tiles = (b + HW_TILE - 1) / HW_TILE;
    const int t_lo = slice * tiles_per_slice;                   // < tiles: slices = ceil(tiles / tiles_per_slice)
    const int t_hi = min(t_lo + tiles_per_slice, tiles);
    const int64_t j = chunk * HW_CHUNK + t;

    // this thread's SNP (a SNP >= M reads row M - 1 and is turned into code 3 below, once)
    float p[KP];
    {
        const float* pr = P + (j < M ? j : M - 1) * KP;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(pr + k);
            p[k] = v.x; p[k + 1] = v.y; p[k + 2] = v.z; p[k + 3] = v.w;
        }
    }
    const uint32_t past_m = 3u & ~lt_mask64(j, M);
    const int sh = 2 * (t & 3);
    float U = 0.f, H = 0.f;
    int n = 0, hobs = 0;

    // loader role: row t / 4 of the tile, 16-byte piece t % 4 of the chunk's 64 bytes.  A piece past the row's end holds SNPs >= M
    // only (4 ld >= M), so its offset is clamped to the row's last piece and the load is unconditional
    const int lrow = t >> 2;
    const int64_t boff = min(chunk * (HW_CHUNK / 4) + 16 * (t & 3), ld - 16);
    auto row_of = [&](const int tile) {                         // matrix row of this thread's row of `tile`, clamped to the batch
        const int sc = min(tile * HW_TILE + lrow, b - 1);
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
            // barrier: one barrier per tile.  A row >= b becomes "every call missing" here, not at the load
            *reinterpret_cast<u32x4_t*>(&Xs[buf][lrow * 64 + 16 * (t & 3)]) = xv | ~lt_mask(tile * HW_TILE + lrow, b);
#pragma unroll
            for (int v = 0; v < QV; ++v) {
                const int e = t + HW_CHUNK * v;
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
                const int e = t + HW_CHUNK * v;
                if (e < QF4) {
                    const int qs = min(nt * HW_TILE + e / (KP / 4), b - 1);
                    qv[v] = *reinterpret_cast<const f32x4_t*>(Q + (int64_t)qs * q_stride + 4 * (e % (KP / 4)));
                }
            }
        }
        if (!work) continue;
        const uint8_t* xb = &Xs[buf][t >> 2];                   // this thread's byte of row i: lanes 4c..4c+3 share it
        const float* qb = Qs[buf];
#pragma unroll 4
        for (int i = 0; i < HW_TILE; ++i) {
            const uint32_t code = (((uint32_t)xb[i * 64] >> sh) | past_m) & 3u;
            // observed ? ~0 : 0, g == 0 ? ~0 : 0 and g == 1 ? ~0 : 0 as arithmetic on the code, applied with v_and / v_bfi
            // (nadm_common.h: no select on a lane condition)
            uint32_t m = ((code + 1u) >> 2) - 1u;
            uint32_t m0 = (uint32_t)((int)(code - 1u) >> 31);
            uint32_t m1 = (uint32_t)((int)((code ^ 1u) - 1u) >> 31);
            asm("" : "+v"(m));
            asm("" : "+v"(m0));
            asm("" : "+v"(m1));
            const float* qr = qb + i * KP;
            float pi = 0.f;
#pragma unroll
            for (int k = 0; k < KP; k += 4) {                   // a broadcast; wide heads take the row the same way, four columns at a time
                const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
                pi = fmaf(t4.x, p[k], pi); pi = fmaf(t4.y, p[k + 1], pi);
                pi = fmaf(t4.z, p[k + 2], pi); pi = fmaf(t4.w, p[k + 3], pi);
            }
            m &= ge0_mask(pi - pimin) & ge0_mask(one_m_pimin - pi);
            // 1 - pi from the UNCLIPPED product, as project_p_accum_kernel
            const float r = fminf(fmaxf(pi, eps), one_m_eps);
            const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
            // g = 0: r / u, g = 2: u / r, g = 1: -1
            const float num = __uint_as_float(blend(__float_as_uint(r), __float_as_uint(u), m0));
            const float den = __uint_as_float(blend(__float_as_uint(u), __float_as_uint(r), m0));
            const float ratio = num * __builtin_amdgcn_rcpf(den);
            const float tt = __uint_as_float(blend(0xBF800000u, __float_as_uint(ratio), m1));
            U += keepf(tt, m);                                  // masked: exactly +0.0f
            H += keepf((pi + pi) * (1.f - pi), m);
            n += (int)(m & 1u);
            hobs += (int)(m & m1 & 1u);
        }
    }
    // every thread of the block writes its SNP's 16 bytes of the slice's slab (rows M..Mp hold zeros and are never read)
    part[(int64_t)slice * Mp + j] = (u32x4_t){__float_as_uint(U), __float_as_uint(H), (uint32_t)n, (uint32_t)hobs};
}

// One thread per SNP j < M: the slices' partials in slice order, U and Hexp in float64, n and Hobs as integers
__global__ __launch_bounds__(256) void snp_hwe_fold_kernel(const u32x4_t* __restrict__ part, const int slices, const int64_t Mp,
                                                           const int64_t M, double* __restrict__ U, double* __restrict__ Hexp,
                                                           int32_t* __restrict__ nobs, int32_t* __restrict__ Hobs) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double us = 0.0, hs = 0.0;
    int n = 0, ho = 0;
    for (int s = 0; s < slices; ++s) {
        const u32x4_t v = part[(int64_t)s * Mp + j];
        us += (double)__uint_as_float(v[0]);
        hs += (double)__uint_as_float(v[1]);
        n += (int)v[2];
        ho += (int)v[3];
    }
    U[j] = us;
    nobs[j] = n;
    if (Hexp) Hexp[j] = hs;
    if (Hobs) Hobs[j] = ho;
}

static int64_t hw_chunks(int64_t M) { return (M + HW_CHUNK - 1) / HW_CHUNK; }
static int hw_tiles(int b) { return (b + HW_TILE - 1) / HW_TILE; }

// tiles per slice, a rule of (b, M) alone: as many slices as it takes to put HW_BLOCKS blocks on the chip while there are tiles to
// split, and never more than HW_MAX_TILES tiles in one slice
static int hw_tiles_per_slice(int b, int64_t M) {
    const int64_t tiles = hw_tiles(b), chunks = hw_chunks(M);
    int64_t want = (HW_BLOCKS + chunks - 1) / chunks;
    if (want > tiles) want = tiles;
    const int64_t least = (tiles + HW_MAX_TILES - 1) / HW_MAX_TILES;
    if (want < least) want = least;
    return (int)((tiles + want - 1) / want);
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_snp_hwe_slices(int32_t b, int64_t M) {
    if (b <= 0 || M <= 0) return 0;
    const int tps = hw_tiles_per_slice(b, M);
    return (hw_tiles(b) + tps - 1) / tps;
}

// scratch: the partials [slices, Mp] x { U, Hexp (fp32), n, Hobs (int32) }, Mp = 256 chunks.  Sized by a bound of slices x chunks that
// grows with b and with M (the product itself does not: ceil(1024 / chunks) chunks wobbles with chunks)
extern "C" int64_t nadm_snp_hwe_scratch_floats(int32_t b, int64_t M) {
    if (b <= 0 || M <= 0) return 0;
    const int64_t tiles = hw_tiles(b), chunks = hw_chunks(M);
    const int64_t least = (tiles + HW_MAX_TILES - 1) / HW_MAX_TILES;
    int64_t blocks = chunks * tiles < HW_BLOCKS - 1 + chunks ? chunks * tiles : HW_BLOCKS - 1 + chunks;
    if (blocks < chunks * least) blocks = chunks * least;
    return blocks * HW_CHUNK * 4;
}

extern "C" int nadm_snp_hwe(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Q, int32_t q_stride,
                            int32_t k, int32_t kp, const float* P, float eps, float pimin, double* U, double* Hexp, int32_t* nobs,
                            int32_t* Hobs, float* scratch, void* stream) {
    if (!xp || !Q || !P || !U || !nobs || !scratch) return fail("nadm_snp_hwe: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_snp_hwe: empty block (need b > 0 and M > 0)");
    if (ld * 4 < M) return fail("nadm_snp_hwe: ld < ceil(M/4)");
    if (ld % 16 != 0 || ld >= (1ll << 32)) return fail("nadm_snp_hwe: ld must be a multiple of 16 and < 2^32");
    if (k < 1 || k > NADM_MAX_K) return fail("nadm_snp_hwe: K must be in 1..NADM_MAX_K");
    if (kp != nadm_pad_k(k)) return fail("nadm_snp_hwe: kp must be nadm_pad_k(k)");
    if (q_stride < kp) return fail("nadm_snp_hwe: q_stride < kp");
    if (q_stride % 4 != 0) return fail("nadm_snp_hwe: q_stride must be a multiple of 4");
    if (!(eps >= 1e-9f && eps < 0.5f)) return fail("nadm_snp_hwe: eps must be in [1e-9, 0.5)");
    if (!(pimin >= 0.f && pimin < 0.5f)) return fail("nadm_snp_hwe: pimin must be in [0, 0.5)");
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)P | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_snp_hwe: xp, Q, P and scratch must be 16-byte aligned");
    if ((((uintptr_t)U | (uintptr_t)Hexp) & 7) != 0 || (((uintptr_t)nobs | (uintptr_t)Hobs | (uintptr_t)idx) & 3) != 0)
        return fail("nadm_snp_hwe: U, Hexp must be 8-byte and nobs, Hobs, idx 4-byte aligned");
    const int64_t chunks = hw_chunks(M), Mp = chunks * HW_CHUNK;
    const int tps = hw_tiles_per_slice(b, M);
    const int slices = (hw_tiles(b) + tps - 1) / tps;
    if (chunks * slices > 0x7FFFFFFFll) return fail("nadm_snp_hwe: too many blocks for one launch");
    u32x4_t* part = reinterpret_cast<u32x4_t*>(scratch);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps, omp = 1.f - pimin;
#define NADM_HW_CASE(KP)                                                                                                               \
    case KP:                                                                                                                           \
        hipLaunchKernelGGL((snp_hwe_accum_kernel<KP>), dim3(grid), dim3(HW_CHUNK), 0, st, xp, ld, idx, b, M, P, Q, q_stride, eps, ome, \
                           pimin, omp, slices, tps, Mp, part);                                                                         \
        break;
    switch (kp) {
        NADM_HW_CASE(4) NADM_HW_CASE(8) NADM_HW_CASE(12) NADM_HW_CASE(16)
        NADM_HW_CASE(24) NADM_HW_CASE(32) NADM_HW_CASE(48) NADM_HW_CASE(64)
        default: return fail("nadm_snp_hwe: unsupported padded K (use nadm_pad_k)");
    }
#undef NADM_HW_CASE
    if (int e = check_launch("snp_hwe (accumulate)")) return e;
    hipLaunchKernelGGL(snp_hwe_fold_kernel, dim3((unsigned)chunks), dim3(256), 0, st, part, slices, Mp, M, U, Hexp, nobs, Hobs);
    return check_launch("snp_hwe (fold)");
}
