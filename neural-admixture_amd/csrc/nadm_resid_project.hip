// Residual PCA given Q and P: the two products of the model's standardised (Pearson) residuals with a tall-skinny fp32 operand
// (include/nadm.h, nadm_resid_project / nadm_resid_project_t).  With pi = q . p in fp32,
//   a_ij = m_ij (g_ij - 2 pi_ij) / sqrt(2 r u),   r = clip(pi), u = clip(1 - pi),   m: observed, j < M and pimin <= pi <= 1 - pimin
//   forward     Y[i, c] = sum_j a_ij W[j, c]     ss_i = sum_j a_ij^2     nobs_i = sum_j m_ij
//   transposed  O[j, c] = sum_i a_ij Yin[i, c]   nobs_snp_j = sum_i m_ij
// The scale depends on sample and SNP jointly, so no operand of nadm_obs_project carries it: each product is one pass of its own.
//
// The column sums are fp32 multiply-adds on the VALU, a lane per output row (DESIGN.md 4.19 gives the budget and why the matrix pipe was
// not taken).  Two launches per call and a third for the transposed product's operand image, no floating-point atomics (two launches
// on the same inputs give the same bits):
//   resid_project_kernel     a lane per sample on the chunk-range plan of nadm_chunk_ranges.h: sample_walk's loop written out (that
//                            header says why) with a second staged matrix.  The CP running sums, ss and n live in registers for the
//                            whole range; the chunk's P rows and W rows sit in LDS once per block.  Per genotype: KP multiply-adds for
//                            pi, the mask, two clips, one multiply-add for g - 2 pi, one multiply and one reciprocal square root for
//                            the scale, CP multiply-adds.  ss is an fp32 sum within a chunk and a float64 sum over the range's chunks.
//   resid_project_t_kernel   the SNP-owner sweep of nadm_snp_sweep.h over ONE operand image [b][KP + CP] = (q row | Yin row) that
//                            resid_pack_kernel writes first: the sweep's loader then brings both rows of a sample to LDS as it brings Q
//                            for the other kernels, unchanged.  A thread's p row, the CP running sums and n live in registers.
//   the two fold kernels     one thread per output row: the ranges' / slices' partials in order in float64, rounded to fp32 once; pad
//                            columns +0.0.
// Missing calls (code 3), rows past the list, SNPs >= M and a masked pi give a = +0.0f exactly.
#include "nadm_chunk_ranges.h"
#include "nadm_snp_sweep.h"

namespace nadm {

constexpr int RP_MAX_KP = 16;
constexpr int RP_TILE = 256;              // samples per block of the forward product: 4 waves, a lane per sample
constexpr int RP_MAX_CHUNKS = 1024;       // chunks per range at most: no fp32 running sum covers more than 2^18 SNPs
constexpr int64_t RP_BLOCKS = 1024;       // blocks wanted at least, while there are chunks to split

// the standardised residual of one call: pi unclipped, code the call, m its mask so far (observed, row and SNP inside); m gains the
// pimin rule.  1 - pi from the UNCLIPPED product, as em_terms (nadm_common.h).  Masked: exactly +0.0f
__device__ __forceinline__ float resid_term(const float pi, const uint32_t code, uint32_t& m, const float eps, const float one_m_eps,
                                            const float pimin, const float one_m_pimin) {
    m &= ge0_mask(pi - pimin) & ge0_mask(one_m_pimin - pi);
    const float r = fminf(fmaxf(pi, eps), one_m_eps);
    const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
    const float d = fmaf(-2.f, pi, (float)code);
    return keepf(d * __builtin_amdgcn_rsqf((r + r) * u), m);
}

template <int KP, int CP>
__global__ __launch_bounds__(RP_TILE) void resid_project_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const float pimin, const float one_m_pimin, const float* __restrict__ W, const int tiles, const int64_t chunks_per_range,
    const int64_t chunks, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Ps[RANGE_CHUNK * KP];      // the chunk's P rows (16 KB at KP = 16)
    __shared__ __attribute__((aligned(16))) float Ws[RANGE_CHUNK * CP];      // the chunk's W rows (32 KB at CP = 32)
    const int t = threadIdx.x;
    const int range = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - range * tiles;       // tile fastest: neighbours share a chunk of P and W
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);
    const RangeRow rr = range_row(xp, ld, idx, tile * RP_TILE + t, b);
    const uint32_t inval = ~rr.valid;                             // a row past the list: every call missing
    const bool wave_live = tile * RP_TILE + (t & ~63) < b;        // wave-uniform

    float q[KP];
    load_row<KP>(Q + (int64_t)rr.posc * q_stride, q);
    float acc[CP];
#pragma unroll
    for (int i = 0; i < CP; ++i) acc[i] = 0.f;
    double ss = 0.0;
    int n = 0;

    u32x4_t nxt[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, c_lo, v, ld);

#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        const int64_t j0 = c * RANGE_CHUNK;
        if (c > c_lo) __syncthreads();                            // the previous chunk's rows have been read
        stage_rows<RANGE_CHUNK, KP, RP_TILE>(P, j0, M, Ps);       // the chunk's P and W rows, zeros past M
        stage_rows<RANGE_CHUNK, CP, RP_TILE>(W, j0, M, Ws);
        uint32_t w[16];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            w[4 * v] = nxt[v][0] | inval; w[4 * v + 1] = nxt[v][1] | inval;
            w[4 * v + 2] = nxt[v][2] | inval; w[4 * v + 3] = nxt[v][3] | inval;
        }
        {
            const int64_t cn = min(c + 1, c_hi - 1);              // the next chunk's words, in flight under this chunk's arithmetic
#pragma unroll
            for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cn, v, ld);
        }
        __syncthreads();
        if (!wave_live) continue;
        float ssc = 0.f;                                          // the chunk's sum of squares: 256 terms in fp32
#pragma unroll 1
        for (int wi = 0; wi < 16; ++wi) {                         // one 32-bit word = 16 SNPs
            const uint32_t bits = chunk_word(w, wi, M - (j0 + 16 * wi));      // SNPs >= M as code 3
#pragma unroll 4
            for (int e = 0; e < 16; ++e) {
                const uint32_t code = (bits >> (2 * e)) & 3u;
                uint32_t m = obs_mask(code);
                const float a = resid_term(dot_row<KP>(q, Ps + (wi * 16 + e) * KP), code, m, eps, one_m_eps, pimin, one_m_pimin);
                n += (int)(m & 1u);
                ssc = fmaf(a, a, ssc);
                const float* wr = Ws + (wi * 16 + e) * CP;
#pragma unroll
                for (int k = 0; k < CP; k += 4) {                 // the same broadcast
                    const float4 t4 = *reinterpret_cast<const float4*>(wr + k);
                    acc[k] = fmaf(a, t4.x, acc[k]); acc[k + 1] = fmaf(a, t4.y, acc[k + 1]);
                    acc[k + 2] = fmaf(a, t4.z, acc[k + 2]); acc[k + 3] = fmaf(a, t4.w, acc[k + 3]);
                }
            }
        }
        ss += (double)ssc;
    }
    // the block's slab [CP + 3][256]: every lane writes (a lane past the list wrote zeros; the fold never reads it)
    float* out = part + ((int64_t)range * tiles + tile) * ((CP + 3) * RP_TILE) + t;
#pragma unroll
    for (int i = 0; i < CP; ++i) out[i * RP_TILE] = acc[i];
    out[CP * RP_TILE] = __int_as_float(__double2loint(ss));
    out[(CP + 1) * RP_TILE] = __int_as_float(__double2hiint(ss));
    out[(CP + 2) * RP_TILE] = __int_as_float(n);
}

// One thread per sample s < b: the ranges' partials in range order in float64, Y rounded once; pad columns +0.0
__global__ __launch_bounds__(256) void resid_project_fold_kernel(const float* __restrict__ part, const int ranges, const int tiles, const int b,
                                                                 const int C, const int CP, float* __restrict__ Y, double* __restrict__ ss,
                                                                 int32_t* __restrict__ nobs) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= b) return;
    const int64_t slab = (int64_t)(CP + 3) * RP_TILE, per_range = (int64_t)tiles * slab;
    const float* base = part + (s / RP_TILE) * slab + (s % RP_TILE);
    for (int c0 = 0; c0 < CP; c0 += 4) {
        float v[4];
        for (int i = 0; i < 4; ++i) {
            double sum = 0.0;
            for (int r = 0; r < ranges; ++r) sum += (double)base[r * per_range + (int64_t)(c0 + i) * RP_TILE];
            v[i] = c0 + i < C ? (float)sum : 0.f;
        }
        *reinterpret_cast<float4*>(Y + s * CP + c0) = make_float4(v[0], v[1], v[2], v[3]);
    }
    double sq = 0.0;
    int n = 0;
    for (int r = 0; r < ranges; ++r) {
        const float* src = base + r * per_range + (int64_t)CP * RP_TILE;
        sq += __hiloint2double(__float_as_int(src[RP_TILE]), __float_as_int(src[0]));
        n += __float_as_int(src[2 * RP_TILE]);
    }
    ss[s] = sq;
    nobs[s] = n;
}

// The transposed product's operand image: row s = (q_s [KP] | Yin_s [CP]), one thread per float4
__global__ __launch_bounds__(256) void resid_pack_kernel(const float* __restrict__ Q, const int q_stride, const float* __restrict__ Yin,
                                                         const int b, const int KP, const int CP, float* __restrict__ img) {
    const int row4 = (KP + CP) / 4;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)b * row4) return;
    const int64_t s = e / row4;
    const int f = (int)(e - s * row4);
    const float* src = f < KP / 4 ? Q + s * q_stride + 4 * f : Yin + s * CP + 4 * (f - KP / 4);
    reinterpret_cast<float4*>(img)[e] = *reinterpret_cast<const float4*>(src);
}

template <int KP, int CP>
__global__ __launch_bounds__(SWEEP_CHUNK) void resid_project_t_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ img, const float eps, const float one_m_eps, const float pimin,
    const float one_m_pimin, const int slices, const int tiles_per_slice, const int64_t Mp, float* __restrict__ part) {
    const SweepPos pos = sweep_pos(slices);
    float p[KP];
    sweep_load_p<KP>(P, pos.j, M, p);
    float acc[CP];
#pragma unroll
    for (int i = 0; i < CP; ++i) acc[i] = 0.f;
    int n = 0;

    snp_sweep<KP + CP>(pos, xp, ld, idx, b, M, img, KP + CP, tiles_per_slice, [&](const uint32_t code, const float* qr) {
        uint32_t m = obs_mask(code);
        float pi = 0.f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {                       // a broadcast: the row is read once, four columns at a time
            const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
            pi = fmaf(t4.x, p[k], pi); pi = fmaf(t4.y, p[k + 1], pi);
            pi = fmaf(t4.z, p[k + 2], pi); pi = fmaf(t4.w, p[k + 3], pi);
        }
        const float a = resid_term(pi, code, m, eps, one_m_eps, pimin, one_m_pimin);
        n += (int)(m & 1u);
#pragma unroll
        for (int k = 0; k < CP; k += 4) {                       // the sample's Yin row behind its q row
            const float4 t4 = *reinterpret_cast<const float4*>(qr + KP + k);
            acc[k] = fmaf(a, t4.x, acc[k]); acc[k + 1] = fmaf(a, t4.y, acc[k + 1]);
            acc[k + 2] = fmaf(a, t4.z, acc[k + 2]); acc[k + 3] = fmaf(a, t4.w, acc[k + 3]);
        }
    });

    float* out = part + (int64_t)pos.slice * (CP + 1) * Mp + pos.j;
#pragma unroll
    for (int i = 0; i < CP; ++i) out[(int64_t)i * Mp] = acc[i];
    out[(int64_t)CP * Mp] = __int_as_float(n);
}

// One thread per SNP j < M: the slices' partials in slice order in float64, rounded once; pad columns +0.0
__global__ __launch_bounds__(256) void resid_project_t_fold_kernel(const float* __restrict__ part, const int slices, const int64_t Mp,
                                                                   const int64_t M, const int C, const int CP, float* __restrict__ O,
                                                                   int32_t* __restrict__ nobs_snp) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int64_t plane = (int64_t)(CP + 1) * Mp;
    for (int c0 = 0; c0 < CP; c0 += 4) {
        float v[4];
        for (int i = 0; i < 4; ++i) {
            double sum = 0.0;
            for (int s = 0; s < slices; ++s) sum += (double)part[s * plane + (int64_t)(c0 + i) * Mp + j];
            v[i] = c0 + i < C ? (float)sum : 0.f;
        }
        *reinterpret_cast<float4*>(O + j * CP + c0) = make_float4(v[0], v[1], v[2], v[3]);
    }
    int n = 0;
    for (int s = 0; s < slices; ++s) n += __float_as_int(part[s * plane + (int64_t)CP * Mp + j]);
    nobs_snp[j] = n;
}

static bool rp_shape_ok(int b, int64_t M) { return b > 0 && M > 0; }
static bool rp_kp_ok(int kp) { return kp >= 4 && kp <= RP_MAX_KP && kp % 4 == 0; }
static bool rp_cp_ok(int CP) { return CP == 16 || CP == 32; }
// the forward product's launch shape, a rule of (b, M) alone
static RangePlan rp_plan(int b, int64_t M) { return range_plan(M, range_tiles(b, RP_TILE), RP_BLOCKS, RP_MAX_CHUNKS); }

// what both entries refuse in the same words, before anything is launched
static int rp_check(const char* who, const void* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, int32_t k, int32_t kp,
                    int32_t q_stride, float eps, float pimin, int32_t C, int32_t CP) {
    if (b <= 0 || M <= 0) return failf(who, "empty block (need b > 0 and M > 0)");
    if (check_packed(who, ld, M) || check_head(who, k, kp, q_stride) || check_eps(who, eps)) return 1;
    if (!(pimin >= 0.f && pimin < 0.5f)) return failf(who, "pimin must be in [0, 0.5)");
    if (kp > RP_MAX_KP) return failf(who, "K must be <= 16 (a row of q or p lives in one thread's registers beside the column sums)");
    if (!rp_cp_ok(CP)) return failf(who, "CP must be 16 or 32");
    if (C < 1 || C > CP) return failf(who, "C must be in 1..CP");
    if (((uintptr_t)xp & 15) != 0 || ((uintptr_t)idx & 3) != 0) return failf(who, "xp must be 16-byte and idx 4-byte aligned");
    return 0;
}

// f(KP, CP) as integral constants for kp in {4, 8, 12, 16} and CP in {16, 32} (both checked before)
template <class F>
static void rp_dispatch(int kp, int CP, F&& f) {
    dispatch_int<4, 8, 12, 16>(kp, [&](auto KP) {
        dispatch_int<16, 32>(CP, [&](auto CPc) { f(KP, CPc); });
    });
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_resid_project_chunks(int32_t b, int64_t M) { return rp_shape_ok(b, M) ? range_count(rp_plan(b, M).cpr) : 0; }
extern "C" int32_t nadm_resid_project_ranges(int32_t b, int64_t M) { return rp_shape_ok(b, M) ? range_count(rp_plan(b, M).ranges) : 0; }

// scratch: the partials [ranges][tiles][CP + 3][256] (CP fp32 sums, ss as the two halves of a double, n as int32)
extern "C" int64_t nadm_resid_project_scratch_floats(int32_t b, int64_t M, int32_t CP) {
    return rp_shape_ok(b, M) && rp_cp_ok(CP) ? rp_plan(b, M).blocks_bound * ((CP + 3) * RP_TILE) : 0;
}

extern "C" int32_t nadm_resid_project_t_slices(int32_t b, int64_t M) { return rp_shape_ok(b, M) ? sweep_slices(b, M) : 0; }

// scratch: the operand image [b][kp + CP], then the partials [slices][CP + 1][Mp] (CP fp32 sums and n as int32), Mp = 256 chunks
extern "C" int64_t nadm_resid_project_t_scratch_floats(int32_t b, int64_t M, int32_t kp, int32_t CP) {
    if (!rp_shape_ok(b, M) || !rp_kp_ok(kp) || !rp_cp_ok(CP)) return 0;
    return (int64_t)b * (kp + CP) + sweep_rows_bound(b, M) * (CP + 1);
}

extern "C" int nadm_resid_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k,
                                  int32_t kp, const float* Q, int32_t q_stride, float eps, float pimin, const float* W, int32_t C,
                                  int32_t CP, float* Y, double* ss, int32_t* nobs, float* scratch, void* stream) {
    const char* who = "nadm_resid_project";
    if (!xp || !P || !Q || !W || !Y || !ss || !nobs || !scratch) return failf(who, "null pointer");
    if (rp_check(who, xp, ld, idx, b, M, k, kp, q_stride, eps, pimin, C, CP)) return 1;
    if ((((uintptr_t)P | (uintptr_t)Q | (uintptr_t)W | (uintptr_t)Y | (uintptr_t)scratch) & 15) != 0)
        return failf(who, "P, Q, W, Y and scratch must be 16-byte aligned");
    if (((uintptr_t)ss & 7) != 0 || ((uintptr_t)nobs & 3) != 0) return failf(who, "ss must be 8-byte and nobs 4-byte aligned");
    const RangePlan pl = rp_plan(b, M);
    if (range_launch_check(who, pl)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - eps, omp = 1.f - pimin;
    rp_dispatch(kp, CP, [&](auto KP, auto CPc) {
        hipLaunchKernelGGL((resid_project_kernel<decltype(KP)::value, decltype(CPc)::value>), range_grid(pl), dim3(RP_TILE), 0, st, xp, ld, idx,
                           b, M, P, Q, q_stride, eps, ome, pimin, omp, W, (int)pl.tiles, pl.cpr, pl.chunks, scratch);
    });
    if (int e = check_launch("resid_project (accumulate)")) return e;
    hipLaunchKernelGGL(resid_project_fold_kernel, fold_grid(b), dim3(256), 0, st, scratch, (int)pl.ranges, (int)pl.tiles, b, C, CP, Y, ss, nobs);
    return check_launch("resid_project (fold)");
}

extern "C" int nadm_resid_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k,
                                    int32_t kp, const float* Q, int32_t q_stride, float eps, float pimin, const float* Yin, int32_t C,
                                    int32_t CP, float* O, int32_t* nobs_snp, float* scratch, void* stream) {
    const char* who = "nadm_resid_project_t";
    if (!xp || !P || !Q || !Yin || !O || !nobs_snp || !scratch) return failf(who, "null pointer");
    if (rp_check(who, xp, ld, idx, b, M, k, kp, q_stride, eps, pimin, C, CP)) return 1;
    if ((((uintptr_t)P | (uintptr_t)Q | (uintptr_t)Yin | (uintptr_t)O | (uintptr_t)scratch) & 15) != 0)
        return failf(who, "P, Q, Yin, O and scratch must be 16-byte aligned");
    if (((uintptr_t)nobs_snp & 3) != 0) return failf(who, "nobs_snp must be 4-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    const int64_t img4 = (int64_t)b * ((kp + CP) / 4);
    if (chunks * slices > 0x7FFFFFFFll || (img4 + 255) / 256 > 0x7FFFFFFFll) return failf(who, "too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    float* img = scratch;
    float* part = scratch + (int64_t)b * (kp + CP);
    hipLaunchKernelGGL(resid_pack_kernel, fold_grid(img4), dim3(256), 0, st, Q, q_stride, Yin, b, kp, CP, img);
    if (int e = check_launch("resid_project_t (operand image)")) return e;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps, omp = 1.f - pimin;
    rp_dispatch(kp, CP, [&](auto KP, auto CPc) {
        hipLaunchKernelGGL((resid_project_t_kernel<decltype(KP)::value, decltype(CPc)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld,
                           idx, b, M, P, img, eps, ome, pimin, omp, slices, tps, Mp, part);
    });
    if (int e = check_launch("resid_project_t (accumulate)")) return e;
    hipLaunchKernelGGL(resid_project_t_fold_kernel, dim3((unsigned)chunks), dim3(256), 0, st, part, slices, Mp, M, C, CP, O, nobs_snp);
    return check_launch("resid_project_t (fold)");
}
