// Cross-validation over held-out genotype CALLS (include/nadm.h: the fold of a call, nadm_cv_mask, nadm_cv_deviance).
//
//   cv_mask_kernel          a plain vector kernel: a thread owns 16 bytes = 64 calls of a row (one 16-byte load, one 16-byte store)
//                           and walks the rows of its grid row.  An observed call of the fold becomes code 3; every other bit is
//                           copied.  Exact; in place is allowed (a thread reads its 16 bytes before it writes them).
//   cv_deviance_accum_kernel  the SNP-owner sweep of nadm_snp_sweep.h, as snp_hwe_accum_kernel: a thread's p row and two running sums
//                           (the deviance in log2 units in fp32, the number of held-out calls in int32) live in registers.  Per
//                           genotype: KP multiply-adds, one cv_mix32, one multiply-high, two v_log_f32.  The body keeps the matrix row
//                           of its sample (uniform over the block).  A call that is missing, not of the fold, of a row >= b or of a
//                           SNP >= M enters both sums as exactly +0.0f / 0.  Writes the slice's partials, 8 bytes per SNP.
//   cv_deviance_fold_kernel one thread per SNP: adds the slices' partials in slice order in float64 and applies 2 ln 2 once.
// No floating-point atomics: two calls on the same inputs give the same bits.
#include "nadm_cv_fold.h"
#include "nadm_snp_sweep.h"

namespace nadm {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void cv_mask_kernel(const uint8_t* xp, const int64_t ld, const int64_t rows, const int64_t row0,
                                                      const int64_t M, const uint64_t seed, const uint32_t folds, const uint32_t fold,
                                                      uint8_t* xo) {
    const int64_t piece = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 16-byte piece of a row: SNPs 64 piece .. 64 piece + 63
    if (piece * 16 >= ld) return;                                       // (ld % 16 == 0: a piece is inside the row or past its end)
    const int64_t j0 = piece * 64;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint32_t key = cv_row_key(seed, (uint32_t)(row0 + r));    // uniform over the block
        u32x4_t v = *reinterpret_cast<const u32x4_t*>(xp + r * ld + 16 * piece);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t x = v[w];
            uint32_t blank = 0u;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int64_t j = j0 + 16 * w + s;                      // SNP j: byte j / 4, bits 2 (j % 4) ..
                const uint32_t hit = obs_mask((x >> (2 * s)) & 3u) & lt_mask64(j, M) & cv_held_mask(key, (uint32_t)j, folds, fold);
                blank |= (hit & 3u) << (2 * s);
            }
            v[w] = x | blank;
        }
        *reinterpret_cast<u32x4_t*>(xo + r * ld + 16 * piece) = v;
    }
}

template <int KP>
__global__ __launch_bounds__(SWEEP_CHUNK) void cv_deviance_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int b, const int64_t M, const float* __restrict__ P,
    const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps, const uint64_t seed, const uint32_t row0,
    const uint32_t folds, const uint32_t fold, const int slices, const int tiles_per_slice, const int64_t Mp,
    u32x2_t* __restrict__ part) {
    const SweepPos pos = sweep_pos(slices);
    float p[KP];
    sweep_load_p<KP>(P, pos.j, M, p);
    float S = 0.f;
    int n = 0;
    const uint32_t j = (uint32_t)pos.j;                                 // (a SNP >= M comes as code 3 whatever its fold)
    uint32_t row = row0 + (uint32_t)(SWEEP_TILE * tiles_per_slice) * (uint32_t)pos.slice;      // the body's own row counter

    snp_sweep<KP>(pos, xp, ld, nullptr, b, M, Q, q_stride, tiles_per_slice, [&](const uint32_t code, const float* qr) {
        const uint32_t m = obs_mask(code) & cv_held_mask(cv_row_key(seed, row), j, folds, fold);
        ++row;
        uint32_t m1 = (uint32_t)((int)((code ^ 1u) - 1u) >> 31);        // g == 1 ? ~0 : 0
        asm("" : "+v"(m1));
        float pi = 0.f;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(qr + k);
            pi = fmaf(t4.x, p[k], pi); pi = fmaf(t4.y, p[k + 1], pi);
            pi = fmaf(t4.z, p[k + 2], pi); pi = fmaf(t4.w, p[k + 3], pi);
        }
        // 1 - pi from the UNCLIPPED product, as em_terms (nadm_common.h)
        const float r = fminf(fmaxf(pi, eps), one_m_eps);
        const float u = fminf(fmaxf(1.f - pi, eps), one_m_eps);
        const float g = (float)code;
        // log2 units (v_log_f32); the heterozygote's 4 ln 2 is 2 of them: a call at pi = 1/2 gives -1 - 1 + 2 = 0 exactly
        const float s = (g * __log2f(r) + (2.f - g) * __log2f(u)) + __uint_as_float(0x40000000u & m1);
        S += keepf(s, m);                                               // masked: exactly +0.0f
        n += (int)(m & 1u);
    });

    part[(int64_t)pos.slice * Mp + pos.j] = (u32x2_t){__float_as_uint(S), (uint32_t)n};
}

// One thread per SNP j < M: the slices' partials in slice order, the deviance in float64, the count as an integer
__global__ __launch_bounds__(256) void cv_deviance_fold_kernel(const u32x2_t* __restrict__ part, const int slices, const int64_t Mp,
                                                               const int64_t M, double* __restrict__ dev, int32_t* __restrict__ nheld) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double s = 0.0;
    int n = 0;
    for (int sl = 0; sl < slices; ++sl) {
        const u32x2_t v = part[(int64_t)sl * Mp + j];
        s += (double)__uint_as_float(v[0]);
        n += (int)v[1];
    }
    dev[j] = 1.3862943611198906 * (0.0 - s);                           // 2 ln 2, once; 0 - s: no held-out call gives +0.0
    nheld[j] = n;
}

}  // namespace nadm

using namespace nadm;

extern "C" int nadm_cv_mask(const uint8_t* xp, int64_t ld, int64_t rows, int64_t row0, int64_t M, uint64_t seed, int32_t folds,
                            int32_t fold, uint8_t* xo, void* stream) {
    if (!xp || !xo) return fail("nadm_cv_mask: null pointer");
    if (rows <= 0 || M <= 0) return fail("nadm_cv_mask: empty block (need rows > 0 and M > 0)");
    if (check_packed("nadm_cv_mask", ld, M) || check_cv_fold("nadm_cv_mask", row0, rows, M, folds, fold)) return 1;
    if ((((uintptr_t)xp | (uintptr_t)xo) & 15) != 0) return fail("nadm_cv_mask: xp and xo must be 16-byte aligned");
    const uintptr_t a = (uintptr_t)xp, o = (uintptr_t)xo, bytes = (uintptr_t)rows * (uintptr_t)ld;
    if (a != o && a < o + bytes && o < a + bytes) return fail("nadm_cv_mask: xo overlaps xp (only xo == xp is allowed)");
    const int64_t gx = (ld / 16 + 255) / 256;
    if (gx > 0x7FFFFFFFll) return fail("nadm_cv_mask: too many blocks for one launch");
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    hipLaunchKernelGGL(cv_mask_kernel, dim3((unsigned)gx, gy), dim3(256), 0, (hipStream_t)stream, xp, ld, rows, row0, M, seed,
                       (uint32_t)folds, (uint32_t)fold, xo);
    return check_launch("cv_mask");
}

extern "C" int32_t nadm_cv_deviance_slices(int32_t b, int64_t M) { return (b <= 0 || M <= 0) ? 0 : sweep_slices(b, M); }

// scratch: the partials [slices, Mp] x { deviance in log2 units (fp32), nheld (int32) }, Mp = 256 chunks
extern "C" int64_t nadm_cv_deviance_scratch_floats(int32_t b, int64_t M) {
    return (b <= 0 || M <= 0) ? 0 : sweep_rows_bound(b, M) * 2;
}

extern "C" int nadm_cv_deviance(const uint8_t* xp, int64_t ld, int32_t b, int64_t row0, int64_t M, const float* Q, int32_t q_stride,
                                int32_t k, int32_t kp, const float* P, float eps, uint64_t seed, int32_t folds, int32_t fold,
                                double* dev, int32_t* nheld, float* scratch, void* stream) {
    if (!xp || !Q || !P || !dev || !nheld || !scratch) return fail("nadm_cv_deviance: null pointer");
    if (b <= 0 || M <= 0) return fail("nadm_cv_deviance: empty block (need b > 0 and M > 0)");
    if (check_packed("nadm_cv_deviance", ld, M) || check_head("nadm_cv_deviance", k, kp, q_stride) || check_eps("nadm_cv_deviance", eps) ||
        check_cv_fold("nadm_cv_deviance", row0, b, M, folds, fold))
        return 1;
    if ((((uintptr_t)xp | (uintptr_t)Q | (uintptr_t)P | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_cv_deviance: xp, Q, P and scratch must be 16-byte aligned");
    if (((uintptr_t)dev & 7) != 0 || ((uintptr_t)nheld & 3) != 0) return fail("nadm_cv_deviance: dev must be 8-byte and nheld 4-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll) return fail("nadm_cv_deviance: too many blocks for one launch");
    u32x2_t* part = reinterpret_cast<u32x2_t*>(scratch);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    const float ome = 1.f - eps;
    if (int e = dispatch_kp("nadm_cv_deviance", kp, [&](auto KP) {
            hipLaunchKernelGGL((cv_deviance_accum_kernel<decltype(KP)::value>), dim3(grid), dim3(SWEEP_CHUNK), 0, st, xp, ld, b, M, P, Q,
                               q_stride, eps, ome, seed, (uint32_t)row0, (uint32_t)folds, (uint32_t)fold, slices, tps, Mp, part);
        }))
        return e;
    if (int e = check_launch("cv_deviance (accumulate)")) return e;
    hipLaunchKernelGGL(cv_deviance_fold_kernel, dim3((unsigned)chunks), dim3(256), 0, st, part, slices, Mp, M, dev, nheld);
    return check_launch("cv_deviance (fold)");
}
