// LD pruning on the packed matrix (include/nadm.h: nadm_snp_counts, nadm_ld_band, nadm_select_snps).
//
//   ld_band_kernel     r^2 of every SNP with its next W neighbours: a banded Gram product over the SAMPLE axis on
//                      v_mfma_i32_16x16x64_i8.  Per side a SNP enters as three int8 pieces -- o (call observed), g o and g^2 o -- and
//                      the six moments of a pair are six products of a piece of a with a piece of b, accumulated in int32: exact.
//                      One 256-thread block owns 64 "a" SNPs (one 16-SNP tile per wave) and up to 8 of the "b" tiles each of them needs
//                      (tiles at .. at + 7 + 8 gy of the wave's tile at; blockIdx.y = gy walks the rest of a wide window), and runs
//                      over all samples in steps of 64 = the K of the instruction.  The matrix is sample-major, the instruction wants
//                      the samples along k: per step the block
//                        STAGES   64 samples x (16 + up to 48) bytes of their rows (one 16-byte load per thread, the next step's issued
//                                 under this step's work) into LDS TRANSPOSED, [byte column][sample]; rows past `rows`, SNPs >= M and
//                                 pad bits are overwritten with the missing code here, so everything behind sees them as exactly 0;
//                        EXPANDS  one dword of that (4 samples of one byte column) into the 4 SNPs x 3 pieces it holds with byte-lane
//                                 arithmetic and writes the operand image [piece][SNP][64 samples], one 80-byte row per SNP;
//                        MULTIPLIES lane l reads 16 bytes = samples 16 (l >> 4) .. + 15 of SNP l & 15 of a tile.  Both operands are read
//                                 with the same lane -> sample rule, and the instruction sums over k, so the order of the samples
//                                 within a step does not matter.
//                      Epilogue: r^2 from the int32 sums in int64 / float64, one pair per accumulator register.
//   snp_counts_kernel  a plain vector kernel: one thread per 16 SNPs (a dword of a row), row slices added with integer atomics.
//   select_snps_kernel one thread per output byte column: gathers its four SNPs' codes row by row.
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int LD_TA = 64;                 // "a" SNPs per block: 4 tiles of 16, one per wave = 16 bytes of a packed row
constexpr int LD_KS = 64;                 // samples per step = K of the instruction
constexpr int LD_NBG = 8;                 // "b" tiles per "a" tile whose accumulators one block holds (8 x 6 x 4 = 192 registers)
constexpr int LD_BT = LD_NBG + 3;         // "b" tiles of the image: wave 3's last is tile 3 + 7
constexpr int LD_SNPS = LD_TA + 16 * LD_BT;        // SNP rows of the operand image (240)
constexpr int LD_ROW = 80;                // bytes per image row: 64 samples + 16 (a dword column of four SNP groups then spreads over the banks)
constexpr int LD_RAWC = 64;               // byte columns of the transposed stage: 16 of "a", 48 of "b"

__global__ __launch_bounds__(256, 2) void ld_band_kernel(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                                         const int rows, const int64_t M, const int64_t m0, const int64_t m1, const int W,
                                                         const int nb_tiles, double* __restrict__ r2, int32_t* __restrict__ mom) {
    __shared__ __attribute__((aligned(16))) uint8_t rawT[LD_RAWC * LD_KS];
    __shared__ __attribute__((aligned(16))) uint8_t Img[3 * LD_SNPS * LD_ROW];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int gy = (int)blockIdx.y;
    const int64_t j0 = (m0 / LD_TA + blockIdx.x) * LD_TA;         // first "a" SNP of the block
    const int64_t jb0 = j0 + (int64_t)16 * LD_NBG * gy;           // first SNP of the "b" part of the image
    const int nbg = min(LD_NBG, nb_tiles - LD_NBG * gy);          // "b" tiles per wave in this block (>= 1)
    const int btiles = nbg + 3;                                   // "b" tiles of the image in use
    const int ncols = 16 + 4 * btiles;                            // byte columns of the stage in use

    // stager role: sample s of the step, 16-byte piece `part` (0: the "a" bytes, 1..3: the "b" bytes)
    const int s = t & 63, part = t >> 6;
    const int64_t js = part == 0 ? j0 : jb0 + 64 * (part - 1);    // first SNP of the piece
    const bool part_used = 16 * part < ncols;
    // a piece past the row's end holds SNPs >= 4 ld >= M only: its offset is clamped, every field is overwritten below
    const int64_t off = min(js / 4, ld - 16);
    uint32_t tail[4];                                             // ones in the fields of SNPs >= M
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int64_t left = M - (js + 16 * d);
        tail[d] = left >= 16 ? 0u : (left <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (2 * (int)left));
    }
    auto load_step = [&](const int step, u32x4_t& v) {
        const int pos = step * LD_KS + s;
        const int posc = min(pos, rows - 1);
        const int64_t row = idx ? idx[posc] : posc;
        v = *reinterpret_cast<const u32x4_t*>(xp + row * ld + off);
        const uint32_t gone = pos < rows ? 0u : 0xFFFFFFFFu;      // a row past the list: every call missing
#pragma unroll
        for (int d = 0; d < 4; ++d) v[d] |= tail[d] | gone;
    };

    i32x4_t acc[LD_NBG][6];
#pragma unroll
    for (int tt = 0; tt < LD_NBG; ++tt)
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[tt][q] = (i32x4_t){0, 0, 0, 0};

    const int steps = (rows + LD_KS - 1) / LD_KS;
    u32x4_t nxt = (u32x4_t){0u, 0u, 0u, 0u};
    if (part_used) load_step(0, nxt);

#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
        // ---- stage, transposed: byte i of the piece -> [16 part + i][s]
        if (part_used) {
#pragma unroll
            for (int i = 0; i < 16; ++i) rawT[(16 * part + i) * LD_KS + s] = (uint8_t)(nxt[i >> 2] >> (8 * (i & 3)));
            load_step(min(step + 1, steps - 1), nxt);
        }
        __syncthreads();
        // ---- expand: (byte column c, samples 4 q .. 4 q + 3) -> 4 SNPs x 3 pieces, a dword each
        for (int e = t; e < ncols * 16; e += 256) {
            const int c = e >> 4, q = e & 15;
            const uint32_t r = reinterpret_cast<const uint32_t*>(rawT)[c * 16 + q];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t x = (r >> (2 * i)) & 0x03030303u;              // the codes of SNP 4 c + i, a sample per byte
                const uint32_t miss = x & (x >> 1) & 0x01010101u;             // 1 where the code is 3
                const uint32_t o = miss ^ 0x01010101u;
                const uint32_t g = x ^ (miss * 3u);                           // 0, 1, 2; 0 where missing
                const uint32_t g2 = (g & 0x01010101u) | ((g & 0x02020202u) << 1);      // 0, 1, 4
                uint32_t* dst = reinterpret_cast<uint32_t*>(Img + (4 * c + i) * LD_ROW) + q;
                dst[0] = o;
                dst[LD_SNPS * LD_ROW / 4] = g;
                dst[2 * LD_SNPS * LD_ROW / 4] = g2;
            }
        }
        __syncthreads();
        // ---- multiply: lane l is SNP l & 15 of its tile and samples 16 (l >> 4) .. + 15 of the step, for both operands
        {
            const uint8_t* ia = Img + (16 * w + (lane & 15)) * LD_ROW + 16 * (lane >> 4);
            const i32x4_t ao = *reinterpret_cast<const i32x4_t*>(ia);
            const i32x4_t ag = *reinterpret_cast<const i32x4_t*>(ia + LD_SNPS * LD_ROW);
            const i32x4_t ag2 = *reinterpret_cast<const i32x4_t*>(ia + 2 * LD_SNPS * LD_ROW);
#pragma unroll
            for (int tt = 0; tt < LD_NBG; ++tt) {
                if (tt < nbg) {                                               // (the same in every lane)
                    const uint8_t* ib = Img + (LD_TA + 16 * (w + tt) + (lane & 15)) * LD_ROW + 16 * (lane >> 4);
                    const i32x4_t bo = *reinterpret_cast<const i32x4_t*>(ib);
                    const i32x4_t bg = *reinterpret_cast<const i32x4_t*>(ib + LD_SNPS * LD_ROW);
                    const i32x4_t bg2 = *reinterpret_cast<const i32x4_t*>(ib + 2 * LD_SNPS * LD_ROW);
                    acc[tt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bo, acc[tt][0], 0, 0, 0);       // n
                    acc[tt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bo, acc[tt][1], 0, 0, 0);       // Sa
                    acc[tt][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bg, acc[tt][2], 0, 0, 0);       // Sb
                    acc[tt][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bg, acc[tt][3], 0, 0, 0);       // Sab
                    acc[tt][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag2, bo, acc[tt][4], 0, 0, 0);      // Saa
                    acc[tt][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bg2, acc[tt][5], 0, 0, 0);      // Sbb
                }
            }
        }
        // (the next step's stage is written after the barrier above, its image after the barrier below it: no third barrier)
    }

    // D: column = lane & 15 = the "b" SNP of the tile, rows 4 (lane >> 4) + i = the "a" SNP
#pragma unroll
    for (int tt = 0; tt < LD_NBG; ++tt) {
        if (tt >= nbg) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t ja = j0 + 16 * w + 4 * (lane >> 4) + i;
            const int64_t jb = jb0 + 16 * (w + tt) + (lane & 15);
            const int64_t d = jb - ja - 1;
            if (ja < m0 || ja >= m1 || d < 0 || d >= W) continue;
            const int64_t n = acc[tt][0][i], Sa = acc[tt][1][i], Sb = acc[tt][2][i], Sab = acc[tt][3][i], Saa = acc[tt][4][i],
                          Sbb = acc[tt][5][i];
            const int64_t cov = n * Sab - Sa * Sb, va = n * Saa - Sa * Sa, vb = n * Sbb - Sb * Sb;
            double v = 0.0;
            if (va != 0 && vb != 0) {
                const double num = (double)cov * (double)cov;
                const double den = (double)va * (double)vb;
                v = num / den;
            }
            const int64_t o = (ja - m0) * W + d;
            r2[o] = v;
            if (mom) {
                int32_t* mo = mom + o * 6;
                mo[0] = (int32_t)n; mo[1] = (int32_t)Sa; mo[2] = (int32_t)Sb; mo[3] = (int32_t)Sab; mo[4] = (int32_t)Saa; mo[5] = (int32_t)Sbb;
            }
        }
    }
}

// thread = dword `wd` of a row (16 SNPs), block row = a slice of the listed rows; counts of the codes 1, 2 and 3 per SNP
__global__ __launch_bounds__(256) void snp_counts_kernel(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                                         const int rows, const int64_t M, const int64_t words, const int rows_per_slice,
                                                         int32_t* __restrict__ cnt) {
    const int64_t wd = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (wd >= words) return;
    const int r0 = (int)blockIdx.y * rows_per_slice, r1 = min(rows, r0 + rows_per_slice);
    int c1[16], c2[16], c3[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) c1[e] = c2[e] = c3[e] = 0;
    for (int r = r0; r < r1; ++r) {
        const int64_t row = idx ? idx[r] : r;
        const uint32_t x = *reinterpret_cast<const uint32_t*>(xp + row * ld + 4 * wd);
        const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
        const uint32_t one = lo & ~hi, two = hi & ~lo, three = lo & hi;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            c1[e] += (int)((one >> (2 * e)) & 1u);
            c2[e] += (int)((two >> (2 * e)) & 1u);
            c3[e] += (int)((three >> (2 * e)) & 1u);
        }
    }
    const int nr = max(r1 - r0, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t j = 16 * wd + e;
        if (j < M) {
            atomicAdd(cnt + 3 * j, nr - c3[e]);
            atomicAdd(cnt + 3 * j + 1, c1[e] + 2 * c2[e]);
            atomicAdd(cnt + 3 * j + 2, c1[e] + 4 * c2[e]);
        }
    }
}

// thread = output byte column c; blockIdx.y strides over the rows
__global__ __launch_bounds__(256) void select_snps_kernel(const uint8_t* __restrict__ xp, const int64_t ld_in, const int64_t rows,
                                                          const int64_t* __restrict__ keep, const int64_t M_out, const int flip,
                                                          uint8_t* __restrict__ out, const int64_t ld_out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ld_out) return;
    int64_t byte_in[4];
    int sh[4];
    uint32_t valid[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t jo = 4 * c + i;
        valid[i] = jo < M_out ? 3u : 0u;
        int64_t k = jo < M_out ? keep[jo] : 0;
        k = min(max(k, (int64_t)0), 4 * ld_in - 1);             // (a value outside the row is the caller's error; it is not followed)
        byte_in[i] = k >> 2;
        sh[i] = 2 * (int)(k & 3);
    }
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint8_t* src = xp + r * ld_in;
        uint32_t b = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t code = (src[byte_in[i]] >> sh[i]) & 3u;
            if (flip) code ^= (~code & 1u) << 1;                 // 0 <-> 2; 1 and 3 stay
            b |= (code & valid[i]) << (2 * i);
        }
        out[r * ld_out + c] = (uint8_t)b;
    }
}

static int ld_common_checks(const char* who, const void* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M) {
    if (rows < 1 || rows > (1ll << 24)) return failf(who, "rows must be in 1..2^24");
    if (M < 1) return failf(who, "M must be >= 1");
    if (check_packed(who, ld, M)) return 1;
    if (((uintptr_t)xp & 15) != 0) return failf(who, "xp must be 16-byte aligned");
    if (((uintptr_t)idx & 3) != 0) return failf(who, "idx must be 4-byte aligned");
    return 0;
}

}  // namespace nadm

using namespace nadm;

extern "C" int nadm_snp_counts(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int32_t* cnt, void* stream) {
    if (!xp || !cnt) return fail("nadm_snp_counts: null pointer");
    if (ld_common_checks("nadm_snp_counts", xp, ld, idx, rows, M)) return 1;
    if (((uintptr_t)cnt & 3) != 0) return fail("nadm_snp_counts: cnt must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(cnt, 0, (size_t)M * 3 * sizeof(int32_t), st) != hipSuccess) return fail("nadm_snp_counts: hipMemsetAsync failed");
    const int64_t words = (M + 15) / 16, gx = (words + 255) / 256;
    // row slices: enough blocks to fill the chip while a slice keeps at least 64 rows
    int64_t slices = (1024 + gx - 1) / gx;
    const int64_t most = (rows + 63) / 64;
    if (slices > most) slices = most;
    if (slices > 65535) slices = 65535;
    const int rps = (int)((rows + slices - 1) / slices);
    slices = (rows + rps - 1) / rps;
    if (gx > 0x7FFFFFFFll) return fail("nadm_snp_counts: too many blocks for one launch");
    hipLaunchKernelGGL(snp_counts_kernel, dim3((unsigned)gx, (unsigned)slices), dim3(256), 0, st, xp, ld, idx, (int)rows, M, words, rps, cnt);
    return check_launch("snp_counts");
}

extern "C" int nadm_ld_band(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int64_t m0, int64_t m1, int32_t W,
                            double* r2, int32_t* mom, void* stream) {
    if (!xp || !r2) return fail("nadm_ld_band: null pointer");
    if (ld_common_checks("nadm_ld_band", xp, ld, idx, rows, M)) return 1;
    if (W < 1 || W > NADM_LD_MAX_WINDOW) return fail("nadm_ld_band: W must be in 1..NADM_LD_MAX_WINDOW");
    if (m0 < 0 || m0 >= m1 || m1 > M) return fail("nadm_ld_band: need 0 <= m0 < m1 <= M");
    if (((uintptr_t)r2 & 7) != 0 || ((uintptr_t)mom & 3) != 0) return fail("nadm_ld_band: r2 must be 8-byte and mom 4-byte aligned");
    const int nb_tiles = (W + 15) / 16 + 1;                       // "b" tiles an "a" tile meets: its own and the next ceil(W / 16)
    const int64_t gx = (m1 - 1) / LD_TA - m0 / LD_TA + 1;
    const int gy = (nb_tiles + LD_NBG - 1) / LD_NBG;
    if (gx > 0x7FFFFFFFll) return fail("nadm_ld_band: too many blocks for one launch");
    hipLaunchKernelGGL(ld_band_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, xp, ld, idx, (int)rows, M, m0,
                       m1, (int)W, nb_tiles, r2, mom);
    return check_launch("ld_band");
}

extern "C" int nadm_select_snps(const uint8_t* xp, int64_t ld_in, int64_t rows, const int64_t* keep, int64_t M_out, int32_t flip,
                                uint8_t* out, int64_t ld_out, void* stream) {
    if (!xp || !keep || !out) return fail("nadm_select_snps: null pointer");
    if (rows < 1 || M_out < 1) return fail("nadm_select_snps: empty selection (need rows > 0 and M_out > 0)");
    if (ld_in < 1 || ld_in >= (1ll << 32) || ld_out >= (1ll << 32)) return fail("nadm_select_snps: ld_in and ld_out must be in 1..2^32-1");
    if (ld_out * 4 < M_out) return fail("nadm_select_snps: ld_out < ceil(M_out/4)");
    if (((uintptr_t)keep & 7) != 0) return fail("nadm_select_snps: keep must be 8-byte aligned");
    const int64_t gx = (ld_out + 255) / 256;
    if (gx > 0x7FFFFFFFll) return fail("nadm_select_snps: too many blocks for one launch");
    const int64_t gy = rows < 4096 ? rows : 4096;
    hipLaunchKernelGGL(select_snps_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, xp, ld_in, rows, keep, M_out,
                       flip != 0 ? 1 : 0, out, ld_out);
    return check_launch("select_snps");
}
