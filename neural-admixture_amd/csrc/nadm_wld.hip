// Weighted admixture LD for dating an admixture (include/nadm.h: nadm_wld).
//
//   wld_kernel   the covariance of every SNP pair (a, b), a < b <= a + W, over the SAMPLE axis on v_mfma_i32_16x16x64_i8, weighted per
//                curve and added into bins of genetic distance.  The product is ld_band_kernel's scheme (nadm_ld.hip) with two int8
//                pieces per side instead of three -- o (call observed) and g o -- and four products per tile: n, Sa, Sb, Sab in int32,
//                exact.  One 256-thread block owns 64 "a" SNPs (one 16-SNP tile per wave) and up to 8 of the "b" tiles each of them
//                needs (tiles at .. at + 7 + 8 gy of the wave's tile at; blockIdx.y = gy walks the rest of a wide reach), and runs over
//                all samples in steps of 64 = the K of the instruction: per step the block
//                  STAGES   64 samples x (16 + up to 48) bytes of their rows into LDS TRANSPOSED, [byte column][sample]; rows past
//                           `rows`, SNPs >= M and pad bits are overwritten with the missing code here, so everything behind sees them
//                           as exactly 0;
//                  EXPANDS  one dword of that (4 samples of one byte column) into the 4 SNPs x 2 pieces it holds with byte-lane
//                           arithmetic and writes the operand image [piece][SNP][64 samples], one 80-byte row per SNP;
//                  MULTIPLIES lane l reads 16 bytes = samples 16 (l >> 4) .. + 15 of SNP l & 15 of a tile, for both operands.
//                Epilogue, one pair per accumulator register: the unbiased covariance in int64 / float64, per curve the weighted value
//                rounded to a 2^-32 fixed-point integer and added with 64-bit integer atomics: any order, the same bits.  The block
//                first adds its pairs in LDS, over a window of 128 bins from the nearest bin it can reach (the operand image's memory,
//                free by then), and sends the window on with one global add per entry that holds something; a pair beyond the
//                window goes to global memory directly.  -DNADM_WLD_GLOBAL_ATOMICS builds the plain form, every add in global
//                memory, for an A/B (tools/build_variant.sh).
//                A block none of whose pairs can fall into a bin (its nearest pair is nbins cells or more apart, or its "b" SNPs lie
//                past m1) leaves before the first load.
// The unit shares no device code with nadm_ld.hip: that unit's objects stay what they were.
#include "nadm_common.h"
#include "nadm_host.h"

namespace nadm {

constexpr int WL_TA = 64;                 // "a" SNPs per block: 4 tiles of 16, one per wave = 16 bytes of a packed row
constexpr int WL_KS = 64;                 // samples per step = K of the instruction
constexpr int WL_NBG = 8;                 // "b" tiles per "a" tile whose accumulators one block holds (8 x 4 x 4 = 128 registers)
constexpr int WL_BT = WL_NBG + 3;         // "b" tiles of the image: wave 3's last is tile 3 + 7
constexpr int WL_SNPS = WL_TA + 16 * WL_BT;        // SNP rows of the operand image (240)
constexpr int WL_ROW = 80;                // bytes per image row: 64 samples + 16 (a dword column of four SNP groups then spreads over the banks)
constexpr int WL_RAWC = 64;               // byte columns of the transposed stage: 16 of "a", 48 of "b"
constexpr int WL_WB = 128;                // bins of the block's LDS window of sums (the epilogue; it takes the image's place)
static_assert((NADM_WLD_MAX_CURVES + 1) * WL_WB * 8 <= 2 * WL_SNPS * WL_ROW, "the window of sums must fit into the operand image");

__global__ __launch_bounds__(256, 2) void wld_kernel(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                                     const int rows, const int64_t M, const int64_t m0, const int64_t m1, const int W,
                                                     const int nb_tiles, const int32_t* __restrict__ cell, const double* __restrict__ wt,
                                                     const int C, const int nbins, const int nmin, unsigned long long* __restrict__ sum,
                                                     unsigned long long* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) uint8_t rawT[WL_RAWC * WL_KS];
    __shared__ __attribute__((aligned(16))) uint8_t Img[2 * WL_SNPS * WL_ROW];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int gy = (int)blockIdx.y;
    const int64_t j0 = (m0 / WL_TA + blockIdx.x) * WL_TA;         // first "a" SNP of the block
    const int64_t jb0 = j0 + (int64_t)16 * WL_NBG * gy;           // first SNP of the "b" part of the image
    // (the same in every thread, before the first barrier) no "b" SNP below m1, or the block's nearest pair -- its last "a" SNP with
    // its first "b" SNP behind it; cell does not decrease -- is already nbins cells apart: nothing to add
    if (jb0 >= m1) return;
    {
        const int64_t a_hi = min(j0 + WL_TA - 1, m1 - 1);
        if (jb0 > a_hi && cell[jb0] - cell[a_hi] >= nbins) return;
    }
    const int nbg = min(WL_NBG, nb_tiles - WL_NBG * gy);          // "b" tiles per wave in this block (>= 1)
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
        const int pos = step * WL_KS + s;
        const int posc = min(pos, rows - 1);
        const int64_t row = idx ? idx[posc] : posc;
        v = *reinterpret_cast<const u32x4_t*>(xp + row * ld + off);
        const uint32_t gone = pos < rows ? 0u : 0xFFFFFFFFu;      // a row past the list: every call missing
#pragma unroll
        for (int d = 0; d < 4; ++d) v[d] |= tail[d] | gone;
    };

    i32x4_t acc[WL_NBG][4];
#pragma unroll
    for (int tt = 0; tt < WL_NBG; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[tt][q] = (i32x4_t){0, 0, 0, 0};

    const int steps = (rows + WL_KS - 1) / WL_KS;
    u32x4_t nxt = (u32x4_t){0u, 0u, 0u, 0u};
    if (part_used) load_step(0, nxt);

#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
        // ---- stage, transposed: byte i of the piece -> [16 part + i][s]
        if (part_used) {
#pragma unroll
            for (int i = 0; i < 16; ++i) rawT[(16 * part + i) * WL_KS + s] = (uint8_t)(nxt[i >> 2] >> (8 * (i & 3)));
            load_step(min(step + 1, steps - 1), nxt);
        }
        __syncthreads();
        // ---- expand: (byte column c, samples 4 q .. 4 q + 3) -> 4 SNPs x 2 pieces, a dword each
        for (int e = t; e < ncols * 16; e += 256) {
            const int c = e >> 4, q = e & 15;
            const uint32_t r = reinterpret_cast<const uint32_t*>(rawT)[c * 16 + q];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t x = (r >> (2 * i)) & 0x03030303u;              // the codes of SNP 4 c + i, a sample per byte
                const uint32_t miss = x & (x >> 1) & 0x01010101u;             // 1 where the code is 3
                const uint32_t o = miss ^ 0x01010101u;
                const uint32_t g = x ^ (miss * 3u);                           // 0, 1, 2; 0 where missing
                uint32_t* dst = reinterpret_cast<uint32_t*>(Img + (4 * c + i) * WL_ROW) + q;
                dst[0] = o;
                dst[WL_SNPS * WL_ROW / 4] = g;
            }
        }
        __syncthreads();
        // ---- multiply: lane l is SNP l & 15 of its tile and samples 16 (l >> 4) .. + 15 of the step, for both operands
        {
            const uint8_t* ia = Img + (16 * w + (lane & 15)) * WL_ROW + 16 * (lane >> 4);
            const i32x4_t ao = *reinterpret_cast<const i32x4_t*>(ia);
            const i32x4_t ag = *reinterpret_cast<const i32x4_t*>(ia + WL_SNPS * WL_ROW);
#pragma unroll
            for (int tt = 0; tt < WL_NBG; ++tt) {
                if (tt < nbg) {                                               // (the same in every lane)
                    const uint8_t* ib = Img + (WL_TA + 16 * (w + tt) + (lane & 15)) * WL_ROW + 16 * (lane >> 4);
                    const i32x4_t bo = *reinterpret_cast<const i32x4_t*>(ib);
                    const i32x4_t bg = *reinterpret_cast<const i32x4_t*>(ib + WL_SNPS * WL_ROW);
                    acc[tt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bo, acc[tt][0], 0, 0, 0);       // n
                    acc[tt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bo, acc[tt][1], 0, 0, 0);       // Sa
                    acc[tt][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ao, bg, acc[tt][2], 0, 0, 0);       // Sb
                    acc[tt][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bg, acc[tt][3], 0, 0, 0);       // Sab
                }
            }
        }
        // (the next step's stage is written after the barrier above, its image after the barrier below it: no third barrier)
    }

#ifndef NADM_WLD_GLOBAL_ATOMICS
    // The block's own sums over a window of WL_WB bins from its nearest possible bin on, in the LDS the operand image no longer needs:
    // rows 0 .. C - 1 the curves, row C the pair counts.
    unsigned long long* const win = reinterpret_cast<unsigned long long*>(Img);
    const int base = gy == 0 ? 0 : cell[jb0] - cell[min(j0 + WL_TA - 1, m1 - 1)];      // (>= 0, < nbins: checked on entry)
    __syncthreads();                                              // every wave has read its last operands
    for (int e = t; e < (C + 1) * WL_WB; e += 256) win[e] = 0ull;
    __syncthreads();
#endif
    // D: column = lane & 15 = the "b" SNP of the tile, rows 4 (lane >> 4) + i = the "a" SNP
#pragma unroll
    for (int tt = 0; tt < WL_NBG; ++tt) {
        if (tt >= nbg) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t ja = j0 + 16 * w + 4 * (lane >> 4) + i;
            const int64_t jb = jb0 + 16 * (w + tt) + (lane & 15);
            const int64_t d = jb - ja;
            if (ja < m0 || jb >= m1 || d < 1 || d > W) continue;             // (jb < m1 and d >= 1 give ja < m1)
            const int bin = cell[jb] - cell[ja];
            if (bin < 0 || bin >= nbins) continue;
            const int64_t n = acc[tt][0][i], Sa = acc[tt][1][i], Sb = acc[tt][2][i], Sab = acc[tt][3][i];
            if (n < nmin) continue;
            const int64_t num = n * Sab - Sa * Sb, den = n * (n - 1);
            const double v = (double)num / (double)den;
            // (inlined at each call: the compiler sees which memory the pointers are in -- LDS adds or global adds, not flat ones)
            auto add_pair = [&](unsigned long long* const dcnt, unsigned long long* const dsum, const int64_t dstride) {
                atomicAdd(dcnt, 1ull);
                for (int c = 0; c < C; ++c) {
                    const double ta = v * wt[(int64_t)c * M + ja];
                    const double tb = ta * wt[(int64_t)c * M + jb];
                    const long long q = llrint(tb * 4294967296.0);
                    if (q != 0) atomicAdd(dsum + c * dstride, (unsigned long long)q);
                }
            };
#ifndef NADM_WLD_GLOBAL_ATOMICS
            const int rel = bin - base;
            if (rel >= 0 && rel < WL_WB) add_pair(win + C * WL_WB + rel, win + rel, WL_WB);       // in the block's window
            else
#endif
                add_pair(cnt + bin, sum + bin, nbins);
        }
    }
#ifndef NADM_WLD_GLOBAL_ATOMICS
    // the window leaves the block: one global add per entry that holds something
    __syncthreads();
    for (int e = t; e < (C + 1) * WL_WB; e += 256) {
        const unsigned long long x = win[e];
        const int c = e / WL_WB, bin = base + e % WL_WB;
        if (x != 0ull && bin >= 0 && bin < nbins) atomicAdd(c < C ? sum + (int64_t)c * nbins + bin : cnt + bin, x);
    }
#endif
}

}  // namespace nadm

using namespace nadm;

extern "C" int nadm_wld(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int64_t m0, int64_t m1, int32_t W,
                        const int32_t* cell, const double* wt, int32_t C, int32_t nbins, int32_t nmin, int64_t* sum, int64_t* cnt,
                        void* stream) {
    const char* who = "nadm_wld";
    if (!xp || !cell || !wt || !sum || !cnt) return failf(who, "null pointer");
    if (((uintptr_t)xp & 15) != 0) return failf(who, "xp must be 16-byte aligned");
    if (((uintptr_t)wt & 7) != 0 || ((uintptr_t)sum & 7) != 0 || ((uintptr_t)cnt & 7) != 0)
        return failf(who, "wt, sum and cnt must be 8-byte aligned");
    if (((uintptr_t)cell & 3) != 0 || ((uintptr_t)idx & 3) != 0) return failf(who, "cell and idx must be 4-byte aligned");
    if (rows < 2 || rows > (1ll << 24)) return failf(who, "rows must be in 2..2^24");
    if (C < 1 || C > NADM_WLD_MAX_CURVES) return failf(who, "C must be in 1..NADM_WLD_MAX_CURVES");
    if (nbins < 1 || nbins > NADM_WLD_MAX_BINS) return failf(who, "nbins must be in 1..NADM_WLD_MAX_BINS");
    if (W < 1 || W > NADM_WLD_MAX_SPAN) return failf(who, "W must be in 1..NADM_WLD_MAX_SPAN");
    if (nmin < 2) return failf(who, "nmin must be >= 2");
    if (m0 < 0 || m0 >= m1 || m1 > M) return failf(who, "need 0 <= m0 < m1 <= M");
    if (check_packed(who, ld, M)) return 1;
    const int nb_tiles = (W + 15) / 16 + 1;                       // "b" tiles an "a" tile meets: its own and the next ceil(W / 16)
    const int64_t gx = (m1 - 1) / WL_TA - m0 / WL_TA + 1;
    const int gy = (nb_tiles + WL_NBG - 1) / WL_NBG;
    if (gx > 0x7FFFFFFFll || gy > 65535) return failf(who, "too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sum, 0, (size_t)C * (size_t)nbins * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(cnt, 0, (size_t)nbins * sizeof(int64_t), st) != hipSuccess)
        return failf(who, "hipMemsetAsync failed");
    hipLaunchKernelGGL(wld_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, xp, ld, idx, (int)rows, M, m0, m1, (int)W, nb_tiles,
                       cell, wt, (int)C, (int)nbins, (int)nmin, reinterpret_cast<unsigned long long*>(sum),
                       reinterpret_cast<unsigned long long*>(cnt));
    return check_launch("wld");
}
