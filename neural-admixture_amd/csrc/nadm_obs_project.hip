// The observed-calls pair products behind the standardised PCA (include/nadm.h, nadm_obs_project / nadm_obs_project_t): two tall-skinny
// products of the packed matrix with fp32 operands of up to 32 columns, on v_mfma_f32_16x16x32_bf16.  With a = g o in {0, 1, 2} and
// o in {0, 1}, both exact in one bf16 piece, and the fp32 operand cut into three round-to-nearest bf16 pieces (split3: exact):
//   forward     Y[s, c]  = sum_j a_sj W1[j, c] + o_sj W2[j, c]          SNPs on the instruction's k axis
//   transposed  O1[j, c] = sum_s a_sj Yin[s, c],  O2[j, c] = sum_s o_sj Yin[s, c]      samples on the k axis
//
// Two launches per call each, no floating-point atomics (two launches on the same inputs give the same bits):
//   obs_project_kernel    one 256-thread block per (256 samples, range of 256-SNP chunks).  Wave w owns four 16-sample row tiles; lane l
//                         is row l & 15 and k group l >> 4 of the A operand and keeps 16 bytes of its row's 64 per chunk IN REGISTERS
//                         (the next chunk's are loaded under the current chunk's work): k group q of step st = 0..7 holds the SNPs
//                         64 q + 8 st .. + 7 of the chunk, so a lane's operand is two of its own bytes and the matrix never goes through
//                         LDS.  W1 and W2 go through LDS as bf16 operand fragments [matrix][piece][step][q][column], four steps (128
//                         SNPs) a stage, built once per block from values fetched one stage ahead.  Per step, row tile and 16 columns six
//                         instructions (lo, mid, hi piece of W1 against a, of W2 against o) into ONE fp32 accumulator that lives for the
//                         range.  Missing calls, SNPs >= M, rows past the list and every pad bit are code 3 before the decode: +0.0f.
//   obs_project_t_kernel  one 256-thread block per (256-SNP chunk, slice of the batch's 64-sample tiles): the split of nadm_snp_sweep.h.
//                         A tile's 64 rows x 64 bytes arrive as one 16-byte load per thread and go to LDS (double-buffered, one barrier
//                         per tile, 16-byte pieces swizzled by the row's k group) beside the tile's Yin rows as bf16 operand fragments
//                         [piece][step][q][column].  Wave w owns the chunk's SNPs 64 w .. 64 w + 63 as four 16-SNP A tiles; lane l is SNP
//                         l & 15 and samples 8 (l >> 4) .. + 7 of the step: eight 16-byte LDS reads (a broadcast per k group) give it the
//                         calls of all four tiles.  Per step, SNP tile and 16 columns three instructions each into the O1 and the O2
//                         accumulator.  Rows past the list are code 3 and their Yin rows zero; SNPs >= M are computed and never folded.
//   the two fold kernels  one thread per output: the ranges' / slices' partials in order in float64, rounded to fp32 once; pad columns 0.
// The forward product's range split, row lookup and clamped piece load are those of nadm_chunk_ranges.h; the transposed product's
// slices are those of nadm_snp_sweep.h.
#include "nadm_chunk_ranges.h"
#include "nadm_snp_sweep.h"

namespace nadm {

constexpr int OBS_CHUNK = RANGE_CHUNK;
constexpr int OBS_ROWS = 256;             // samples per block of the forward product: 4 waves x OBS_RT row tiles of 16
constexpr int OBS_RT = 4;
constexpr int OBS_STAGE = 4;              // steps of 32 SNPs whose W fragments are in LDS at a time
constexpr int OBS_MAX_CHUNKS = 1024;      // chunks per range at most: no fp32 accumulator covers more than 2^18 SNPs
constexpr int64_t OBS_BLOCKS = 1024;      // blocks wanted at least, while there are chunks to split

// bf16 bit patterns of a = g o in {0, 1, 2} and of o in {0, 1} for a 2-bit code (3 = missing -> 0 in both), as arithmetic on the code
__device__ __forceinline__ uint32_t a16(uint32_t code) { return (0x3F00u + (code << 7)) & (0u - ((code ^ (code >> 1)) & 1u)); }
__device__ __forceinline__ uint32_t o16(uint32_t code) { return 0x3F80u & (((code + 1u) >> 2) - 1u); }

// the two operands of a lane from its eight codes (element e at bits [2e, 2e + 2) of h)
__device__ __forceinline__ void obs_operands(const uint32_t h, bf16x8_t& av, bf16x8_t& ov) {
    u32x4_t a, o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c0 = (h >> (4 * i)) & 3u, c1 = (h >> (4 * i + 2)) & 3u;
        a[i] = a16(c0) | (a16(c1) << 16);
        o[i] = o16(c0) | (o16(c1) << 16);
    }
    av = __builtin_bit_cast(bf16x8_t, a);
    ov = __builtin_bit_cast(bf16x8_t, o);
}

// eight fp32 values (0 where their mask is clear) -> the three 16-byte operand fragments hi, mid, lo
__device__ __forceinline__ void obs_split8(const float (&v)[8], const uint32_t (&m)[8], u32x4_t& hi, u32x4_t& mid, u32x4_t& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t h0, m0, l0, h1, m1, l1;
        split3(keepf(v[2 * i], m[2 * i]), h0, m0, l0);
        split3(keepf(v[2 * i + 1], m[2 * i + 1]), h1, m1, l1);
        hi[i] = h0 | (h1 << 16);
        mid[i] = m0 | (m1 << 16);
        lo[i] = l0 | (l1 << 16);
    }
}

template <int CP>
__global__ __launch_bounds__(256) void obs_project_kernel(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                                          const int b, const int64_t M, const float* __restrict__ W1,
                                                          const float* __restrict__ W2, const int tiles, const int chunks_per_range,
                                                          const int64_t chunks, float* __restrict__ part) {
    constexpr int CT = CP / 16;
    constexpr int FR = OBS_STAGE * 4 * CP;                        // fragments of one piece of one matrix in a stage
    constexpr int NF = 2 * FR / 256;                              // (matrix, fragment) pairs a thread builds per stage
    __shared__ __attribute__((aligned(16))) u32x4_t Img[2 * 3 * FR];      // [matrix][piece][step][q][column]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 15, q = lane >> 4;
    const int range = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - range * tiles;
    const auto [c_lo, c_hi] = chunk_range(range, chunks_per_range, chunks);

    // A role: row r of row tile rt of wave w, k group q
    const uint8_t* xrow[OBS_RT];
    uint32_t inval[OBS_RT];                                       // a row past the list: every call missing
#pragma unroll
    for (int rt = 0; rt < OBS_RT; ++rt) {
        const RangeRow rr = range_row(xp, ld, idx, tile * OBS_ROWS + 64 * w + 16 * rt + r, b);
        xrow[rt] = rr.x;
        inval[rt] = ~rr.valid;
    }
    auto load_x = [&](const int64_t c, u32x4_t (&xv)[OBS_RT]) {
#pragma unroll
        for (int rt = 0; rt < OBS_RT; ++rt) xv[rt] = range_piece(xrow[rt], c, q, ld);
    };
    // builder role: pair v is matrix x >> 4, step x >> 2 & 3 of the stage, k group x & 3 and column f % CP, f = t + 256 v, x = f / CP
    auto w_j0 = [&](const int v, const int64_t c, const int half) {
        const int x = (t + 256 * v) / CP;
        return c * OBS_CHUNK + 64 * (x & 3) + 8 * (OBS_STAGE * half + ((x >> 2) & 3));
    };
    auto load_w = [&](const int64_t c, const int half, float (&wv)[NF][8]) {      // a row >= M reads row M - 1; masked when it is split
#pragma unroll
        for (int v = 0; v < NF; ++v) {
            const int f = t + 256 * v;
            const float* Wm = (f / CP) >> 4 ? W2 : W1;
            const int64_t j0 = w_j0(v, c, half);
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[v][e] = Wm[min(j0 + e, M - 1) * CP + f % CP];
        }
    };

    f32x4_t acc[OBS_RT][CT];
#pragma unroll
    for (int rt = 0; rt < OBS_RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    u32x4_t nxt[OBS_RT], cur[OBS_RT];
    float wv[NF][8];
    load_x(c_lo, nxt);
    load_w(c_lo, 0, wv);

#pragma unroll 1
    for (int64_t c = c_lo; c < c_hi; ++c) {
        // SNPs >= M of this lane's 64 become code 3 (and with them the pad bits of the row's last byte and the bytes behind it)
        const int rem = (int)max(min(M - (c * OBS_CHUNK + 64 * q), (int64_t)64), (int64_t)0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = max(min(rem - 16 * i, 16), 0);
            const uint32_t tail = v >= 16 ? 0u : 0xFFFFFFFFu << (2 * v);
#pragma unroll
            for (int rt = 0; rt < OBS_RT; ++rt) cur[rt][i] = nxt[rt][i] | inval[rt] | tail;
        }
        load_x(min(c + 1, c_hi - 1), nxt);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            __syncthreads();                                      // the previous stage's fragments have been read
#pragma unroll
            for (int v = 0; v < NF; ++v) {
                const int f = t + 256 * v, x = f / CP;
                const int64_t j0 = w_j0(v, c, half);
                uint32_t m[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = lt_mask64(j0 + e, M);
                u32x4_t hi, mid, lo;
                obs_split8(wv[v], m, hi, mid, lo);
                u32x4_t* o = Img + ((x >> 4) * 3) * FR + (x & 15) * CP + f % CP;
                o[0 * FR] = hi;
                o[1 * FR] = mid;
                o[2 * FR] = lo;
            }
            __syncthreads();
            // the next stage's values, in flight under this stage's arithmetic (the last stage fetches itself again)
            load_w(half == 0 ? c : min(c + 1, c_hi - 1), half == 0 ? 1 : 0, wv);
#pragma unroll
            for (int s4 = 0; s4 < OBS_STAGE; ++s4) {
                bf16x8_t av[OBS_RT], ov[OBS_RT];
#pragma unroll
                for (int rt = 0; rt < OBS_RT; ++rt)
                    obs_operands((cur[rt][2 * half + (s4 >> 1)] >> (16 * (s4 & 1))) & 0xFFFFu, av[rt], ov[rt]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const u32x4_t* ib = Img + (s4 * 4 + q) * CP + 16 * ct + r;
                    bf16x8_t b1[3], b2[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        b1[p] = __builtin_bit_cast(bf16x8_t, ib[p * FR]);
                        b2[p] = __builtin_bit_cast(bf16x8_t, ib[(3 + p) * FR]);
                    }
#pragma unroll
                    for (int rt = 0; rt < OBS_RT; ++rt) {
#pragma unroll
                        for (int p = 2; p >= 0; --p) {           // lo, mid, hi
                            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[rt], b1[p], acc[rt][ct], 0, 0, 0);
                            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ov[rt], b2[p], acc[rt][ct], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // D: column = lane & 15, rows 4 (lane >> 4) + i of the row tile.  Every block writes its whole slab [256, CP]
    float* out = part + ((int64_t)range * tiles + tile) * (OBS_ROWS * CP);
#pragma unroll
    for (int rt = 0; rt < OBS_RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[(64 * w + 16 * rt + 4 * q + i) * CP + 16 * ct + r] = acc[rt][ct][i];
}

// One thread per (sample s < b, column c < CP): the ranges' partials in range order in float64, rounded once; pad columns 0
__global__ __launch_bounds__(256) void obs_project_fold_kernel(const float* __restrict__ part, const int ranges, const int64_t rows_p,
                                                               const int b, const int C, const int CP, float* __restrict__ Y) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)b * CP) return;
    const int c = (int)(e % CP);
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += (double)part[(int64_t)r * rows_p * CP + e];
    Y[e] = c < C ? (float)s : 0.f;
}

template <int CP>
__global__ __launch_bounds__(256) void obs_project_t_kernel(const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx,
                                                            const int b, const float* __restrict__ Yin, const int slices,
                                                            const int tiles_per_slice, const int64_t Mp, float* __restrict__ part) {
    constexpr int CT = CP / 16;
    constexpr int FR = 2 * 4 * CP;                                // fragments of one piece in a tile: [step][q][column]
    __shared__ __attribute__((aligned(16))) u32x4_t Xs[2][SWEEP_TILE * 4];        // [row][16-byte piece ^ (row >> 3 & 3)]
    __shared__ __attribute__((aligned(16))) u32x4_t Ys[2][3 * FR];                // [piece][step][q][column]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 15, q = lane >> 4;
    const SweepPos pos = sweep_pos(slices);
    const int tiles = (b + SWEEP_TILE - 1) / SWEEP_TILE;
    const int t_lo = pos.slice * tiles_per_slice;                 // < tiles: slices = ceil(tiles / tiles_per_slice)
    const int t_hi = min(t_lo + tiles_per_slice, tiles);

    // loader roles.  X: row t / 4 of the tile, 16-byte piece t % 4 of the chunk's 64 bytes (a piece past the row's end holds SNPs >= M
    // only: clamped, unconditional).  Yin: fragment t = (step, q, column), the eight samples 32 step + 8 q .. + 7 of the tile
    const int lrow = t >> 2;
    const int64_t boff = min(pos.chunk * (OBS_CHUNK / 4) + 16 * (t & 3), ld - 16);
    auto row_of = [&](const int tile) {
        const int sc = min(tile * SWEEP_TILE + lrow, b - 1);
        return idx ? idx[sc] : sc;
    };
    const bool builder = t < FR;
    const int fcol = t % CP, fs0 = 32 * ((t / CP) >> 2) + 8 * ((t / CP) & 3);
    int row = row_of(t_lo);
    u32x4_t xv = {0u, 0u, 0u, 0u};
    float yv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = 0.f;

    f32x4_t acc1[4][CT], acc2[4][CT];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc1[jt][ct] = acc2[jt][ct] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // one iteration ahead of the arithmetic, as snp_sweep: iteration `tile` stores the tile's rows (fetched by the iteration before) to
    // LDS, issues the loads of tile + 1 and then works on tile.  The other buffer was read in the previous iteration, which every thread
    // left before it passed this iteration's barrier: one barrier per tile
#pragma unroll 1
    for (int tile = t_lo - 1; tile < t_hi; ++tile) {
        const bool work = tile >= t_lo;
        const int buf = (tile - t_lo) & 1;
        if (work) {
            Xs[buf][lrow * 4 + ((t & 3) ^ ((lrow >> 3) & 3))] = xv | ~lt_mask(tile * SWEEP_TILE + lrow, b);
            if (builder) {
                uint32_t m[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = lt_mask(tile * SWEEP_TILE + fs0 + e, b);
                u32x4_t hi, mid, lo;
                obs_split8(yv, m, hi, mid, lo);
                Ys[buf][0 * FR + t] = hi;
                Ys[buf][1 * FR + t] = mid;
                Ys[buf][2 * FR + t] = lo;
            }
        }
        __syncthreads();
        {
            const int nt = min(tile + 1, t_hi - 1);
            xv = *reinterpret_cast<const u32x4_t*>(xp + (int64_t)row * ld + boff);
            row = row_of(min(tile + 2, t_hi - 1));
            if (builder) {
#pragma unroll
                for (int e = 0; e < 8; ++e) yv[e] = Yin[(int64_t)min(nt * SWEEP_TILE + fs0 + e, b - 1) * CP + fcol];
            }
        }
        if (!work) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // the calls of this lane's SNP (r of each of the wave's four 16-SNP tiles) in its eight samples
            uint32_t hh[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const u32x4_t v = Xs[buf][(32 * h + 8 * q + e) * 4 + (w ^ q)];       // (row >> 3 & 3 = q)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) hh[jt] |= ((v[jt] >> (2 * r)) & 3u) << (2 * e);
            }
            bf16x8_t av[4], ov[4];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) obs_operands(hh[jt], av[jt], ov[jt]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const u32x4_t* ib = Ys[buf] + (h * 4 + q) * CP + 16 * ct + r;
                bf16x8_t bp[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) bp[p] = __builtin_bit_cast(bf16x8_t, ib[p * FR]);
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
                    for (int p = 2; p >= 0; --p) {               // lo, mid, hi
                        acc1[jt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[jt], bp[p], acc1[jt][ct], 0, 0, 0);
                        acc2[jt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ov[jt], bp[p], acc2[jt][ct], 0, 0, 0);
                    }
                }
            }
        }
    }
    // D: column = lane & 15, rows (SNPs) 4 (lane >> 4) + i of the SNP tile.  The slice's slab is [Mp][O1 | O2][CP]; rows M..Mp are never read
    float* out = part + ((int64_t)pos.slice * Mp + pos.chunk * OBS_CHUNK) * (2 * CP);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = (64 * w + 16 * jt + 4 * q + i) * (2 * CP) + 16 * ct + r;
                out[o] = acc1[jt][ct][i];
                out[o + CP] = acc2[jt][ct][i];
            }
}

// One thread per (SNP j < M, column c < CP): the slices' partials in slice order in float64, rounded once; pad columns 0
__global__ __launch_bounds__(256) void obs_project_t_fold_kernel(const float* __restrict__ part, const int slices, const int64_t Mp,
                                                                 const int64_t M, const int C, const int CP, float* __restrict__ O1,
                                                                 float* __restrict__ O2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * CP) return;
    const int64_t j = e / CP;
    const int c = (int)(e - j * CP);
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < slices; ++s) {
        const float* p = part + ((int64_t)s * Mp + j) * (2 * CP) + c;
        s1 += (double)p[0];
        s2 += (double)p[CP];
    }
    O1[e] = c < C ? (float)s1 : 0.f;
    O2[e] = c < C ? (float)s2 : 0.f;
}

static bool obs_shape_ok(int b, int64_t M) { return b > 0 && b <= NADM_OBS_MAX_ROWS && M > 0; }
static bool obs_cp_ok(int CP) { return CP == 16 || CP == 32; }
// the forward product's launch shape, a rule of (b, M) alone
static RangePlan obs_plan(int b, int64_t M) { return range_plan(M, range_tiles(b, OBS_ROWS), OBS_BLOCKS, OBS_MAX_CHUNKS); }

static int obs_check(const char* who, const void* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, int32_t C, int32_t CP) {
    if (b <= 0 || M <= 0) return failf(who, "empty block (need b > 0 and M > 0)");
    if (b > NADM_OBS_MAX_ROWS) return failf(who, "b must be <= NADM_OBS_MAX_ROWS");
    if (check_packed(who, ld, M)) return 1;
    if (!obs_cp_ok(CP)) return failf(who, "CP must be 16 or 32");
    if (C < 1 || C > CP) return failf(who, "C must be in 1..CP");
    if (((uintptr_t)xp & 15) != 0 || ((uintptr_t)idx & 3) != 0) return failf(who, "xp must be 16-byte and idx 4-byte aligned");
    return 0;
}

}  // namespace nadm

using namespace nadm;

extern "C" int32_t nadm_obs_project_chunks(int32_t b, int64_t M) { return obs_shape_ok(b, M) ? range_count(obs_plan(b, M).cpr) : 0; }
extern "C" int32_t nadm_obs_project_ranges(int32_t b, int64_t M) { return obs_shape_ok(b, M) ? range_count(obs_plan(b, M).ranges) : 0; }

// scratch: [ranges][256 tiles][CP] float
extern "C" int64_t nadm_obs_project_scratch_floats(int32_t b, int64_t M, int32_t CP) {
    return obs_shape_ok(b, M) && obs_cp_ok(CP) ? obs_plan(b, M).blocks_bound * (OBS_ROWS * CP) : 0;
}

extern "C" int32_t nadm_obs_project_t_slices(int32_t b, int64_t M) { return obs_shape_ok(b, M) ? sweep_slices(b, M) : 0; }

// scratch: [slices][Mp][O1 | O2][CP] float, Mp = 256 chunks
extern "C" int64_t nadm_obs_project_t_scratch_floats(int32_t b, int64_t M, int32_t CP) {
    if (!obs_shape_ok(b, M) || !obs_cp_ok(CP)) return 0;
    return sweep_rows_bound(b, M) * (2 * CP);
}

extern "C" int nadm_obs_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* W1, const float* W2,
                                int32_t C, int32_t CP, float* Y, float* scratch, void* stream) {
    if (!xp || !W1 || !W2 || !Y || !scratch) return fail("nadm_obs_project: null pointer");
    if (obs_check("nadm_obs_project", xp, ld, idx, b, M, C, CP)) return 1;
    if ((((uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)Y | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_obs_project: W1, W2, Y and scratch must be 16-byte aligned");
    const RangePlan pl = obs_plan(b, M);
    if (range_launch_check("nadm_obs_project", pl)) return 1;
    hipStream_t st = (hipStream_t)stream;
    auto accum = CP == 16 ? obs_project_kernel<16> : obs_project_kernel<32>;
    hipLaunchKernelGGL(accum, range_grid(pl), dim3(256), 0, st, xp, ld, idx, b, M, W1, W2, (int)pl.tiles, (int)pl.cpr, pl.chunks, scratch);
    if (int e = check_launch("obs_project (accumulate)")) return e;
    hipLaunchKernelGGL(obs_project_fold_kernel, fold_grid((int64_t)b * CP), dim3(256), 0, st, scratch, (int)pl.ranges, pl.tiles * OBS_ROWS, b, C,
                       CP, Y);
    return check_launch("obs_project (fold)");
}

extern "C" int nadm_obs_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Yin, int32_t C,
                                  int32_t CP, float* O1, float* O2, float* scratch, void* stream) {
    if (!xp || !Yin || !O1 || !O2 || !scratch) return fail("nadm_obs_project_t: null pointer");
    if (obs_check("nadm_obs_project_t", xp, ld, idx, b, M, C, CP)) return 1;
    if ((((uintptr_t)Yin | (uintptr_t)O1 | (uintptr_t)O2 | (uintptr_t)scratch) & 15) != 0)
        return fail("nadm_obs_project_t: Yin, O1, O2 and scratch must be 16-byte aligned");
    const int64_t chunks = sweep_chunks(M), Mp = chunks * SWEEP_CHUNK;
    const int tps = sweep_tiles_per_slice(b, M), slices = sweep_slices(b, M);
    if (chunks * slices > 0x7FFFFFFFll) return fail("nadm_obs_project_t: too many blocks for one launch");
    if ((M * CP + 255) / 256 > 0x7FFFFFFFll) return fail("nadm_obs_project_t: M too large for the fold's launch");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * slices);
    if (CP == 16)
        hipLaunchKernelGGL((obs_project_t_kernel<16>), dim3(grid), dim3(256), 0, st, xp, ld, idx, b, Yin, slices, tps, Mp, scratch);
    else
        hipLaunchKernelGGL((obs_project_t_kernel<32>), dim3(grid), dim3(256), 0, st, xp, ld, idx, b, Yin, slices, tps, Mp, scratch);
    if (int e = check_launch("obs_project_t (accumulate)")) return e;
    hipLaunchKernelGGL(obs_project_t_fold_kernel, dim3((unsigned)((M * CP + 255) / 256)), dim3(256), 0, st, scratch, slices, Mp, M, C, CP,
                       O1, O2);
    return check_launch("obs_project_t (fold)");
}
