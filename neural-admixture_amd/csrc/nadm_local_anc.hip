// Local ancestry: the forward-backward recursion of the linkage model along the genome (include/nadm.h, nadm_local_anc).  Each of a
// sample's two haplotypes carries an ancestry that is redrawn from the sample's q with probability rho[j] between SNP j - 1 and j
// (Falush et al. 2003); the unphased call is emitted from the two ancestries' frequencies (Corbett-Detig & Nielsen 2017).  The chain
// is sequential along the SNP axis, N M K^2 work with a dependent step per SNP: nothing of it is a Gram product.
//
// Two launches per call, no atomics (two launches on the same inputs give the same bits), one 256-thread block per (256-sample tile,
// segment), a lane per sample, on the pieces of nadm_chunk_ranges.h (range_row, range_piece, stage_rows, chunk_word, load_row) with the
// chunk loop written out, as resid_project_kernel writes its loop out: the walk runs over the chunks that overlap the segment, SNPs
// outside the segment are skipped word by word, and the chunk's rho sits in LDS next to its P rows.
//   local_anc_fwd_kernel   SNPs ascending.  The state is the upper triangle of the symmetric a(x, y): T = KP (KP + 1) / 2 registers,
//                          with its KP row sums beside it.  Per SNP: the emission factors of the call (bit selects, no compare), per
//                          pair three multiply-adds for the prior, two for the emission, one multiply, the row sums, one multiply to
//                          normalise; one reciprocal and one log2 per SNP.  ln S is summed as log2 S in fp32 within a chunk, times
//                          ln 2 in float64 across chunks.  At an output point the normalised state goes to the checkpoints
//                          [out point][state][lane]: a wave's stores are contiguous.
//   local_anc_bwd_kernel   SNPs descending from the segment's last SNP to its first output point, the same registers for b(x, y).  At
//                          an output point the checkpoint is read back state by state: gamma's row sums, the heaviest unordered pair
//                          and the normaliser in one pass, then dosage, call and post.
// A pad column has q = 0: its states are exactly +0.0f in both passes.  At KP = 16 a lane holds 136 states + 16 row sums + 16 q +
// 48 emission factors + 32 packed words: a 256-thread block is one wave per SIMD, which may use the whole register file, so nothing
// spills.  Not built: phased input, per-component rates, Viterbi paths, heads wider than 16.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int LA_MAX_KP = 16;
constexpr int LA_TILE = 256;              // samples per block: 4 waves, a lane per sample
constexpr double LA_LN2 = 0.693147180559945309417232121458;
__host__ __device__ constexpr int la_pairs(int k) { return k * (k + 1) / 2; }

// The emission of a call as e(x, y) = fma(u_x, v_y, u_y w_x):
//   code 0   u = v = c, w = 0   ->  c_x c_y                      code 2   u = v = p, w = 0   ->  p_x p_y
//   code 1   u = p, v = w = c   ->  fma(p_x, c_y, p_y c_x)       missing  u = v = 1, w = 0   ->  exactly 1
// p = clip(P), c = clip(1 - P) from the UNCLIPPED value, as em_terms (nadm_common.h).  The factors are picked with bit masks formed
// from the code's two bits (nadm_common.h says why not with selects)
template <int KP>
__device__ __forceinline__ void la_factors(const float* prow, const uint32_t code, const float eps, const float one_m_eps, float (&u)[KP],
                                           float (&v)[KP], float (&w)[KP]) {
    const uint32_t lo = code & 1u, hi = code >> 1;
    uint32_t m1 = 0u - (lo & ~hi), m3 = 0u - (lo & hi), mu = 0u - (lo ^ hi), mv = 0u - (hi & ~lo & 1u);
    asm("" : "+v"(m1), "+v"(m3), "+v"(mu), "+v"(mv));
    const uint32_t one = 0x3F800000u & m3, nu = ~(mu | m3), nv = ~(mv | m3);
    float pr[KP];
    load_row<KP>(prow, pr);                                       // in LDS, the same address in every lane: a broadcast
#pragma unroll
    for (int x = 0; x < KP; ++x) {
        const uint32_t pb = __float_as_uint(fminf(fmaxf(pr[x], eps), one_m_eps));
        const uint32_t cb = __float_as_uint(fminf(fmaxf(1.f - pr[x], eps), one_m_eps));
        u[x] = __uint_as_float((pb & mu) | (cb & nu) | one);
        v[x] = __uint_as_float((pb & mv) | (cb & nv) | one);
        w[x] = __uint_as_float(cb & m1);
    }
}

// what both kernels set up the same way
struct LaBlock { int sg, tile; int64_t s0, s1; };
__device__ __forceinline__ LaBlock la_block(const int32_t* __restrict__ seg, const int tiles) {
    const int sg = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - sg * tiles;          // tile fastest: neighbours share a chunk of P
    return {sg, tile, (int64_t)seg[sg], (int64_t)seg[sg + 1]};
}
// the chunk's rho into LDS (blockDim = 256 = the chunk): exactly 1 at `first` (a restart: whatever the array holds there), 0 past M
__device__ __forceinline__ void la_stage_rho(const float* __restrict__ rho, const int64_t j0, const int64_t M, const int64_t first, float* Rs) {
    const int64_t j = j0 + threadIdx.x;
    Rs[threadIdx.x] = j == first ? 1.f : (j < M ? rho[j] : 0.f);
}

template <int KP>
__global__ __launch_bounds__(LA_TILE) void local_anc_fwd_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const float* __restrict__ rho, const int32_t* __restrict__ seg, const int n_seg, const int32_t* __restrict__ out_snp,
    const int32_t* __restrict__ oseg, const int n_out, const int tiles, float* __restrict__ ckpt, double* __restrict__ ll) {
    constexpr int T = la_pairs(KP);
    __shared__ __attribute__((aligned(16))) float Ps[RANGE_CHUNK * KP];      // the chunk's P rows (16 KB at KP = 16)
    __shared__ float Rs[RANGE_CHUNK];                                        // the chunk's rho
    const int t = threadIdx.x;
    const LaBlock bk = la_block(seg, tiles);
    const RangeRow rr = range_row(xp, ld, idx, bk.tile * LA_TILE + t, b);
    const uint32_t inval = ~rr.valid;                             // a row past the list: every call missing
    const bool wave_live = bk.tile * LA_TILE + (t & ~63) < b;     // wave-uniform
    const int64_t lanes = (int64_t)tiles * LA_TILE;

    float q[KP];
    load_row<KP>(Q + (int64_t)rr.posc * q_stride, q);
    float A[T], R[KP];                                            // the normalised state and its row sums; a restart finds zeros
#pragma unroll
    for (int i = 0; i < T; ++i) A[i] = 0.f;
#pragma unroll
    for (int x = 0; x < KP; ++x) R[x] = 0.f;
    double llv = 0.0;

    if (bk.s0 < bk.s1) {                                          // (block-uniform; an empty segment has ll = 0)
        const int64_t c_lo = bk.s0 / RANGE_CHUNK, c_hi = (bk.s1 + RANGE_CHUNK - 1) / RANGE_CHUNK;
        int o = ckpt ? max(oseg[bk.sg], 0) : 0;                   // (the caller checked oseg; the clamps keep a bad one inside the scratch)
        const int o_end = ckpt ? min(oseg[bk.sg + 1], n_out) : 0;
        int64_t next_out = o < o_end ? (int64_t)out_snp[o] : -1;

        u32x4_t nxt[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, c_lo, v, ld);
#pragma unroll 1
        for (int64_t c = c_lo; c < c_hi; ++c) {
            const int64_t j0 = c * RANGE_CHUNK;
            if (c > c_lo) __syncthreads();                        // the previous chunk's rows have been read
            stage_rows<RANGE_CHUNK, KP, LA_TILE>(P, j0, M, Ps);
            la_stage_rho(rho, j0, M, bk.s0, Rs);
            uint32_t wd[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) wd[i] = nxt[i >> 2][i & 3] | inval;
            {
                const int64_t cn = min(c + 1, c_hi - 1);          // the next chunk's words, in flight under this chunk's arithmetic
#pragma unroll
                for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cn, v, ld);
            }
            __syncthreads();
            if (!wave_live) continue;
            const int lo = (int)max(bk.s0 - j0, (int64_t)0), hi = (int)min(bk.s1 - j0, (int64_t)RANGE_CHUNK);     // the segment's part
            float lsum = 0.f;                                     // the chunk's sum of log2 S: 256 terms in fp32
#pragma unroll 1
            for (int wi = lo >> 4; wi < (hi + 15) >> 4; ++wi) {   // one 32-bit word = 16 SNPs
                const uint32_t bits = chunk_word(wd, wi, M - (j0 + 16 * wi));     // SNPs >= M as code 3
                const int e_lo = max(lo - 16 * wi, 0), e_hi = min(hi - 16 * wi, 16);
#pragma unroll 1
                for (int e = e_lo; e < e_hi; ++e) {
                    const int sl = wi * 16 + e;
                    float u[KP], v[KP], w[KP];
                    la_factors<KP>(Ps + sl * KP, (bits >> (2 * e)) & 3u, eps, one_m_eps, u, v, w);
                    const float r = Rs[sl], s = 1.f - r;
                    const float c0 = s * s, c1 = r * s, hc2 = 0.5f * (r * r);
                    // pr(x, y) = c0 a + q_y G_x + q_x G_y with G_x = c1 R_x + (c2 / 2) q_x
                    float G[KP], Rn[KP];
#pragma unroll
                    for (int x = 0; x < KP; ++x) { G[x] = fmaf(c1, R[x], hc2 * q[x]); Rn[x] = 0.f; }
                    int i = 0;
#pragma unroll
                    for (int a = 0; a < KP; ++a)
#pragma unroll
                        for (int d = a; d < KP; ++d, ++i) {
                            const float pr = fmaf(c0, A[i], fmaf(q[d], G[a], q[a] * G[d]));
                            const float val = pr * fmaf(u[a], v[d], u[d] * w[a]);
                            A[i] = val;
                            Rn[a] += val;                         // row x: y ascending
                            if (d != a) Rn[d] += val;
                        }
                    float S = Rn[0];
#pragma unroll
                    for (int x = 1; x < KP; ++x) S += Rn[x];
                    const float inv = __builtin_amdgcn_rcpf(S);
#pragma unroll
                    for (int k = 0; k < T; ++k) A[k] *= inv;
#pragma unroll
                    for (int x = 0; x < KP; ++x) R[x] = Rn[x] * inv;
                    lsum += __builtin_amdgcn_logf(S);             // v_log_f32: log2
                    if (j0 + sl == next_out) {                    // (block-uniform)
                        float* dst = ckpt + (int64_t)o * T * lanes + bk.tile * LA_TILE + t;
#pragma unroll
                        for (int k = 0; k < T; ++k) dst[k * lanes] = A[k];
                        ++o;
                        next_out = o < o_end ? (int64_t)out_snp[o] : -1;
                    }
                }
            }
            llv += (double)lsum * LA_LN2;
        }
    }
    if (rr.valid) ll[(int64_t)rr.posc * n_seg + bk.sg] = llv;
}

template <int KP>
__global__ __launch_bounds__(LA_TILE) void local_anc_bwd_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const int k_real, const float* __restrict__ Q, const int q_stride, const float eps, const float one_m_eps,
    const float* __restrict__ rho, const int32_t* __restrict__ seg, const int32_t* __restrict__ out_snp,
    const int32_t* __restrict__ oseg, const int n_out, const int tiles, const float* __restrict__ ckpt, float* __restrict__ dosage,
    uint8_t* __restrict__ call, float* __restrict__ post) {
    constexpr int T = la_pairs(KP);
    constexpr int SW = (T + 31) / 32;
    __shared__ __attribute__((aligned(16))) float Ps[RANGE_CHUNK * KP];
    __shared__ float Rs[RANGE_CHUNK];
    const int t = threadIdx.x;
    const LaBlock bk = la_block(seg, tiles);
    const int o_lo = max(oseg[bk.sg], 0);
    int o = min(oseg[bk.sg + 1], n_out) - 1;
    if (o < o_lo || bk.s0 >= bk.s1) return;                       // (block-uniform) a segment without output points
    const int64_t first = out_snp[o_lo];                          // nothing below the first output point is needed
    int64_t next_out = out_snp[o];
    const RangeRow rr = range_row(xp, ld, idx, bk.tile * LA_TILE + t, b);
    const uint32_t inval = ~rr.valid;
    const bool wave_live = bk.tile * LA_TILE + (t & ~63) < b;     // wave-uniform
    const int64_t lanes = (int64_t)tiles * LA_TILE;

    float q[KP];
    load_row<KP>(Q + (int64_t)rr.posc * q_stride, q);
    // sup(x, y) = q_x q_y > 0, a bit per pair; b at the segment's last SNP is sup
    uint32_t sup[SW];
#pragma unroll
    for (int i = 0; i < SW; ++i) sup[i] = 0u;
    float B[T];
    {
        int i = 0;
#pragma unroll
        for (int a = 0; a < KP; ++a)
#pragma unroll
            for (int d = a; d < KP; ++d, ++i) {
                const bool on = q[a] * q[d] > 0.f;
                sup[i >> 5] |= on ? 1u << (i & 31) : 0u;
                B[i] = on ? 1.f : 0.f;
            }
    }

    const int64_t c_lo = first / RANGE_CHUNK, c_hi = (bk.s1 + RANGE_CHUNK - 1) / RANGE_CHUNK;
    u32x4_t nxt[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, c_hi - 1, v, ld);
#pragma unroll 1
    for (int64_t c = c_hi - 1; c >= c_lo; --c) {
        const int64_t j0 = c * RANGE_CHUNK;
        if (c < c_hi - 1) __syncthreads();                        // the previous chunk's rows have been read
        stage_rows<RANGE_CHUNK, KP, LA_TILE>(P, j0, M, Ps);
        la_stage_rho(rho, j0, M, -1, Rs);
        uint32_t wd[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) wd[i] = nxt[i >> 2][i & 3] | inval;
        {
            const int64_t cn = max(c - 1, c_lo);                  // the chunk below, in flight under this chunk's arithmetic
#pragma unroll
            for (int v = 0; v < 4; ++v) nxt[v] = range_piece(rr.x, cn, v, ld);
        }
        __syncthreads();
        if (!wave_live) continue;
        const int lo = (int)max(first - j0, (int64_t)0), hi = (int)min(bk.s1 - j0, (int64_t)RANGE_CHUNK);
#pragma unroll 1
        for (int wi = ((hi + 15) >> 4) - 1; wi >= lo >> 4; --wi) {
            const uint32_t bits = chunk_word(wd, wi, M - (j0 + 16 * wi));
            const int e_lo = max(lo - 16 * wi, 0), e_hi = min(hi - 16 * wi, 16);
#pragma unroll 1
            for (int e = e_hi - 1; e >= e_lo; --e) {
                const int sl = wi * 16 + e;
                if (j0 + sl == next_out) {                        // (block-uniform) gamma = a b / sum(a b), from the checkpoint
                    const float* src = ckpt + (int64_t)o * T * lanes + bk.tile * LA_TILE + t;
                    float D[KP];
#pragma unroll
                    for (int x = 0; x < KP; ++x) D[x] = 0.f;
                    float best = -1.f;
                    int bi = 0, i = 0;
#pragma unroll
                    for (int a = 0; a < KP; ++a)
#pragma unroll
                        for (int d = a; d < KP; ++d, ++i) {
                            const float g = src[i * lanes] * B[i];
                            D[a] += g;                            // row x: y ascending
                            if (d != a) D[d] += g;
                            const float mass = d == a ? g : g + g;        // of the unordered pair; a pad pair has 0 and never wins
                            const int ci = a * k_real - a * (a - 1) / 2 + (d - a);
                            if (mass > best) { best = mass; bi = ci; }     // strictly: the lowest index wins a tie
                        }
                    float Z = D[0];
#pragma unroll
                    for (int x = 1; x < KP; ++x) Z += D[x];
                    const float inv = __builtin_amdgcn_rcpf(Z);
                    const bool ok = Z > 0.f && Z < __builtin_inff();      // a NaN fails both
                    const float bad = __builtin_nanf("");
                    if (rr.valid) {
                        const int64_t pt = (int64_t)rr.posc * n_out + o;
                        float* dr = dosage + pt * KP;
#pragma unroll
                        for (int x = 0; x < KP; x += 4) {
                            float dv[4];
#pragma unroll
                            for (int z = 0; z < 4; ++z)
                                dv[z] = x + z >= k_real ? 0.f : (ok ? fminf(2.f * (D[x + z] * inv), 2.f) : bad);
                            *reinterpret_cast<float4*>(dr + x) = make_float4(dv[0], dv[1], dv[2], dv[3]);
                        }
                        call[pt] = ok ? (uint8_t)bi : (uint8_t)255;
                        post[pt] = ok ? best * inv : bad;
                    }
                    --o;
                    next_out = o >= o_lo ? (int64_t)out_snp[o] : -1;
                }
                if (j0 + sl <= first) continue;                   // (block-uniform) the first output point is the walk's end
                // from SNP j to j - 1: h = b e_j, H_x = sum_y q_y h(x, y), Tt = sum_x q_x H_x,
                // b(x, y) = sup (c0 h + J_x + J_y) with J_x = c1 H_x + (c2 / 2) Tt and rho[j], then normalised by its ordered sum
                float u[KP], v[KP], w[KP];
                la_factors<KP>(Ps + sl * KP, (bits >> (2 * e)) & 3u, eps, one_m_eps, u, v, w);
                const float r = Rs[sl], s = 1.f - r;
                const float c0 = s * s, c1 = r * s, hc2 = 0.5f * (r * r);
                float H[KP];
#pragma unroll
                for (int x = 0; x < KP; ++x) H[x] = 0.f;
                int i = 0;
#pragma unroll
                for (int a = 0; a < KP; ++a)
#pragma unroll
                    for (int d = a; d < KP; ++d, ++i) {
                        const float h = B[i] * fmaf(u[a], v[d], u[d] * w[a]);
                        B[i] = h;
                        H[a] = fmaf(q[d], h, H[a]);               // row x: y ascending
                        if (d != a) H[d] = fmaf(q[a], h, H[d]);
                    }
                float Tt = 0.f;
#pragma unroll
                for (int x = 0; x < KP; ++x) Tt = fmaf(q[x], H[x], Tt);
                const float hT = hc2 * Tt;
                float J[KP];
#pragma unroll
                for (int x = 0; x < KP; ++x) J[x] = fmaf(c1, H[x], hT);
                float Zd = 0.f, Zo = 0.f;                         // the diagonal and the upper triangle, a-major
                i = 0;
#pragma unroll
                for (int a = 0; a < KP; ++a)
#pragma unroll
                    for (int d = a; d < KP; ++d, ++i) {
                        const uint32_t m = (uint32_t)((int32_t)(sup[i >> 5] << (31 - (i & 31))) >> 31);
                        const float val = keepf(fmaf(c0, B[i], J[a] + J[d]), m);
                        B[i] = val;
                        if (d == a) Zd += val; else Zo += val;
                    }
                const float inv = __builtin_amdgcn_rcpf(fmaf(2.f, Zo, Zd));
#pragma unroll
                for (int k = 0; k < T; ++k) B[k] *= inv;
            }
        }
    }
}

static bool la_kp_ok(int kp) { return kp >= 4 && kp <= LA_MAX_KP && kp % 4 == 0; }
static int64_t la_tiles(int b) { return ((int64_t)b + LA_TILE - 1) / LA_TILE; }

}  // namespace nadm

using namespace nadm;

// scratch: the checkpoints [n_out][kp (kp + 1) / 2][tiles x 256] (one point's worth where n_out = 0); 0 for a width without a kernel
extern "C" int64_t nadm_local_anc_scratch_floats(int32_t b, int64_t n_out, int32_t kp) {
    if (b <= 0 || n_out < 0 || !la_kp_ok(kp)) return 0;
    return (n_out > 0 ? n_out : 1) * la_pairs(kp) * la_tiles(b) * LA_TILE;
}

extern "C" int nadm_local_anc(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k,
                              int32_t kp, const float* Q, int32_t q_stride, float eps, const float* rho, const int32_t* seg,
                              int32_t n_seg, const int32_t* out_snp, const int32_t* oseg, int64_t n_out, float* dosage, uint8_t* call,
                              float* post, double* ll, float* scratch, void* stream) {
    const char* who = "nadm_local_anc";
    const bool full = dosage != nullptr;
    if (!xp || !P || !Q || !rho || !seg || !ll) return failf(who, "null pointer");
    if (full && (!call || !post || !scratch || !out_snp || !oseg)) return failf(who, "null pointer (a full call needs call, post, scratch, out_snp and oseg)");
    if (b <= 0 || M <= 0) return failf(who, "empty batch (need b > 0 and M > 0)");
    if (M > 0x7FFFFFFFll) return failf(who, "M must be < 2^31 (seg and out_snp are int32)");
    if (check_packed(who, ld, M) || check_head(who, k, kp, q_stride) || check_eps(who, eps)) return 1;
    if (kp > LA_MAX_KP) return failf(who, "K must be <= 16 (the K (K + 1) / 2 states of a sample live in one thread's registers)");
    if (n_seg < 1) return failf(who, "n_seg must be >= 1");
    if (n_out < 0 || n_out > 0x7FFFFFFFll) return failf(who, "n_out must be in 0..2^31 - 1");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)Q | (uintptr_t)scratch | (uintptr_t)dosage) & 15) != 0)
        return failf(who, "xp, P, Q, scratch and dosage must be 16-byte aligned");
    if (((uintptr_t)ll & 7) != 0 ||
        (((uintptr_t)rho | (uintptr_t)seg | (uintptr_t)out_snp | (uintptr_t)oseg | (uintptr_t)post | (uintptr_t)idx) & 3) != 0)
        return failf(who, "ll must be 8-byte and rho, seg, out_snp, oseg, post, idx 4-byte aligned");
    const int64_t tiles = la_tiles(b);
    if (tiles * n_seg > 0x7FFFFFFFll) return failf(who, "too many blocks for one launch");
    hipStream_t st = (hipStream_t)stream;
    const float ome = 1.f - eps;
    const dim3 grid((unsigned)(tiles * n_seg));
    float* ckpt = full && n_out > 0 ? scratch : nullptr;
    if (int e = dispatch_kp(who, kp, [&](auto KP) {
            if constexpr (decltype(KP)::value <= LA_MAX_KP)
                hipLaunchKernelGGL((local_anc_fwd_kernel<decltype(KP)::value>), grid, dim3(LA_TILE), 0, st, xp, ld, idx, b, M, P, Q, q_stride,
                                   eps, ome, rho, seg, n_seg, out_snp, oseg, (int)n_out, (int)tiles, ckpt, ll);
        }))
        return e;
    if (int e = check_launch("local_anc (forward)")) return e;
    if (!ckpt) return 0;
    dispatch_kp(who, kp, [&](auto KP) {
        if constexpr (decltype(KP)::value <= LA_MAX_KP)
            hipLaunchKernelGGL((local_anc_bwd_kernel<decltype(KP)::value>), grid, dim3(LA_TILE), 0, st, xp, ld, idx, b, M, P, k, Q, q_stride,
                               eps, ome, rho, seg, out_snp, oseg, (int)n_out, (int)tiles, scratch, dosage, call, post);
    });
    return check_launch("local_anc (backward)");
}
