// Projection: refine Q against a FIXED P with masked EM steps of the binomial admixture model (include/nadm.h, nadm_project_q).
//
// Two launches per step, no floating-point atomics (two launches on the same inputs give the same bits):
//   project_accum_kernel  one wave per (256-SNP chunk, 64-sample tile): a lane owns one sample, keeps its q and its sums a_k in
//                         registers, reads its row's 64 bytes of the chunk with four 16-byte loads and decodes the 2-bit codes in
//                         registers; the chunk's P rows sit in LDS once per block and every lane reads the SAME row (a broadcast).
//                         Missing calls (code 3) and SNPs >= M enter every sum as exactly +0.0f.  Writes the chunk's partials of
//                         a_k (fp32), n (int32) and, when asked, ll (fp32).
//                         The WEIGHTED form (nadm_project_q_w, bootstrap replicates) multiplies every SNP's terms by its count w_j:
//                         the chunk's 256 weight bytes sit in LDS next to the P rows and every lane reads the same byte; a chunk
//                         whose weights are all zero writes +0.0f / 0 partials and returns (wave-uniform).
//   project_fold_kernel   one wave per sample: adds the partials over the chunks in a fixed order (a, ll in float64) and applies
//                         q'_k = q_k a_k / (2n), the floor qmin, the renormalisation.
#include "nadm_chunk_ranges.h"

namespace nadm {

constexpr int PROJ_CHUNK = RANGE_CHUNK;      // SNPs per chunk = 64 bytes of a packed row = four 16-byte loads
constexpr int PROJ_TILE = 64;        // samples per block (one wave, a lane per sample)

// KP <= 16: the whole chunk of P is staged at once (16 KB at KP = 16); wider heads stage 64 SNPs at a time (16 KB at KP = 64)
template <int KP> struct ProjStage { static constexpr int SNPS = KP <= 16 ? PROJ_CHUNK : 64; };

// the chunk's weights in LDS, one byte per SNP (the WEIGHTED instantiations only: the others never name it and get no LDS for it)
__device__ __forceinline__ uint32_t* proj_weight_lds() {
    __shared__ __attribute__((aligned(16))) uint32_t Wl[PROJ_CHUNK / 4];
    return Wl;
}

template <int KP, bool WITH_LL, bool WEIGHTED>
__global__ __launch_bounds__(PROJ_TILE) void project_accum_kernel(
    const uint8_t* __restrict__ xp, const int64_t ld, const int32_t* __restrict__ idx, const int b, const int64_t M,
    const float* __restrict__ P, const float* __restrict__ Qin, const int q_stride, const float eps, const float one_m_eps,
    const int tiles, float* __restrict__ apart, int32_t* __restrict__ npart, float* __restrict__ llpart,
    const uint8_t* __restrict__ wts) {
    constexpr int STAGE = ProjStage<KP>::SNPS;
    __shared__ __attribute__((aligned(16))) float Ps[STAGE * KP];
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - chunk * tiles);
    const int s = tile * PROJ_TILE + lane;
    const bool live = s < b;
    const int64_t j0 = chunk * PROJ_CHUNK;

    if constexpr (WEIGHTED) {
        // lane l brings the weights of SNPs j0 + 4l .. j0 + 4l + 3 (no byte at or beyond M is read; those SNPs are masked anyway)
        const int64_t jw = j0 + 4 * lane;
        uint32_t ww = 0u;
        if (jw + 4 <= M) {
            ww = *reinterpret_cast<const uint32_t*>(wts + jw);
        } else {
            for (int t = 0; t < 4; ++t)
                if (jw + t < M) ww |= (uint32_t)wts[jw + t] << (8 * t);
        }
        if (__ballot(ww != 0u) == 0ull) {                       // nothing of this chunk was drawn: the sums the long way are +0.0f / 0
            if (live) {
                const int64_t o = chunk * b + s;
#pragma unroll
                for (int k = 0; k < KP; k += 4) *reinterpret_cast<float4*>(apart + o * KP + k) = make_float4(0.f, 0.f, 0.f, 0.f);
                npart[o] = 0;
                if constexpr (WITH_LL) llpart[o] = 0.f;
            }
            return;
        }
        proj_weight_lds()[lane] = ww;                           // visible after the first stage's barrier
    }

    // this lane's row: the chunk's 64 bytes (16-byte pieces past the row's end read as zeros; their SNPs are >= M anyway)
    uint32_t w[16];
    {
        const int64_t row = live ? (idx ? (int64_t)idx[s] : (int64_t)s) : 0;
        const uint8_t* rp = xp + row * ld + chunk * (PROJ_CHUNK / 4);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            if (live && chunk * (PROJ_CHUNK / 4) + 16 * (v + 1) <= ld) u = *reinterpret_cast<const uint4*>(rp + 16 * v);
            w[4 * v] = u.x; w[4 * v + 1] = u.y; w[4 * v + 2] = u.z; w[4 * v + 3] = u.w;
        }
    }
    float q[KP], a[KP];
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) t = *reinterpret_cast<const float4*>(Qin + (int64_t)s * q_stride + k);
        q[k] = t.x; q[k + 1] = t.y; q[k + 2] = t.z; q[k + 3] = t.w;
        a[k] = a[k + 1] = a[k + 2] = a[k + 3] = 0.f;
    }
    float ll = 0.f;
    int n = 0;

#pragma unroll 1
    for (int st = 0; st < PROJ_CHUNK / STAGE; ++st) {
        // the stage's P rows into LDS (rows >= M as zeros): STAGE * KP / 4 float4, coalesced
        if (st) __syncthreads();
        {
            const int64_t jb = j0 + (int64_t)st * STAGE;
            const float4* src = reinterpret_cast<const float4*>(P + jb * KP);
            const int64_t lim = (M - jb) * (KP / 4);            // float4 of the stage that exist
            for (int e = lane; e < STAGE * KP / 4; e += PROJ_TILE)
                reinterpret_cast<float4*>(Ps)[e] = e < lim ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
#pragma unroll 1
        for (int wd = 0; wd < STAGE / 16; ++wd) {               // one 32-bit word = 16 SNPs
            const int wi = st * (STAGE / 16) + wd;
            const uint32_t bits = chunk_word(w, wi, M - (j0 + 16 * wi));     // SNPs >= M as code 3: the element loop masks on the code alone
            float llw = 0.f;
#pragma unroll 4
            for (int t = 0; t < 16; ++t) {
                const uint32_t code = (bits >> (2 * t)) & 3u;
                const uint32_t m = obs_mask(code);
                const float* pr = Ps + (wd * 16 + t) * KP;
                float p[KP];
                EmTerms e = em_terms(dot_row<KP>(q, pr, p), code, m, eps, one_m_eps);
                uint32_t wj = 1u;
                float wf = 1.f;
                if constexpr (WEIGHTED) {                        // every lane reads the same byte: a broadcast
                    wj = reinterpret_cast<const uint8_t*>(proj_weight_lds())[wi * 16 + t];
                    wf = (float)wj;
                    e.t1 *= wf;
                    e.t0 *= wf;
                }
                // both terms as they stand: (1 - p_jk) / (1 - r_j) <= 1 / q_k however small 1 - r_j gets, whereas the cheaper
                // sum_j t0_j + sum_j p_jk (t1_j - t0_j) cancels two sums of ~1/eps when a row of P is all ones
#pragma unroll
                for (int k = 0; k < KP; ++k) a[k] = fmaf(1.f - p[k], e.t0, fmaf(p[k], e.t1, a[k]));
                if constexpr (WEIGHTED) n += (int)(wj & m);
                else n += (int)(m & 1u);
                if constexpr (WITH_LL) {                                                               // v_log_f32; ln 2 once per word
                    if constexpr (WEIGHTED) llw = fmaf(wf, keepf(e.g * __log2f(e.r) + e.h * __log2f(e.u), m), llw);
                    else llw += keepf(e.g * __log2f(e.r) + e.h * __log2f(e.u), m);
                }
            }
            if constexpr (WITH_LL) ll += llw * 0.693147180559945f;
        }
    }
    if (!live) return;
    const int64_t o = chunk * b + s;
#pragma unroll
    for (int k = 0; k < KP; k += 4)
        *reinterpret_cast<float4*>(apart + o * KP + k) = make_float4(a[k], a[k + 1], a[k + 2], a[k + 3]);
    npart[o] = n;
    if constexpr (WITH_LL) llpart[o] = ll;
}

// One wave per sample.  Lane l holds column k = l % KW (KW = 16 for kp <= 16, else 64) and sums the chunks of part l / KW in chunk
// order; the parts are then added in part order.  n and ll: lane l takes chunks l, l + 64, ..., then a fixed butterfly.
__global__ __launch_bounds__(64) void project_fold_kernel(const float* __restrict__ apart, const int32_t* __restrict__ npart,
                                                          const float* __restrict__ llpart, const int64_t chunks, const int b, const int k,
                                                          const int kp, const float* Qin, float* Qout,   /* may alias */
                                                          const int q_stride, const float qmin, double* __restrict__ loglik,
                                                          int32_t* __restrict__ nobs) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int KW = kp <= 16 ? 16 : 64, parts = 64 / KW;
    const int col = lane & (KW - 1), part = lane / KW;
    const int64_t per = (chunks + parts - 1) / parts;
    const int64_t c_lo = part * per, c_hi = (c_lo + per < chunks) ? c_lo + per : chunks;
    double acc = 0.0;
    if (col < kp)
        for (int64_t c = c_lo; c < c_hi; ++c) acc += (double)apart[(c * b + s) * kp + col];
    double tot = 0.0;
    for (int pt = 0; pt < parts; ++pt) tot += __shfl(acc, pt * KW + col, 64);
    int n = 0;
    double ll = 0.0;
    for (int64_t c = lane; c < chunks; c += 64) {
        n += npart[c * b + s];
        if (llpart) ll += (double)llpart[c * b + s];
    }
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o, 64);
        ll += __shfl_xor(ll, o, 64);
    }
    const float qi = (col < kp) ? Qin[(int64_t)s * q_stride + col] : 0.f;
    float out = qi;                                              // n == 0: the row is returned as it came
    if (n > 0) {
        double qn = (col < k) ? (double)qi * tot / (2.0 * (double)n) : 0.0;
        if (col < k && qn < (double)qmin) qn = (double)qmin;
        double sum = qn;
        for (int o = 1; o < KW; o <<= 1) sum += __shfl_xor(sum, o, 64);
        out = (float)(qn / sum);
    }
    if (part == 0 && col < kp) Qout[(int64_t)s * q_stride + col] = out;
    if (lane == 0) {
        if (loglik) loglik[s] = (n > 0) ? ll : 0.0;
        if (nobs) nobs[s] = n;
    }
}

template <int KP, bool WEIGHTED>
static void launch_accum(bool with_ll, unsigned grid, hipStream_t st, const uint8_t* xp, int64_t ld, const int32_t* idx, int b, int64_t M,
                         const float* P, const float* Qin, int q_stride, float eps, int tiles, float* apart, int32_t* npart, float* llpart,
                         const uint8_t* wts) {
    const float ome = 1.f - eps;
    if (with_ll)
        hipLaunchKernelGGL((project_accum_kernel<KP, true, WEIGHTED>), dim3(grid), dim3(PROJ_TILE), 0, st, xp, ld, idx, b, M, P, Qin, q_stride, eps,
                           ome, tiles, apart, npart, llpart, wts);
    else
        hipLaunchKernelGGL((project_accum_kernel<KP, false, WEIGHTED>), dim3(grid), dim3(PROJ_TILE), 0, st, xp, ld, idx, b, M, P, Qin, q_stride, eps,
                           ome, tiles, apart, npart, llpart, wts);
}

static int64_t project_chunks(int64_t M) { return (M + PROJ_CHUNK - 1) / PROJ_CHUNK; }

}  // namespace nadm

using namespace nadm;

// scratch: a partials [chunks, b, kp] float | n partials [chunks, b] int32 | ll partials [chunks, b] float
extern "C" int64_t nadm_project_scratch_floats(int32_t b, int64_t M, int32_t kp) {
    if (b <= 0 || M <= 0 || kp <= 0 || kp > NADM_MAX_K) return 0;
    return project_chunks(M) * (int64_t)b * (kp + 2);
}

// both entries: `who` names the caller in a refusal, wts == NULL runs the unweighted instantiations
static int project_q_any(const char* who, const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k,
                         int32_t kp, const float* Qin, float* Qout, int32_t q_stride, float eps, float qmin, double* loglik, int32_t* nobs,
                         float* scratch, const uint8_t* wts, bool weighted, void* stream) {
    if (!xp || !P || !Qin || !Qout || !scratch || (weighted && !wts)) return failf(who, "null pointer");
    if (b <= 0 || M <= 0) return failf(who, "empty batch (need b > 0 and M > 0)");
    if (check_packed(who, ld, M) || check_head(who, k, kp, q_stride) || check_eps(who, eps)) return 1;
    if (!(qmin >= 0.f && qmin < 1.f)) return failf(who, "qmin must be in [0, 1)");
    if ((((uintptr_t)xp | (uintptr_t)P | (uintptr_t)Qin | (uintptr_t)Qout | (uintptr_t)scratch) & 15) != 0)
        return failf(who, "xp, P, Qin, Qout and scratch must be 16-byte aligned");
    if (weighted && ((uintptr_t)wts & 15) != 0) return failf(who, "w must be 16-byte aligned");
    const int64_t chunks = project_chunks(M);
    const int tiles = (b + PROJ_TILE - 1) / PROJ_TILE;
    if (chunks * tiles > 0x7FFFFFFFll) return failf(who, "too many (chunk, tile) blocks for one launch");
    float* apart = scratch;
    int32_t* npart = reinterpret_cast<int32_t*>(scratch + chunks * b * kp);
    float* llpart = loglik ? scratch + chunks * b * (kp + 1) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(chunks * tiles);
    const bool wl = loglik != nullptr;
    if (int e = dispatch_kp(who, kp, [&](auto KP) {
            if (weighted)
                launch_accum<decltype(KP)::value, true>(wl, grid, st, xp, ld, idx, b, M, P, Qin, q_stride, eps, tiles, apart, npart, llpart, wts);
            else
                launch_accum<decltype(KP)::value, false>(wl, grid, st, xp, ld, idx, b, M, P, Qin, q_stride, eps, tiles, apart, npart, llpart,
                                                         nullptr);
        }))
        return e;
    if (int e = check_launch("project_q (accumulate)")) return e;
    hipLaunchKernelGGL(project_fold_kernel, dim3((unsigned)b), dim3(64), 0, st, apart, npart, llpart, chunks, b, k, kp, Qin, Qout, q_stride, qmin,
                       loglik, nobs);
    return check_launch("project_q (fold)");
}

extern "C" int nadm_project_q(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k, int32_t kp,
                              const float* Qin, float* Qout, int32_t q_stride, float eps, float qmin, double* loglik, int32_t* nobs,
                              float* scratch, void* stream) {
    return project_q_any("nadm_project_q", xp, ld, idx, b, M, P, k, kp, Qin, Qout, q_stride, eps, qmin, loglik, nobs, scratch, nullptr, false,
                         stream);
}

extern "C" int nadm_project_q_w(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* P, int32_t k, int32_t kp,
                                const float* Qin, float* Qout, int32_t q_stride, float eps, float qmin, double* loglik, int32_t* nobs,
                                float* scratch, const uint8_t* w, void* stream) {
    return project_q_any("nadm_project_q_w", xp, ld, idx, b, M, P, k, kp, Qin, Qout, q_stride, eps, qmin, loglik, nobs, scratch, w, true,
                         stream);
}
