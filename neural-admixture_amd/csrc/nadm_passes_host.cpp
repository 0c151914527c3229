// The host side of the three genotype passes and the MLP pair: the public entry points, their argument checks, the rules that decide which
// kernel runs with how many slices and which grid, and the size queries.  Every public form is an adapter that fills the launch's struct
// (nadm_pass_args.h) and calls the pass's one checked path; the plan's step (nadm_step.hip) fills the same structs.  The kernels and the
// launchers are in nadm_genotype_passes.hip and nadm_small_kernels.hip.  Plain C++: no HIP call, no HIP header (host_selfcheck.cpp links
// this unit against launchers that only record what they are given).
#include "nadm_host_rules.h"

using namespace nadm;

// =================================================================================================
// chunk, image and slab sizes
// =================================================================================================
// The matrix-core kernels of passes 1 and 3 cover CP <= 8; wider encoders (n_components > 8) run the VALU kernels.
// The chunk count must not depend on CP (callers size zpart before they pass CP): both pass-1 kernels write 2048-SNP chunks.
extern "C" int64_t nadm_encode_chunks(int64_t M) { return (M + EM_CHUNK_SNPS - 1) / EM_CHUNK_SNPS; }

extern "C" int32_t nadm_decode_chunk_snps(int kp) {
    if (kp <= 16) return mf_chunk_snps(kp);
    return 256 * dec_spl(kp);
}

extern "C" int64_t nadm_decode_chunks(int64_t M, int kp) {
    const int64_t c = nadm_decode_chunk_snps(kp);
    return (M + c - 1) / c;
}

extern "C" int64_t nadm_encode_bwd_chunks(int64_t M) { return (M + EB_CHUNK_SNPS - 1) / EB_CHUNK_SNPS; }

extern "C" int64_t nadm_q_image_bytes(int32_t b) { return (int64_t)((b + QI_TS - 1) / QI_TS) * QI_TILE_U4 * 16; }
extern "C" int64_t nadm_batch_copy_bytes(int32_t b, int64_t M) { return ((M + 4 * XG_TILE_COLS - 1) / (4 * XG_TILE_COLS)) * (int64_t)b * XG_TILE_COLS; }
extern "C" int64_t nadm_tiled_bytes(int64_t rows, int64_t M) {
    return rows > 0 && M > 0 ? ((M + 4 * XG_TILE_COLS - 1) / (4 * XG_TILE_COLS)) * rows * XG_TILE_COLS : 0;
}
extern "C" int64_t nadm_dz_image_tile_bytes(void) { return (int64_t)DZI_TILE_U4 * 16; }
extern "C" int64_t nadm_dz_image_bytes(int32_t b) { return (int64_t)((b + DZI_TS - 1) / DZI_TS) * DZI_TILE_U4 * 16; }

// =================================================================================================
// the tiled, cleaned copy of the matrix and the X source of a pass (XSource, nadm_pass_args.h)
// =================================================================================================
extern "C" int nadm_tile_packed(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, uint8_t* xt, void* stream) {
    if (!xp || !xt) return fail("nadm_tile_packed: null pointer");
    if (rows <= 0 || M <= 0) return fail("nadm_tile_packed: empty matrix");
    if (check_packed("nadm_tile_packed", ld, M)) return 1;
    if (rows >> 31) return fail("nadm_tile_packed: at most 2^31 - 1 rows (the passes' row indices are int32)");
    if (((uintptr_t)xp | (uintptr_t)xt) & 15) return fail("nadm_tile_packed: xp and xt must be 16-byte aligned");
    const uint8_t* xe = xp + rows * ld; const uint8_t* te = xt + nadm_tiled_bytes(rows, M);
    if (xp < te && xt < xe) return fail("nadm_tile_packed: xt overlaps xp");
    return launch_tile_packed(xp, ld, rows, M, xt, stream);
}

// a tiled source as the step hands it over (the public forms of the passes only build row-major ones): refused in the pass's name
static int tiled_source_args(const char* who, const XSource& x) {
    if (x.row_stride != XG_TILE_COLS || x.tile_stride < XG_TILE_COLS || x.tile_stride % XG_TILE_COLS != 0)
        return failf(who, "a tiled source has rows of 128 bytes and tiles of rows x 128 bytes");
    if ((uintptr_t)x.base & 15) return failf(who, "a tiled source must be 16-byte aligned");
    return 0;
}

// =================================================================================================
// sample slices, the host's side of slice_tiles (nadm_pass_args.h), shared by passes 2 and 3
// =================================================================================================
// the n_slices argument of a pass, refused in the entry point's own words (`no_kernel`: why this shape has no sliced kernel, or NULL)
static int slice_args(int32_t n_slices, int tiles, const float* slab, const int32_t* counters, const char* out_of_range, const char* no_kernel,
                      const char* no_slab, const char* empty_slice) {
    if (n_slices < 1 || n_slices > NADM_MAX_P2_SLICES) return fail(out_of_range);
    if (n_slices == 1) return 0;
    if (no_kernel) return fail(no_kernel);
    if (!slab || !counters || ((uintptr_t)slab & 15)) return fail(no_slab);
    return slices_leave_one_empty(tiles, n_slices) ? fail(empty_slice) : 0;
}
// the most slices any batch of up to bmax rows is cut into: the rule of the pass at every tile count
static int32_t slices_max(int32_t (*rule)(int32_t, int64_t, int32_t), int32_t bmax, int64_t M, int32_t width, int tile_rows) {
    int32_t mx = 1;
    for (int32_t b = bmax; b > 0; b -= tile_rows) { const int32_t s = rule(b, M, width); if (s > mx) mx = s; }
    return mx;
}

// ---- pass 2 with the batch's sample tiles dealt to n_slices blocks per SNP chunk (see decode_bce_bf16_kernel)
extern "C" int32_t nadm_decode_slices(int32_t b, int64_t M, int32_t kp) {
    if (kp > 16 || b <= 0 || M <= 0) return 1;
    const int64_t chunks = (M + mf_chunk_snps(8) - 1) / mf_chunk_snps(8);
    const int tiles = (b + NADM_BF_TS - 1) / NADM_BF_TS;
    int s = hook_p2_slices();                                       // 0 (always, in the shipping library): the rule below
    if (s == 0) {
        // Measured (profiles/r05_ablations.txt item 11): below ~130k SNPs pass 2 is bound by the serial chain of ONE block -- its prologue
        // (P rows into operands, ~1.5 tile-times) + 13 tiles at b = 800 = 49 us whether 98 or 196 blocks run -- not by the chip; slices of
        // ~4-5 tiles shorten the chain (M = 25k: 49 -> 32 us, 50k: 50 -> 43, 100k: 73.5 -> 66.5; 6400 rows x 62.5k SNPs, the SNP-sharded
        // rank of configs[3]: 326 -> 244).  A slice costs a prologue and the launch ~5 us for the hand-off: short batches (< 8 tiles: b = 400
        // at M = 100k 44.4 -> 45.3, b = 200 at 50k 20.9 -> 23.6) and launches of more than ~1.7 rounds of blocks do not pay; from 150k SNPs
        // on the chunks fill the chip and nothing changes.
        if (chunks >= 512 || tiles < 8) return 1;
        s = (int)((2 * tiles + 4) / 9);                             // round(tiles / 4.5)
        const int64_t lim = 1280 / chunks;                           // blocks <= 1280 = 1.7 rounds of 768
        if (s > lim) s = (int)lim;
        if (s > NADM_MAX_P2_SLICES) s = NADM_MAX_P2_SLICES;
    }
    return slices_without_empty(tiles, s);
}

extern "C" int32_t nadm_decode_slices_max(int32_t bmax, int64_t M, int32_t kp) { return slices_max(nadm_decode_slices, bmax, M, kp, NADM_BF_TS); }

extern "C" int64_t nadm_decode_slab_floats(int64_t M, int32_t kp, int32_t n_slices) {
    if (kp > 16 || n_slices < 2 || M <= 0) return 0;
    return (int64_t)n_slices * ((M + mf_chunk_snps(8) - 1) / mf_chunk_snps(8)) * p2_slab_floats(kp);
}

// ---- pass 3 with the batch's 128-sample tiles dealt to n_slices blocks per SNP chunk (see encode_bwd_fp4_kernel)
extern "C" int32_t nadm_encode_slices(int32_t b, int64_t M, int32_t cp) {
    if (cp > 8 || b <= 0 || M <= 0) return 1;
    const int64_t chunks = (M + EB_CHUNK_SNPS - 1) / EB_CHUNK_SNPS;
    const int tiles = (b + DZI_TS - 1) / DZI_TS;
    int s = hook_p3_slices();                                       // 0 (always, in the shipping library): the rule below
    if (s == 0) {
        // Measured (profiles/r06_p3_slices.txt): a launch of ~120 chunk blocks that each walk 50 tiles (6400 rows x 62.5k SNPs, the SNP-sharded
        // rank of configs[3] on 8 GPUs) lasts as long as one block's chain, 77 us where the same genotypes as 977 blocks take 41; two slices
        // 57 us, three 62, four 64, eight 76 -- every slice pays a prologue and the hand-off (park 16 KB through to memory, be counted, the
        // last one reads them all back and runs Adam: ~8 us of tail).  At 3200 x 125k (245 chunks x 25 tiles, 46 us) any cut loses: 53 / 65.
        // So: two slices, only for few chunks AND long chains; every single-GPU BASELINE shape stays whole.
        if (chunks >= 192 || tiles < 32) return 1;
        s = 2;
    }
    return slices_without_empty(tiles, s);
}

extern "C" int32_t nadm_encode_slices_max(int32_t bmax, int64_t M, int32_t cp) { return slices_max(nadm_encode_slices, bmax, M, cp, DZI_TS); }

extern "C" int64_t nadm_encode_slab_floats(int64_t M, int32_t cp, int32_t n_slices) {
    if (cp > 8 || n_slices < 2 || M <= 0) return 0;
    return (int64_t)n_slices * ((M + EB_CHUNK_SNPS - 1) / EB_CHUNK_SNPS) * p3_slab_floats(cp);
}

// =================================================================================================
// the optional Adam state of a fused epilogue
// =================================================================================================
static int adam_fused_args(const nadm_adam_t* adam, const char* who, AdamFused* out) {
    *out = AdamFused{nullptr, nullptr, 0.f, 0.f, 0.f};
    if (!adam) return 0;
    if (!adam->m || !adam->v) return failf(who, "Adam state is NULL");
    if (adam->step < 1) return fail("nadm_*_step: Adam step is 1-based");
    if (((uintptr_t)adam->m | (uintptr_t)adam->v) & 15) return fail("nadm_*_step: Adam state must be 16-byte aligned");
    out->m = adam->m; out->v = adam->v; out->grad_scale = adam->grad_scale;
    if (adam->reserved != 0) return fail("nadm_*_step: nadm_adam_t.reserved must be 0");
    adam_scalars(adam->lr, adam->step, &out->step_size, &out->inv_bc2);
    return 0;
}

// =================================================================================================
// pass 1
// =================================================================================================
// Every block of the matrix-core kernel first splits its 2048 x CP slice of V into bf16 operands (about as much work as 11 sample tiles),
// so a block should see many tiles; but the 512 block slots of the chip (2 per CU) want to be filled, and a partly filled last round
// costs most of a full one.  grid.y = the number of batch splits (never fewer than 4 tiles per block) that minimises
//   rounds_eff(chunks * gy / slots) * (11.3 + tiles / gy),   slots = 2 blocks per CU of the device the launch goes to (512 on an
//   MI355X in SPX mode; a partition or another SKU reports its own CU count)
// with rounds_eff() read off measured launches (profiles/r03_p1_batch_splits.txt: b = 800, M = 500k .. 1M, grid.y = 1..4; the
// model reproduces all twenty within 2 us except one): a block alone on its CU runs 1.5 x faster, a round that is a
// little over-full costs 1.4 rounds.  M = 500k: 2 splits (43.6 us; 1 / 3 / 4: 49.1 / 47.7 / 49.0), 600k: 3 (56.1; 60.0 with
// the 2 that r02's rule "as few splits as give 480 blocks" picked), 800k: 1 (70.9; 73.3 with 2), 1M: 1 (73.6).
// (A launch that is one PART of a pass shares the device with the other parts: the split is the whole pass's, nadm_encode_fwd_part.)
int nadm::pass1_batch_splits(int32_t b, int64_t chunks, int64_t total_chunks, int cu_count, int* tpb_out) {
    const int ntiles = (b + 15) / 16;
    auto rounds_eff = [](double x) {
        if (x <= 0.5) return 0.67;
        if (x <= 1.0) return 0.92 + 0.16 * (x - 0.5);
        if (x <= 1.5) return 1.40;
        if (x <= 1.95) return 1.70;
        if (x <= 2.0) return 2.00;
        return 0.45 + 0.72 * x;
    };
    const double slots = 2.0 * (double)cu_count;
    const int64_t fill_chunks = total_chunks > chunks ? total_chunks : chunks;
    int64_t gy = 1;
    double best = 1e30;
    for (int64_t g = 1; g <= 64 && g <= (ntiles + 3) / 4; ++g) {
        const double cost = rounds_eff((double)(fill_chunks * g) / slots) * (11.3 + (double)((ntiles + g - 1) / g));
        if (cost < best) { best = cost; gy = g; }
    }
    int tpb = (int)((ntiles + gy - 1) / gy);
    if (tpb > EM_TILES_PER_BLOCK) tpb = EM_TILES_PER_BLOCK;
    *tpb_out = tpb;
    return (ntiles + tpb - 1) / tpb;
}

int nadm::pass1_small_args(Pass1Launch& a, const float* small_part, int32_t splits, int32_t n_small, float* grad_small, float* small,
                           const nadm_adam_t* adam) {
    if (!small_part || !grad_small) return fail("nadm_encode_fwd_small: null pointer");
    if (splits <= 0 || n_small <= 0) return fail("nadm_encode_fwd_small: empty");
    SmallSide ss{small_part, grad_small, small, nullptr, nullptr, splits, n_small, 0.f, 0.f, 0.f};
    if (adam) {
        if (!adam->m || !adam->v || !small) return fail("nadm_encode_fwd_small: Adam state / parameters are NULL");
        if (adam->step < 1) return fail("nadm_encode_fwd_small: Adam step is 1-based");
        ss.m = adam->m; ss.v = adam->v; ss.grad_scale = adam->grad_scale;
        adam_scalars(adam->lr, adam->step, &ss.step_size, &ss.inv_bc2);
    }
    a.ss = ss;
    return 0;
}

int nadm::pass1(Pass1Launch a) {
    if (!a.x.base || !a.idx || !a.V || !a.zpart) return fail("nadm_encode_fwd: null pointer");
    if (a.b <= 0 || a.M <= 0) return fail("nadm_encode_fwd: empty batch or M");
    if (a.x.clean) {
        if (tiled_source_args("nadm_encode_fwd", a.x)) return 1;
        if (a.missing_bf16 != 0u) return fail("nadm_encode_fwd: a missing call read as 1.5 needs the row-major matrix (the tiled copy holds no code 3)");
        if (a.CP > 8) return fail("nadm_encode_fwd: the tiled copy feeds the matrix-core pass only (C <= 8)");
    } else {
    if (a.x.row_stride % 16 != 0 || a.x.row_stride * 4 < a.M) return fail("nadm_encode_fwd: ld must be a multiple of 16 and >= ceil(M/4)");
    if (a.x.row_stride >> 32) return fail("nadm_encode_fwd: rows of 4 GiB and more (ld >= 2^32) are not supported");      // the matrix pass forms row addresses from 32-bit factors
    }
    a.chunks = nadm_encode_chunks(a.M);
    if (a.CP <= 8) {
        a.gy = pass1_batch_splits(a.b, a.chunks, a.total_chunks, device_cu_count(), &a.tpb);
        a.side_blocks = a.ss.part ? (a.ss.n + 511) / 512 : 0;
        return launch_pass1(a);
    }
    if (a.ss.part) return fail("nadm_encode_fwd_small: only the matrix-core pass (CP <= 8) hosts the side blocks");
    if (a.CP != 12 && a.CP != 16 && a.CP != 24 && a.CP != 32) return fail("nadm_encode_fwd: unsupported CP (4,8,12,16,24,32)");
    a.medium = false;                                   // (the VALU kernel is the same under either precision)
    return launch_pass1(a);
}

extern "C" int nadm_encode_fwd(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                               const float* V, int32_t CP, float* zpart, void* stream) {
    return pass1(Pass1Launch{x_rows(xp, ld), idx, b, M, V, CP, zpart, 0, 0u, false, SmallSide{}, stream});
}

extern "C" int nadm_encode_fwd_part(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                    const float* V, int32_t CP, float* zpart, int64_t total_chunks, void* stream) {
    return pass1(Pass1Launch{x_rows(xp, ld), idx, b, M, V, CP, zpart, total_chunks, 0u, false, SmallSide{}, stream});
}

extern "C" int nadm_encode_fwd_small(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                     const float* V, int32_t CP, float* zpart, const float* small_part, int32_t splits, int32_t n_small,
                                     float* grad_small, float* small, const nadm_adam_t* adam, void* stream) {
    Pass1Launch a{x_rows(xp, ld), idx, b, M, V, CP, zpart, 0, 0u, false, SmallSide{}, stream};
    if (pass1_small_args(a, small_part, splits, n_small, grad_small, small, adam)) return 1;
    return pass1(a);
}

extern "C" int nadm_pca_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                const float* V, int32_t CP, float* zpart, void* stream) {
    if (CP > 8) return fail("nadm_pca_project: only the matrix-core pass (CP <= 8) has the missing = 1.5 variant");
    return pass1(Pass1Launch{x_rows(xp, ld), idx, b, M, V, CP, zpart, 0, 0x3FC0u, false, SmallSide{}, stream});
}

// =================================================================================================
// pass 2
// =================================================================================================
int nadm::pass2_step_args(Pass2Launch& a, const char* who, const nadm_adam_t* adam, bool p_aligned_without_adam) {
    if (adam_fused_args(adam, who, &a.ad)) return 1;
    if ((a.ad.m || p_aligned_without_adam) && ((uintptr_t)a.P & 15)) return failf(who, "P must be 16-byte aligned");
    return 0;
}

int nadm::pass2(Pass2Launch a) {
    if (!a.x.base || !a.idx || !a.P || !a.Q || !a.dP || !a.dqpart) return fail("nadm_decode_bce: null pointer");
    if (a.medium && a.kp <= 16 && (!a.qimg || NADM_BF_TS != QI_TS))        // (kp > 16: the VALU kernel, the same under either precision)
        return fail("nadm_step: precision \"medium\" runs pass 2 from the Q images (nadm_plan_desc_t.qimg) at padded K <= 16");
    if (a.x.clean) {
        if (tiled_source_args("nadm_decode_bce", a.x)) return 1;
        if (a.kp > 16 || !a.qimg) return fail("nadm_decode_bce: the tiled copy feeds the matrix-core pass from the Q images only (padded K <= 16, qimg)");
    } else if (a.x.row_stride >> 32) return fail("nadm_decode_bce: rows of 4 GiB and more (ld >= 2^32) are not supported");      // the matrix pass forms row addresses from 32-bit factors
    if (slice_args(a.n_slices, (a.b + NADM_BF_TS - 1) / NADM_BF_TS, a.slab, a.counters, "nadm_decode_bce_sliced: n_slices must be in 1..8",
                   a.kp > 16 ? "nadm_decode_bce_sliced: sample slices exist for padded K <= 16 only" : nullptr,
                   "nadm_decode_bce_sliced: n_slices > 1 needs the slab (16-byte aligned) and the counters",
                   "nadm_decode_bce_sliced: a slice would be empty (take n_slices from nadm_decode_slices)")) return 1;
    if (a.qimg && (a.kp > 16 || NADM_BF_TS != QI_TS)) return fail("nadm_decode_bce_images: Q images exist for padded K <= 16 only");
    if ((uintptr_t)a.qimg & 15) return fail("nadm_decode_bce_images: qimg must be 16-byte aligned");
    if (a.with_loss < 0 || a.with_loss > 3) return fail("nadm_decode_bce: with_loss is a bit set (1: loss value, 2: P may lie outside [0,1])");
    a.loss = (a.with_loss & 1) != 0;
    a.unit_p = !(a.loss && (a.with_loss & 2));          // 3: the loss value with P possibly outside [0, 1] (before the first restrict_P)
    if (a.loss && !a.losspart) return fail("nadm_decode_bce: with_loss needs losspart");
    if (a.b <= 0 || a.M <= 0) return fail("nadm_decode_bce: empty batch or M");
    if (!a.x.clean && (a.x.row_stride % 16 != 0 || a.x.row_stride * 4 < a.M)) return fail("nadm_decode_bce: ld must be a multiple of 16 and >= ceil(M/4)");
    if (dispatch_kp("nadm_decode_bce", a.kp, [](auto) {})) return 1;
    a.sliced = a.n_slices > 1;
    return launch_pass2(a);
}

extern "C" int nadm_decode_bce(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                               const float* P, int32_t kp, const float* Q, int32_t SP, float* dP, float* dqpart,
                               float* losspart, int32_t with_loss, void* stream) {
    return pass2(Pass2Launch{x_rows(xp, ld), idx, b, M, const_cast<float*>(P), kp, Q, SP, dP, dqpart, losspart, with_loss, nullptr, nullptr, 1, nullptr, nullptr, false, stream});
}

extern "C" int nadm_decode_bce_gather(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                      const float* P, int32_t kp, const float* Q, int32_t SP, float* dP, float* dqpart,
                                      float* losspart, int32_t with_loss, uint8_t* xg, void* stream) {
    if (!xg) return fail("nadm_decode_bce_gather: null pointer");
    return pass2(Pass2Launch{x_rows(xp, ld), idx, b, M, const_cast<float*>(P), kp, Q, SP, dP, dqpart, losspart, with_loss, xg, nullptr, 1, nullptr, nullptr, false, stream});
}

extern "C" int nadm_decode_bce_step(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                    float* P, int32_t kp, const float* Q, int32_t SP, float* dP, float* dqpart,
                                    float* losspart, int32_t with_loss, uint8_t* xg, const nadm_adam_t* adam, void* stream) {
    Pass2Launch a{x_rows(xp, ld), idx, b, M, P, kp, Q, SP, dP, dqpart, losspart, with_loss, xg, nullptr, 1, nullptr, nullptr, false, stream};
    if (pass2_step_args(a, "nadm_decode_bce_step", adam, true)) return 1;
    return pass2(a);
}

extern "C" int nadm_decode_bce_images(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                      float* P, int32_t kp, const float* Q, int32_t SP, float* dP, float* dqpart,
                                      float* losspart, int32_t with_loss, uint8_t* xg, const nadm_adam_t* adam, const void* qimg,
                                      void* stream) {
    Pass2Launch a{x_rows(xp, ld), idx, b, M, P, kp, Q, SP, dP, dqpart, losspart, with_loss, xg, qimg, 1, nullptr, nullptr, false, stream};
    if (pass2_step_args(a, "nadm_decode_bce_images", adam, false)) return 1;
    if (!qimg) return fail("nadm_decode_bce_images: qimg is NULL (use nadm_decode_bce_step)");
    return pass2(a);
}

extern "C" int nadm_decode_bce_sliced(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                      float* P, int32_t kp, const float* Q, int32_t SP, float* dP, float* dqpart,
                                      float* losspart, int32_t with_loss, uint8_t* xg, const nadm_adam_t* adam, const void* qimg,
                                      int32_t n_slices, float* slab, int32_t* counters, void* stream) {
    Pass2Launch a{x_rows(xp, ld), idx, b, M, P, kp, Q, SP, dP, dqpart, losspart, with_loss, xg, qimg, n_slices, slab, counters, false, stream};
    if (pass2_step_args(a, "nadm_decode_bce_sliced", adam, false)) return 1;
    return pass2(a);
}

// =================================================================================================
// pass 3
// =================================================================================================
extern "C" int nadm_dz_image(const float* dZ, int32_t b, int32_t CP, void* dzimg, void* stream) {
    if (!dZ || !dzimg) return fail("nadm_dz_image: null pointer");
    if (b <= 0 || CP <= 0 || CP > 8) return fail("nadm_dz_image: b > 0 and 0 < CP <= 8 (the matrix-core pass 3)");
    if ((uintptr_t)dzimg & 15) return fail("nadm_dz_image: the image must be 16-byte aligned");
    return launch_dz_image(dZ, b, CP, dzimg, stream);
}

int nadm::pass3_step_args(Pass3Launch& a, const char* who, const nadm_adam_t* adam, bool sliced_form) {
    if (adam_fused_args(adam, who, &a.ad)) return 1;
    if (a.ad.m && (!a.V || ((uintptr_t)a.V & 15))) return failf(who, "V must be non-NULL and 16-byte aligned");
    if (sliced_form && a.CP > 8) return failf(who, "the matrix-core pass only (C <= 8)");
    const nadm_mlp_weights_t* w = a.weights;
    if (w && (!w->hd || !w->Zn || !w->H || !w->dL || !w->dHpre || !w->dgp || !w->small_part))
        return failf(who, "null pointer in the MLP weight-gradient arguments");
    return 0;
}

int nadm::pass3(Pass3Launch a) {
    if (!a.x.base || !a.idx || !a.dZ || !a.dV) return fail("nadm_encode_bwd: null pointer");
    const bool resident = a.x.clean;                    // the step's tiled copy of the whole matrix; NADM_X_CLEAN: pass 2's copy of the batch, handed over like a matrix
    if (resident && (a.flags & NADM_X_CLEAN)) return fail("nadm_encode_bwd: NADM_X_CLEAN names pass 2's batch copy, not the tiled copy of the matrix");
    if (a.CP > 8 && ((a.flags & NADM_X_CLEAN) || resident)) return fail("nadm_encode_bwd: the batch copy (NADM_X_CLEAN) is tiled for the matrix-core pass, C <= 8");
    if (a.CP <= 8 && (!a.dzimg || ((uintptr_t)a.dzimg & 15)))
        return fail("nadm_encode_bwd: C <= 8 runs on the FP4 x FP6 matrix instruction and needs the operand image of dZ (nadm_dz_image), 16-byte aligned");
    if (a.b <= 0 || a.M <= 0) return fail("nadm_encode_bwd: empty batch or M");
    if (resident) {
        if (tiled_source_args("nadm_encode_bwd", a.x)) return 1;
        if (a.missing_bf16 != 0u) return fail("nadm_encode_bwd: a missing call read as 1.5 needs the row-major matrix (the tiled copy holds no code 3)");
    } else if (a.x.row_stride % 16 != 0 || a.x.row_stride * 4 < a.M) return fail("nadm_encode_bwd: ld must be a multiple of 16 and >= ceil(M/4)");
    if (a.CP <= 8) {
        if (slice_args(a.n_slices, (a.b + DZI_TS - 1) / DZI_TS, a.slab, a.counters, "nadm_encode_bwd_sliced: n_slices must be in 1..8", nullptr,
                       "nadm_encode_bwd_sliced: the slab (16-byte aligned) and the counters are NULL",
                       "nadm_encode_bwd_sliced: an empty sample slice")) return 1;
        a.clean = resident || ((a.flags & NADM_X_CLEAN) != 0 && a.missing_bf16 == 0u);
        a.gather = resident;
        if (a.clean && !resident) a.x = x_tiled(a.x.base, a.b);
        a.sliced = a.n_slices > 1;
        return launch_pass3(a);
    }
    if (a.CP != 12 && a.CP != 16 && a.CP != 24 && a.CP != 32) return fail("nadm_encode_bwd: unsupported CP (4,8,12,16,24,32)");
    a.n_slices = 1;                                     // (the VALU kernel has no sliced form: the count is not looked at)
    return launch_pass3(a);
}

extern "C" int nadm_encode_bwd(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                               const float* dZ, const void* dzimg, int32_t CP, float* dV, int32_t flags, void* stream) {
    return pass3(Pass3Launch{x_rows(xp, ld), idx, b, M, dZ, dzimg, CP, nullptr, dV, nullptr, flags, 0u, 1, nullptr, nullptr, stream});
}

extern "C" int nadm_pca_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                  const float* Y, const void* yimg, int32_t CP, float* out, void* stream) {
    if (CP > 8) return fail("nadm_pca_project_t: only the matrix-core pass (CP <= 8) has the missing = 1.5 variant");
    return pass3(Pass3Launch{x_rows(xp, ld), idx, b, M, Y, yimg, CP, nullptr, out, nullptr, 0, 0x3FC0u, 1, nullptr, nullptr, stream});
}

extern "C" int nadm_encode_bwd_step(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                    const float* dZ, const void* dzimg, int32_t CP, float* V, float* dV, const nadm_adam_t* adam,
                                    const nadm_mlp_weights_t* weights, int32_t flags, void* stream) {
    Pass3Launch a{x_rows(xp, ld), idx, b, M, dZ, dzimg, CP, V, dV, weights, flags, 0u, 1, nullptr, nullptr, stream};
    if (pass3_step_args(a, "nadm_encode_bwd_step", adam, false)) return 1;
    return pass3(a);
}

extern "C" int nadm_encode_bwd_sliced(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                                      const float* dZ, const void* dzimg, int32_t CP, float* V, float* dV, const nadm_adam_t* adam,
                                      const nadm_mlp_weights_t* weights, int32_t flags, int32_t n_slices, float* slab, int32_t* counters, void* stream) {
    Pass3Launch a{x_rows(xp, ld), idx, b, M, dZ, dzimg, CP, V, dV, weights, flags, 0u, n_slices, slab, counters, stream};
    if (pass3_step_args(a, "nadm_encode_bwd_sliced", adam, true)) return 1;
    return pass3(a);
}

// =================================================================================================
// the MLP pair
// =================================================================================================
// which kernel: the fast ones cover Hd <= 2048 and C <= 8 (the test build can force the generic one)
static void mlp_form(const nadm_heads_t* hd, const float* small, MlpForm* form, int* jh, bool* c8) {
    *form = hd->Hd <= 256 * MLP_JMAX && hd->C <= 8 && !hook_generic_mlp() ? MLP_FAST : hd->Hd <= 2048 ? MLP_GENERIC4 : MLP_GENERIC1;
    *jh = hd->Hd <= 1024 ? 4 : 8;
    *c8 = hd->C == 8 && ((reinterpret_cast<uintptr_t>(small) + 4 * (size_t)hd->w1_off) & 15) == 0;
}

int nadm::mlp_fwd(MlpFwdLaunch a) {
    if (a.images) {
        if (!a.qimg) return fail("nadm_mlp_fwd_images: qimg is NULL (use nadm_mlp_fwd)");
        if (((uintptr_t)a.qimg & 15) || (a.qimg_head_bytes & 15)) return fail("nadm_mlp_fwd_images: qimg and the head stride must be multiples of 16 bytes");
        if (a.qimg_head_bytes < nadm_q_image_bytes(a.b)) return fail("nadm_mlp_fwd_images: head stride smaller than nadm_q_image_bytes(b)");
    }
    if (!a.hd || !a.small || !a.zpart || !a.Z || !a.rinv || !a.Zn || !a.H || !a.Q) return fail("nadm_mlp_fwd: null pointer");
    if (a.b <= 0) return fail("nadm_mlp_fwd: empty batch");
    mlp_form(a.hd, a.small, &a.form, &a.jh, &a.c8);
    return launch_mlp_fwd(a);
}

extern "C" int nadm_mlp_fwd(const nadm_heads_t* hd, const float* small, const float* zpart, int64_t n_chunks, int32_t b,
                            float* Z, float* rinv, float* Zn, float* H, float* Q, void* stream) {
    return mlp_fwd(MlpFwdLaunch{hd, small, zpart, n_chunks, b, Z, rinv, Zn, H, Q, false, nullptr, 0, stream});
}

extern "C" int nadm_mlp_fwd_images(const nadm_heads_t* hd, const float* small, const float* zpart, int64_t n_chunks, int32_t b,
                                   float* Z, float* rinv, float* Zn, float* H, float* Q, void* qimg, int64_t qimg_head_bytes, void* stream) {
    return mlp_fwd(MlpFwdLaunch{hd, small, zpart, n_chunks, b, Z, rinv, Zn, H, Q, true, qimg, qimg_head_bytes, stream});
}

int nadm::mlp_bwd(MlpBwdLaunch a) {
    if (a.image && (!a.dzimg || !a.dz_counters)) return fail("nadm_mlp_bwd_image: null pointer");
    if (!a.hd || !a.small || !a.dqpart || !a.Z || !a.rinv || !a.Zn || !a.H || !a.Q || !a.dL || !a.dHpre || !a.dgp || !a.small_part || !a.dZ)
        return fail("nadm_mlp_bwd: null pointer");
    if (a.dzimg && (!a.dz_counters || a.hd->CP > 8 || ((uintptr_t)a.dzimg & 15)))
        return fail("nadm_mlp_bwd_image: the image needs its group counters, C <= 8 and 16-byte alignment");
    if (a.n_loss > 0 && (!a.losspart || !a.loss_acc)) return fail("nadm_mlp_bwd: n_loss > 0 needs losspart and loss_acc");
    if (a.b <= 0) return fail("nadm_mlp_bwd: empty batch");
    mlp_form(a.hd, a.small, &a.form, &a.jh, &a.c8);
    return launch_mlp_bwd(a);
}

extern "C" int nadm_mlp_bwd(const nadm_heads_t* hd, const float* small, float* dqpart, int64_t M, int32_t b,
                            const float* Z, const float* rinv, const float* Zn, const float* H, const float* Q,
                            float* dL, float* dHpre, float* dgp, float* small_part, float* dZ, float* grad_small,
                            const float* losspart, int64_t n_loss, double* loss_acc, void* stream) {
    return mlp_bwd(MlpBwdLaunch{hd, small, dqpart, M, b, Z, rinv, Zn, H, Q, dL, dHpre, dgp, small_part, dZ, grad_small, losspart, n_loss, loss_acc,
                                false, nullptr, nullptr, stream});
}

extern "C" int nadm_mlp_bwd_image(const nadm_heads_t* hd, const float* small, float* dqpart, int64_t M, int32_t b,
                                  const float* Z, const float* rinv, const float* Zn, const float* H, const float* Q,
                                  float* dL, float* dHpre, float* dgp, float* small_part, float* dZ, float* grad_small,
                                  const float* losspart, int64_t n_loss, double* loss_acc, void* dzimg, int32_t* dz_counters, void* stream) {
    return mlp_bwd(MlpBwdLaunch{hd, small, dqpart, M, b, Z, rinv, Zn, H, Q, dL, dHpre, dgp, small_part, dZ, grad_small, losspart, n_loss, loss_acc,
                                true, dzimg, dz_counters, stream});
}
