/*
 * nadm.h -- C ABI of the MI355X-native Neural ADMIXTURE training engine (libnadm.so).
 *
 * This is the drop-in boundary for the reference's hot path.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repo).  Conventions:
 *   - plain pointers and sizes only; no torch / ATen types.
 *   - every device pointer is CALLER-OWNED (the reference's contract too: the caller allocates
 *     both tensors of pack2bit_cpu_to_gpu / unpack2bit_gpu_to_gpu, train.py:121,
 *     neural_admixture.py:377,405); the library never allocates or frees device memory.
 *   - every call is ASYNCHRONOUS on the hipStream_t passed as `stream` (void*; 0 = null stream)
 *     unless stated otherwise.  (The reference's extension blocks with cudaDeviceSynchronize on the
 *     legacy default stream, pack2bit.cu:115,141; callers that want that behaviour synchronise.)
 *     ALL device work of a call -- every launch, memset and copy of it -- is issued on `stream`, and the address of row r of
 *     a packed matrix, r * ld, is formed in 64 bits for any ld < 2^32 (tests/test_placement.py holds both).
 *   - return value: 0 = ok, nonzero = error; nadm_last_error() returns a thread-local message
 *     (the reference raises RuntimeError through TORCH_CHECK, pack2bit.cu:67-76,121-130; the
 *     Python host mirror turns nonzero statuses into RuntimeError).
 *   - one host thread per process/GPU, not re-entrant per stream (same as the reference).
 *
 * Device data layout (all float32 unless noted):
 *   xp     uint8 [rows, ld]   2-bit packed genotypes, sample-major, SNP 4c+i in bits [2i,2i+1] of
 *                             byte c (pack2bit.cu:26-31); ld >= ceil(M/4), ld % 16 == 0, ld < 2^32 (the matrix-pipe passes form row addresses from
 *                             32-bit factors and refuse longer rows), pad bytes 0.
 *   V      [M, CP]            encoder projection, CP = C rounded up to a multiple of 4, pad cols 0
 *                             (reference: Q_P.V [M,C], neural_admixture.py:129-130).
 *   P_h    [M, KP_h]          decoder head h, SNP-major, KP_h = padded K (nadm_pad_k), pad cols 0
 *                             (reference: decoders[h].weight, logical [M,k], neural_admixture.py:73-74).
 *   small  flat               g[C] | W1[Hd,C] | b1[Hd] | for h: Wk_h[k_h,Hd] | bk_h[k_h]
 *                             (batch_norm.weight, common_encoder.0.{weight,bias},
 *                              multihead_encoder.heads.h.{weight,bias}).
 *   Q      [b, SP]            per-head softmax outputs; head h occupies columns
 *                             [qoff_h, qoff_h + k_h), SP = sum KP_h; pad cols 0.
 */
#ifndef NADM_H
#define NADM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NADM_MAX_HEADS 32
#define NADM_MAX_K 64
#define NADM_MAX_BUCKETS 8
#define NADM_MAX_P2_SLICES 8   /* sample slices of pass 2 (nadm_decode_bce_sliced) */
#define NADM_ABI_VERSION 14  /* 14: nadm_clock_probe; new symbols only, same version: nadm_plan_set_precision / nadm_plan_precision (NADM_PRECISION_*), nadm_class_sums + NADM_LABEL_NONE (labels in [-1, k)), nadm_project_q / nadm_project_scratch_floats (projection: Q refined against a fixed P), nadm_snp_counts / nadm_ld_band / nadm_select_snps / nadm_ld_sweep (LD pruning), nadm_ibd / nadm_ibd_ranges / nadm_ibd_scratch_floats + NADM_IBD_MAX_ROWS (IBD-sharing sums given ancestry); 13: pass 3 in sample slices (nadm_encode_bwd_sliced, nadm_encode_slices(_max), nadm_encode_slab_floats, nadm_encode_bwd_chunks, nadm_plan_desc_t.p3_slab / p3_cnt); 12: nadm_test_force_slices / nadm_test_force_generic_mlp exist in the test build only (-DNADM_TEST_HOOKS), nadm_calib_clock / nadm_wall_clock_khz; 11: nadm_gmm_fit_means_dev, nadm_loglik_blocks counts 8 row slices per 1024-SNP block, nadm_decode_bce_sliced / nadm_decode_slices / nadm_decode_slab_floats / nadm_test_force_slices + nadm_plan_desc_t.p2_slab / p2_cnt (pass 2 in sample slices when the SNP chunks alone do not fill the chip); 10: message B of the sample-sharded step in SNP-range buckets (nadm_flat_layout takes n_buckets, nadm_flat_layout_t.bkt_*, nadm_plan_desc_t.n_buckets / p3_whole / comm_a / debug, nadm_encode_fwd_part, nadm_plan_bucket_ms), nadm_comm_t.async_error, nadm_comm_rccl_probe, nadm_comm_rccl with a watchdog (timeout_ms), a failed step poisons its plan; 9: nadm_step / nadm_plan_* / nadm_comm_* / nadm_flat_layout (the step as one call, sharded optimizer), nadm_test_force_generic_mlp; 8: nadm_dz_image(_bytes), nadm_mlp_bwd_image; nadm_encode_bwd, nadm_encode_bwd_step, nadm_pca_project_t take the operand image of dZ / Y; 7: nadm_encode_fwd_step, nadm_sum_rows, dqpart of nadm_mlp_bwd is float* (folded in place); 6: nadm_mlp_fwd_images, nadm_decode_bce_images, nadm_q_image_bytes, nadm_encode_fwd_small; 5: nadm_adam_t.when, nadm_adam2, with_loss bit 1; 4: nadm_decode_bce_step, nadm_encode_bwd_step (nadm_adam_t, nadm_mlp_weights_t), nadm_small_grads; 3: nadm_decode_bce_gather; 2: nadm_mlp_bwd_weights, nadm_supervised_ce, nadm_pca_project(_t), nadm_loglik, nadm_savetxt_f32, nadm_decode_chunk_snps; grad_small of nadm_mlp_bwd may be NULL */

/* Head table shared by the MLP entry points (mirror of NeuralEncoder/NeuralDecoder's ks list,
 * neural_admixture.py:27-29,66-76). Offsets are element offsets into the `small` flat buffer. */
typedef struct nadm_heads {
    int32_t n_heads;
    int32_t C;              /* n_components (true) */
    int32_t CP;             /* padded */
    int32_t Hd;             /* hidden size */
    int32_t SP;             /* sum of padded K = row length of Q / dQ */
    int32_t n_small;        /* number of floats in the small flat buffer */
    int32_t k[NADM_MAX_HEADS];
    int32_t kp[NADM_MAX_HEADS];
    int32_t qoff[NADM_MAX_HEADS];
    int32_t wk_off[NADM_MAX_HEADS];
    int32_t bk_off[NADM_MAX_HEADS];
    int32_t g_off, w1_off, b1_off;
} nadm_heads_t;

/* ---- introspection ------------------------------------------------------------------- */
int         nadm_abi_version(void);
const char* nadm_last_error(void);
/* Padded widths used by the kernels: multiple of 4 up to 16, then {24,32,48,64}. <=0 if unsupported. */
int         nadm_pad_k(int k);
/* Fill a head table from (C, Hd, ks[n]) -- the layout every other call assumes. */
int         nadm_heads_init(nadm_heads_t* out, int C, int Hd, const int32_t* ks, int n);
/* Number of SNP chunks (= rows of partial buffers) the three genotype passes use for M SNPs. */
int64_t     nadm_encode_chunks(int64_t M);      /* zpart  is [chunks, b, CP]  */
int64_t     nadm_decode_chunks(int64_t M, int kp); /* per head: dqpart slab [chunks, b, kp], losspart [chunks] */
/* SNPs per chunk of the decoder pass.  nadm_decode_bce / nadm_encode_bwd may be launched on an SNP sub-range
 * [m0, m1) with m0 a multiple of lcm(this, 1024): pass xp + m0/4, P/dP (V/dV) + m0*kp, M = m1 - m0 and the slab /
 * loss pointers advanced by m0/chunk_snps rows (a caller that wants a piece of a gradient early). */
int32_t     nadm_decode_chunk_snps(int kp);
int32_t     nadm_sample_splits(int b);          /* small_part is [splits, n_small] */

/* ---- a1/a2: packing  (replaces pack2bit.cu:10-36,65-117 and :38-62,120-142) ------------ */
/* Host-side pack: g_host uint8 [N,M] (row stride M) -> out_host [N,ld].  Synchronous, OpenMP. */
int nadm_pack2bit_host(const uint8_t* g_host, uint8_t* out_host, int64_t N, int64_t M, int64_t ld);
/* Device pack kernel: g_dev uint8 [rows,M] unpacked on device -> out_dev [rows,ld] (pad bytes zeroed). */
int nadm_pack2bit(const uint8_t* g_dev, uint8_t* out_dev, int64_t rows, int64_t M, int64_t ld, void* stream);
/* Device unpack (test / interop only; the training kernels decode in registers):
 * in_dev [rows,ld] -> out_dev uint8 [rows,M]. */
int nadm_unpack2bit(const uint8_t* in_dev, uint8_t* out_dev, int64_t rows, int64_t M, int64_t ld, void* stream);

/* ---- 8(f)-1: PLINK .bed -> packed sample-major, no uint8 [N,M] detour -------------------------
 * (replaces SNPReader._read_bed + utils_c.read_bed + pack2bit for BED input: src/snp_reader.py:16-45,
 * src/utils_c/utils.pyx:43-67, pack2bit.cu:65-117).  bed = the file contents AFTER the 3 magic bytes,
 * SNP-major [M, ceil(N/4)], 4 samples per byte, PLINK codes mapped with the reference's table [2,3,1,0]
 * (0b01 = missing -> 3).  out_host [N, ld] gets the layout every kernel here consumes.  counts[4] receives
 * the number of genotypes with code 0..3 (before any flip).  If flip_if_mean_ge1 != 0 and the mean code
 * (3s included, like the reference's G.mean(), snp_reader.py:110) is >= 1, alleles are flipped 0<->2 and
 * *flipped is set to 1; missing stays 3 (the reference's uint8 `2 - G` turns 3 into 255, which its own GPU
 * path masks back to 3, pack2bit.cu:29).  Synchronous, multi-threaded. */
int nadm_bed_to_packed(const uint8_t* bed, int64_t N, int64_t M, uint8_t* out_host, int64_t ld,
                       int64_t* counts, int32_t flip_if_mean_ge1, int32_t* flipped);

/* The same conversion on the device: bed_dev = the file contents after the 3 magic bytes, already in HBM ([M, ceil(N/4)]);
 * out_dev [N, ld] (ld % 16 == 0; the row padding is written as zeros); counts_dev uint64[4] and flipped_dev int32[1] are
 * device scratch/outputs (zeroed here).  The flip decision is taken on the device, nothing is read back: asynchronous. */
int nadm_bed_to_packed_dev(const uint8_t* bed_dev, int64_t N, int64_t M, uint8_t* out_dev, int64_t ld, uint64_t* counts_dev,
                           int32_t flip_if_mean_ge1, int32_t* flipped_dev, void* stream);

/* ---- a4/a5: encoder projection  Z = X.V  (neural_admixture.py:169-172) ----------------- */
/* rows idx[0..b) of xp are the batch (replaces Dataset_admixture.__getitem__ + collate,
 * loaders.py:62-72, and the per-step unpack2bit_gpu_to_gpu, neural_admixture.py:404-406).
 * Writes per-chunk partial sums zpart [nadm_encode_chunks(M), b, CP]; nadm_mlp_fwd reduces them. */
int nadm_encode_fwd(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                    const float* V, int32_t CP, float* zpart, void* stream);

/* nadm_encode_fwd on an SNP sub-range that is ONE PART of a pass launched in several (the sample-sharded step: one part per
 * bucket of message B, each part waiting for its own bucket, include "The training step as ONE call" below): pointers already
 * advanced to the range -- xp + m0/4, V + m0*CP, zpart + (m0/2048)*b*CP, M = m1 - m0, m0 a multiple of 2048 -- and total_chunks =
 * nadm_encode_chunks of the WHOLE pass, which the batch split is chosen for (the parts share the device; a part sized on its own
 * would cut the batch finer and pay the per-block operand build that often).  Same results as the one launch, bit for bit. */
int nadm_encode_fwd_part(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                         const float* V, int32_t CP, float* zpart, int64_t total_chunks, void* stream);

/* ---- 8(f)-3: init-time PCA projection  X_pca = (G/2).V  with a MISSING call counted as 1.5 --------------
 * (train.py:49-55: `batch.astype(np.float32)/2 @ V.T` on the raw codes, no masking; feeds the sklearn GMM.  Also the
 * first tall-skinny product of the randomized SVD, src/svd.py:52,62 -> utils_c/rsvd.pyx multiply_A_omega.)
 * Same kernel, buffers and partial-sum layout as nadm_encode_fwd; CP <= 8 only. */
int nadm_pca_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                     const float* V, int32_t CP, float* zpart, void* stream);
/* Transposed product with the same convention,  out [M,CP] = (G/2)^T . Y  for the rows idx[0..b), Y [b,CP]: the second
 * tall-skinny product of the randomized SVD (src/svd.py:60,77 -> utils_c/rsvd.pyx multiply_QT_A; A = raw codes = 2 * G/2).
 * Same kernel as nadm_encode_bwd; CP <= 8 only; yimg = nadm_dz_image of Y. */
int nadm_pca_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                       const float* Y, const void* yimg, int32_t CP, float* out, void* stream);

/* ---- a6-a8: RMSNorm + Linear/ReLU + per-head Linear + softmax (neural_admixture.py:173-176) */
int nadm_mlp_fwd(const nadm_heads_t* hd, const float* small, const float* zpart, int64_t n_chunks, int32_t b,
                 float* Z, float* rinv, float* Zn, float* H, float* Q, void* stream);
/* The same, and Q additionally as the bf16 MFMA operand images pass 2 builds from it (heads with padded K <= 16): every block
 * of nadm_decode_bce* otherwise splits the batch's Q into bf16 pieces itself, tile by tile (1954 blocks at M = 500k doing the
 * same 800 x K conversion).  qimg: n_heads regions of qimg_head_bytes >= nadm_q_image_bytes(b) bytes, 16-byte aligned and
 * ZERO-FILLED ONCE by the caller (slots that hold no piece are never written); head h's images start at h * qimg_head_bytes.
 * Hand a head's region to nadm_decode_bce_images together with the same Q. */
int64_t nadm_q_image_bytes(int32_t b);
int nadm_mlp_fwd_images(const nadm_heads_t* hd, const float* small, const float* zpart, int64_t n_chunks, int32_t b,
                        float* Z, float* rinv, float* Zn, float* H, float* Q, void* qimg, int64_t qimg_head_bytes, void* stream);

/* ---- a9-a11: decoder Q.P^T -> clamp -> BCE(sum) forward + backward, one head -------------
 * (neural_admixture.py:94-97, :288/:431, autograd of both).  P,dP [M,kp]; Q = Qbase + qoff
 * with row stride SP; dqpart = this head's slab [nadm_decode_chunks(M,kp), b, kp]; losspart
 * [chunks] (written only if with_loss != 0).  Missing genotypes are x = 0 in input and target.
 * with_loss is a bit set: 1 = compute the loss value; 2 = P may hold values outside [0, 1] (before the first restrict_P: the
 * reference's supervised run starts from per-class means of the raw codes, train.py:82) -- the matrix-core kernels then
 * clamp the reconstruction before the logarithm, which they otherwise skip because clamp(r) == r up to rounding. */
int nadm_decode_bce(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                    const float* P, int32_t kp, const float* Q, int32_t SP,
                    float* dP, float* dqpart, float* losspart, int32_t with_loss, void* stream);

/* The same pass with a by-product for pass 3: the batch as a copy of its own in xg -- rows in batch order, every missing call
 * (code 3) already replaced by 0 (the model's input, neural_admixture.py:170), TILED by pass 3's chunks: byte column c of batch
 * row i at  (c / 128) * b * 128 + i * 128 + c % 128  (nadm_batch_copy_bytes(b, M) bytes; an SNP sub-range launch starting at
 * SNP m0 passes xg + (m0 / 4) * b).  Pass 3 (nadm_encode_bwd) is then given xg instead of xp with flags = NADM_X_CLEAN (idx is
 * not read): each of its blocks streams one contiguous b x 128 byte region instead of gathering 128-byte row pieces 125 KB
 * apart out of the resident matrix (those arrive at 2.6 TB/s, and at 12.5 GB resident 13 % of them miss the translation
 * cache).  No reference counterpart: the reference re-gathers the unpacked batch per pass (utils.pyx:43-67). */
int nadm_decode_bce_gather(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                           const float* P, int32_t kp, const float* Q, int32_t SP,
                           float* dP, float* dqpart, float* losspart, int32_t with_loss, uint8_t* xg, void* stream);

/* ---- single-GPU step: Adam applied where the gradient is completed -----------------------------------------------------
 * In a step on one GPU the gradient of a P row is final when the pass-2 block that owns it finishes, and nothing else in
 * the step reads that row again; likewise for V rows and pass 3.  The *_step entry points take the Adam state of those
 * rows and apply optimizer.step() + restrict_P (neural_admixture.py:187-204,411-412) to them in the kernel's epilogue --
 * the same element update as nadm_adam, bit for bit -- instead of writing the gradient out for a separate launch (which
 * the sample-sharded step still does: its gradients have to be summed over ranks first, nadm_step).  adam == NULL: exactly
 * nadm_decode_bce(_gather) / nadm_encode_bwd.  With adam, m and v point at the Adam moments of the SAME rows as P / V
 * (sub-range launches advance them like P / V), the gradient buffer is left untouched by the matrix-core kernels
 * (K <= 16, C <= 8; the other variants write it and run the update as a second kernel), xg may be NULL. */
typedef struct {
    float*  m;            /* first moment of the rows being updated  */
    float*  v;            /* second moment                            */
    float   lr;
    int32_t step;         /* 1-based step count                       */
    float   grad_scale;   /* gradients are multiplied by this first   */
    int32_t reserved;     /* 0 */
} nadm_adam_t;
int nadm_decode_bce_step(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                         float* P, int32_t kp, const float* Q, int32_t SP,
                         float* dP, float* dqpart, float* losspart, int32_t with_loss,
                         uint8_t* xg, const nadm_adam_t* adam, void* stream);
/* nadm_decode_bce_step (xg and adam may be NULL: then nadm_decode_bce / _gather) with this head's Q operand images from
 * nadm_mlp_fwd_images (kp <= 16): the same bf16 pieces, the same results bit for bit. */
int nadm_decode_bce_images(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                           float* P, int32_t kp, const float* Q, int32_t SP,
                           float* dP, float* dqpart, float* losspart, int32_t with_loss,
                           uint8_t* xg, const nadm_adam_t* adam, const void* qimg, void* stream);
/* The same kernel (qimg may be NULL) with the batch's 64-sample tiles dealt to n_slices blocks per 256-SNP chunk: below ~130k SNPs a
 * launch lasts as long as ONE block's serial chain (prologue + 13 tiles at b = 800: 49 us whether 98 or 196 blocks run), not as long as
 * the chip needs, and pass 2 runs at a third to a half of its rate (profiles/r05_ablations.txt item 11).  dQ rows, the batch copy and everything else per sample are written by the slice that owns the sample; every
 * slice parks its partial of dP (and of the loss value) in `slab`, and the block that is counted last in `counters` adds the
 * partials in slice order and runs the epilogue -- no block waits for another, the result is reproducible bit for bit, and it differs
 * from the n_slices = 1 result by the rounding of that sum only.  n_slices: take nadm_decode_slices(b, M, kp) (1 for kp > 16 and
 * wherever the chunks suffice) -- the plan (nadm_step) and every caller that wants its bits use that function; slab: at least
 * nadm_decode_slab_floats(M, kp, n_slices) floats, 16-byte aligned; counters: one int32 per chunk (nadm_decode_chunks), ZERO-FILLED
 * ONCE by the caller (a launch returns them to zero).  Concurrent launches (heads on two streams) need regions of their own. */
int32_t nadm_decode_slices(int32_t b, int64_t M, int32_t kp);
int32_t nadm_decode_slices_max(int32_t bmax, int64_t M, int32_t kp);   /* the largest value over batches of 1..bmax rows: what sizes a slab */
int64_t nadm_decode_slab_floats(int64_t M, int32_t kp, int32_t n_slices);
int nadm_decode_bce_sliced(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                           float* P, int32_t kp, const float* Q, int32_t SP,
                           float* dP, float* dqpart, float* losspart, int32_t with_loss,
                           uint8_t* xg, const nadm_adam_t* adam, const void* qimg,
                           int32_t n_slices, float* slab, int32_t* counters, void* stream);
#ifdef NADM_TEST_HOOKS   /* the TEST build only (csrc/build.sh -> libnadm_testhooks.so); the shipping library does not export it */
/* n > 0 makes nadm_decode_slices return n (capped by the number of tiles) for every kp <= 16 shape, 0 = the library's choice.
 * Process-wide; set it before the buffers of a plan are sized (a plan refuses a step that would need more slices than its slab holds). */
void nadm_test_force_slices(int32_t n);
#endif
/* `weights` (may be NULL): the MLP weight-gradient partials -- the first half of nadm_mlp_bwd_weights, which like pass 3
 * depends only on the outputs of nadm_mlp_bwd(grad_small = NULL) -- are computed by extra blocks of the same launch (they
 * fill the under-occupied last round of pass 3) into small_part [nadm_sample_splits(b), n_small]; nadm_small_grads then
 * sums them into grad_small and, with Adam state, updates the small parameters in the same launch. */
typedef struct {
    const nadm_heads_t* hd;
    const float *Zn, *H, *dL, *dHpre, *dgp;   /* as for nadm_mlp_bwd_weights */
    float* small_part;
} nadm_mlp_weights_t;
int nadm_encode_bwd_step(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                         const float* dZ, const void* dzimg, int32_t CP, float* V, float* dV, const nadm_adam_t* adam,
                         const nadm_mlp_weights_t* weights, int32_t flags /* NADM_X_CLEAN, see nadm_encode_bwd */, void* stream);
/* Pass 3 with the batch's 128-sample tiles dealt to n_slices blocks per 512-SNP chunk (r06; C <= 8): for launches whose chunks alone leave
 * most CUs idle -- an SNP-sharded rank's 6400 rows x 62.5k SNPs is 122 blocks.  Every slice parks its partial [512 x CP] sum in `slab`
 * (nadm_encode_slab_floats(M, CP, n_slices) floats, 16-byte aligned), the block counted last (`counters`: nadm_encode_bwd_chunks(M) int32,
 * zero-filled once, left zero) adds them in slice order and applies the update / stores the gradient: pass 2's hand-off, reproducible
 * bit for bit.  n_slices comes from nadm_encode_slices(b, M, CP) -- a function of the shape alone, 1 for every single-GPU BASELINE shape --
 * so that every path to the pass cuts the batch the same way; adam / weights as for nadm_encode_bwd_step (both may be NULL). */
int32_t nadm_encode_slices(int32_t b, int64_t M, int32_t CP);
int32_t nadm_encode_slices_max(int32_t bmax, int64_t M, int32_t CP);
int64_t nadm_encode_slab_floats(int64_t M, int32_t CP, int32_t n_slices);
int64_t nadm_encode_bwd_chunks(int64_t M);
int nadm_encode_bwd_sliced(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                           const float* dZ, const void* dzimg, int32_t CP, float* V, float* dV, const nadm_adam_t* adam,
                           const nadm_mlp_weights_t* weights, int32_t flags, int32_t n_slices, float* slab, int32_t* counters, void* stream);
#ifdef NADM_TEST_HOOKS   /* the TEST build only: n > 0 makes nadm_encode_slices return n (capped by the tiles), 0 = the library's choice */
void nadm_test_force_p3_slices(int32_t n);
#endif
int nadm_small_grads(const float* small_part, int32_t splits, int32_t n_small, float* grad_small, float* small,
                     const nadm_adam_t* adam, void* stream);
/* nadm_encode_fwd of the NEXT step with nadm_small_grads of this one riding in the same launch as side blocks (pass 1 reads
 * none of the small parameters; the MLP forward behind it reads the updated ones): same sums, same update, one launch and a
 * launch gap less per step.  The caller owes the update to anything that reads `small` before that next pass 1. CP <= 8. */
int nadm_encode_fwd_small(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                          const float* V, int32_t CP, float* zpart, const float* small_part, int32_t splits, int32_t n_small,
                          float* grad_small, float* small, const nadm_adam_t* adam, void* stream);

/* ---- a11: MLP backward (softmax, Linear, ReLU, RMSNorm) ---------------------------------- */
/* Reduces dqpart (the heads' slabs laid back to back in head order, head h holding
 * nadm_decode_chunks(M,kp_h)*b*kp_h floats), writes dZ [b,CP], the flat small-parameter gradient
 * grad_small [n_small] (NULL: left to nadm_mlp_bwd_weights), and when n_loss>0 adds the step's loss (sum of losspart[0..n_loss)) to
 * loss_acc[0] (running sum) and stores it in loss_acc[1] (last step); loss_acc is double[2].
 * Scratch: dL [b,SP], dHpre [b,Hd], dgp [b,CP], small_part [nadm_sample_splits(b), n_small].  dqpart is IN/OUT scratch of the
 * step (hence not const): a slab of more than 2560 rows is folded to 64 rows IN PLACE first (its first 64 rows then hold
 * partial sums, the others are unchanged); shorter slabs are left untouched.  Do not read dqpart after this call. */
int nadm_mlp_bwd(const nadm_heads_t* hd, const float* small, float* dqpart, int64_t M, int32_t b,
                 const float* Z, const float* rinv, const float* Zn, const float* H, const float* Q,
                 float* dL, float* dHpre, float* dgp, float* small_part,
                 float* dZ, float* grad_small,
                 const float* losspart, int64_t n_loss, double* loss_acc, void* stream);

/* out[e] = sum over r < rows of src[r * n + e]  (fixed order; n a multiple of 4, 16-byte aligned pointers): the fold of a
 * partial slab -- zpart [chunks, b*CP] of nadm_encode_fwd, a head's dqpart [chunks, b*kp] -- to one row.  The SNP-sharded step
 * (8(f)-4) folds its rank-local partial sums with it before the two small all-reduces of a step. */
int nadm_sum_rows(const float* src, int64_t rows, int64_t n, float* out, void* stream);

/* ---- 8(f): supervised mode,  weight * CrossEntropyLoss(sum)(Q_0, labels)  (neural_admixture.py:293,470-473;
 * the reference feeds the softmax OUTPUT of head 0 to CrossEntropyLoss, i.e. a second softmax; default weight 100).
 * labels int32 [rows] = class per resident row (train.py:78-81 mapping), idx = the batch's rows (NULL: labels is
 * already per batch row); n_classes must equal k (train.py:79 asserts it).  Call after head 0's nadm_decode_bce and
 * before nadm_mlp_bwd: ADDS weight*(softmax(q_i) - onehot(y_i)) to chunk 0 of head 0's dQ slab (dqpart0 [.., b, kp])
 * and writes the weighted loss to *loss_slot (one float that nadm_mlp_bwd's n_loss range should cover).
 * Labels lie in [-1, k): NADM_LABEL_NONE marks a sample without a label (semi-supervised run: a labelled panel plus query
 * samples).  Such a row is skipped -- its dQ is not touched and it adds nothing to the loss, which is what
 * CrossEntropyLoss(reduction='sum') does with an ignored target; the sum is NOT renormalised by the number of labelled rows.
 * A batch with no labelled row writes 0 to *loss_slot.  A label outside [-1, k) is the caller's error (not checked on the device). */
#define NADM_LABEL_NONE (-1)
int nadm_supervised_ce(const float* Q, int32_t SP, int32_t k, int32_t kp, const int32_t* labels, const int32_t* idx,
                       int32_t b, int32_t n_classes, float weight, float* dqpart0, float* loss_slot, void* stream);

/* Per-class genotype sums from the packed matrix: the numerator of the supervised P init (per-class mean of the RAW codes,
 * train.py:82) in one pass over X.  sums uint32 [n_classes, M] (device, row stride M):
 *     sums[c][m] += sum over j in [class_start[c], class_start[c+1]) of code(xp[idx[j]], m),     code = 0, 1, 2 and 3 for missing.
 * idx int32 (device) lists the rows of xp [rows, ld] GROUPED BY CLASS (a stable argsort of the labels with the unlabelled rows
 * dropped; entries outside [0, rows) are ignored); class_start int64 [n_classes + 1] is HOST memory, read before the call
 * returns, non-decreasing, listing at most `rows` rows in all.  idx may be NULL when no row is listed (nothing is launched).
 * The call ADDS: the caller zero-fills sums once, and a matrix streamed in row chunks accumulates over calls.  Integer
 * arithmetic throughout (atomic adds where row slices share an output word), so the result is exact and independent of the order.
 * Overflow: an entry holds at most 3 * (rows of its class, all calls together), which must fit in 32 bits -- a call refuses
 * rows > (2^32 - 1) / 3 = 1431655765; over several calls the bound on the total is the caller's.
 * 1 <= n_classes <= NADM_MAX_K; ld a multiple of 4 and >= ceil(M/4), xp 4-byte aligned; only SNPs < M are written and the
 * bytes of a row past its last 32-bit word with a SNP in it are not read.  Asynchronous on `stream`. */
int nadm_class_sums(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, const int32_t* idx, const int64_t* class_start,
                    int32_t n_classes, uint32_t* sums, void* stream);

/* The weight-gradient half of nadm_mlp_bwd on its own (dWk, dbk, dW1, db1, dg from dL, dHpre, dgp, H, Zn -> grad_small):
 * pass grad_small = NULL to nadm_mlp_bwd and call this on any stream ordered after it -- it is independent of pass 3,
 * so a second stream can run it (and the small Adam) underneath nadm_encode_bwd. */
int nadm_mlp_bwd_weights(const nadm_heads_t* hd, int32_t b, const float* Zn, const float* H, const float* dL,
                         const float* dHpre, const float* dgp, float* small_part, float* grad_small, void* stream);

/* ---- a11: dV = X^T . dZ  (autograd of neural_admixture.py:172) ---------------------------
 * C <= 8 (CP 4, 8) runs on gfx950's FP4 x FP6 block-scaled matrix instruction: the 2-bit codes enter it as FP4 numbers without a
 * conversion, and dZ enters as an OPERAND IMAGE -- per 32 samples x column eight FP6 pieces (the hexadecimal digits of |dZ| in
 * fixed point below the block's maximum) with their E8M0 scales, laid out per lane of the instruction.  The image is the same
 * for every block of the launch, so it is built once: nadm_dz_image(dZ [b, CP] -> dzimg, nadm_dz_image_bytes(b) bytes, 16-byte
 * aligned), on the stream, before the pass.  dZ itself is read by the CP > 8 variants only (dzimg may be NULL for them). */
int64_t nadm_dz_image_bytes(int32_t b);
int64_t nadm_dz_image_tile_bytes(void);      /* bytes of one 128-sample tile of the image */
int nadm_dz_image(const float* dZ, int32_t b, int32_t CP, void* dzimg, void* stream);
/* nadm_mlp_bwd that also leaves dZ's operand image in dzimg: the block that completes a group of 32 samples last builds the group's
 * part (no launch of its own, no launch gap).  dz_counters: (b + 31) / 32 int32 on the device, ZERO-FILLED ONCE by the caller (the
 * launch returns them to zero).  Only the 32-sample groups the batch touches are written: a caller whose batch is shorter than the
 * one before clears the image's last tile first (nadm_dz_image_tile_bytes; nadm_step does), or the groups between the batch and
 * the end of that tile keep the earlier batch's pieces -- harmless while they are finite (pass 3 multiplies them by X = 0), but
 * a group that held an inf carries the NaN scale. */
int nadm_mlp_bwd_image(const nadm_heads_t* hd, const float* small, float* dqpart, int64_t M, int32_t b,
                       const float* Z, const float* rinv, const float* Zn, const float* H, const float* Q,
                       float* dL, float* dHpre, float* dgp, float* small_part, float* dZ, float* grad_small,
                       const float* losspart, int64_t n_loss, double* loss_acc, void* dzimg, int32_t* dz_counters, void* stream);
#define NADM_X_CLEAN 1     /* flags: xp is nadm_decode_bce_gather's copy of the batch (tiled, rows in batch order, missing calls already 0) */
int64_t nadm_batch_copy_bytes(int32_t b, int64_t M);
/* The WHOLE matrix as a tiled, cleaned copy, made once when the matrix is handed over (the rows never change during training): the
 * layout of the batch copy with b := rows -- byte column c of row r at  (c / 128) * rows * 128 + r * 128 + c % 128  -- every missing
 * call (code 3) 0, every code of an SNP >= M 0, the last tile 128 bytes wide: nadm_tiled_bytes(rows, M) = ceil(M / 512) * rows * 128
 * bytes (0 for an empty shape).  A plan that is given the copy (nadm_plan_set_tiles) gathers the batch's rows for its matrix-core
 * passes out of it: a block's pieces then lie inside one rows x 128 B window instead of one row length apart, and nothing is cleaned
 * or masked per batch.  Results are bit-identical to the row-major source.  xp [rows, ld] as everywhere (ld % 16 == 0, ld >= ceil(M/4),
 * ld < 2^32), rows < 2^31, xp and xt 16-byte aligned and not overlapping.  Refusals in this order: null pointer, empty matrix, ld,
 * rows, alignment, overlap. */
int64_t nadm_tiled_bytes(int64_t rows, int64_t M);
int nadm_tile_packed(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, uint8_t* xt, void* stream);
int nadm_encode_bwd(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                    const float* dZ, const void* dzimg, int32_t CP, float* dV, int32_t flags, void* stream);

/* ---- a12/a13: Adam(betas .9/.95, eps 1e-8) + restrict_P (neural_admixture.py:187-204,411-412)
 * Flat update of n floats; `step` is the 1-based step count; gradients are multiplied by
 * grad_scale first (1/world for the DDP mean, neural_admixture.py:317); elements with index
 * >= clamp_from are clamped to [0,1] after the update (pass n for "no clamp"). */
int nadm_adam(float* param, const float* grad, float* m, float* v, int64_t n, int64_t clamp_from,
              float lr, int32_t step, float grad_scale, void* stream);

/* ======================================================================================================================
 * The training step as ONE call  (replaces NeuralAdmixture._run_step + the DDP hooks + optimizer.step + restrict_P,
 * neural_admixture.py:315-319,403-414, as one host call per step; the entry points above remain the pieces it is made of)
 * ======================================================================================================================
 * Flat parameter layout.  Parameters, gradients and (single / SNP-sharded mode) Adam moments live in ONE flat float buffer each:
 *     [ small | pad | V [M,CP] | gap | P_0 [M,KP_0] | P_1 ... | gap ]
 * cut into the two MESSAGES of the sample-sharded step: B = [0, msg_a_off) holds the small parameters and V, A =
 * [msg_a_off, msg_a_off + world * slice_a) holds every head's P; the gaps (zeros, < 4 * world floats) make both a multiple of
 * `world` slices.  world = 1: no gaps, pad = to a multiple of 64 floats.
 * Message B travels as n_buckets BUCKETS (r05; DDP's bucketed exchange, neural_admixture.py:315-319): bucket j = the floats
 * [bkt_off[j], bkt_off[j+1]) = the V rows of the SNP range [bkt_m0[j], bkt_m0[j+1]) -- bucket 0 also the small parameters in front of
 * them -- as `world` contiguous slices of bkt_slice[j] floats (range-major: every bucket is a message of its own, reduce-scattered,
 * updated and all-gathered while the other ranges are still being computed or already consumed).  Range boundaries are multiples of
 * every kernel's chunk (2048 SNPs) AND of what makes a bucket 4 * world floats long; a request for more buckets than M allows yields
 * fewer (n_buckets is the number actually cut; 1 = the single message of r04).  slice_b = sum of bkt_slice = floats of B per rank;
 * the rank's moments of bucket j start at bkt_mom[j] in its moment buffers (DP mode: [slice_b | slice_a] floats each). */
typedef struct nadm_flat_layout {
    int64_t n_flat;                       /* floats in a flat buffer                                  */
    int64_t off_v;                        /* V starts here (n_small rounded up to lcm(64, 4 * world)) */
    int64_t off_p[NADM_MAX_HEADS];        /* head h's P starts here                                   */
    int64_t slice_b, slice_a;             /* floats per rank of message B (all buckets) / A           */
    int64_t msg_a_off;                    /* where message A starts = end of the last bucket of B     */
    int32_t n_buckets, reserved;          /* buckets message B is cut into (>= 1)                     */
    int64_t bkt_off[NADM_MAX_BUCKETS + 1];/* bucket j = floats [bkt_off[j], bkt_off[j+1]); [n] = msg_a_off */
    int64_t bkt_slice[NADM_MAX_BUCKETS];  /* floats per rank of bucket j                              */
    int64_t bkt_m0[NADM_MAX_BUCKETS + 1]; /* bucket j holds the V rows of SNPs [bkt_m0[j], bkt_m0[j+1]); [n] = M */
    int64_t bkt_mom[NADM_MAX_BUCKETS];    /* start of the rank's slice of bucket j in its B moments   */
} nadm_flat_layout_t;
int nadm_flat_layout(const nadm_heads_t* hd, int64_t M, int32_t world, int32_t n_buckets, nadm_flat_layout_t* out);

/* Transport of the step's collectives.  The step issues them on hipStreams it names; an implementation must order its work on
 * that stream (RCCL does; a host transport synchronises the stream).  All three operate IN PLACE on float buffers:
 *   reduce_scatter(buf, slice): buf holds world * slice floats; afterwards THIS rank's slice [rank*slice, (rank+1)*slice) holds the
 *                               sum over ranks of that slice (the other slices are scratch)                    (ncclReduceScatter)
 *   all_gather(buf, slice):     every rank contributes its own slice; afterwards buf is complete everywhere    (ncclAllGather)
 *   all_reduce(buf, n):         sum over ranks                                                                 (ncclAllReduce)
 *   async_error():              (may be NULL) nonzero + nadm_last_error() if a collective queued earlier has failed asynchronously
 *                               (ncclCommGetAsyncError); nadm_plan_flush asks, and every step of a plan built with debug != 0
 * nadm_comm_rccl: a communicator of its own over RCCL / xGMI (ncclCommInitRank with `unique_id`, 128 bytes from
 * nadm_comm_rccl_unique_id on rank 0, distributed by the caller -- the reference gets its communicator from
 * init_process_group("nccl"), src/utils.py:88-93).  librccl_path: the librccl.so to dlopen (NULL: "librccl.so"); pass the path of
 * the copy already mapped into the process.  ncclCommInitRank is itself a collective -- it returns when EVERY rank has entered it --
 * so it runs under a watchdog: after timeout_ms (<= 0: wait forever) the call gives up with status 5 and a message naming the
 * rank; the helper thread stays blocked inside the library, i.e. the process is expected to tear down (the reference's behaviour on
 * any rank failure: teardown + re-raise, src/main.py:119-133).  nadm_comm_rccl_probe: dlopen + symbol resolution only -- what can
 * fail without any other rank being involved; callers agree on its outcome BEFORE anyone enters ncclCommInitRank (comm.py).
 * nadm_comm_emulated: rank 0 of `world` ranks with no-op collectives -- the per-rank cost of a world-rank step measured on ONE GPU
 * (bench.py --emulate-world; the run's results are meaningless). */
typedef struct nadm_comm {
    int32_t rank, world;
    void* ctx;
    int (*reduce_scatter)(void* ctx, float* buf, int64_t slice, void* stream);
    int (*all_gather)(void* ctx, float* buf, int64_t slice, void* stream);
    int (*all_reduce)(void* ctx, float* buf, int64_t n, void* stream);
    void (*destroy)(void* ctx);           /* may be NULL */
    int (*async_error)(void* ctx);        /* may be NULL */
} nadm_comm_t;
int  nadm_comm_rccl_probe(const char* librccl_path);
int  nadm_comm_rccl_unique_id(const char* librccl_path, void* id128);
int  nadm_comm_rccl(const char* librccl_path, const void* id128, int32_t rank, int32_t world, int32_t timeout_ms, nadm_comm_t** out);
int  nadm_comm_emulated(int32_t world, nadm_comm_t** out);
void nadm_comm_free(nadm_comm_t* comm);
/* ncclCommAbort instead of ncclCommDestroy: frees a communicator whose collectives may never complete (a peer is gone) */
void nadm_comm_abort(nadm_comm_t* comm);

/* How the work of a step is spread over ranks */
#define NADM_MODE_SINGLE 0   /* one GPU: Adam + restrict_P in the epilogues of passes 2 and 3                                        */
#define NADM_MODE_DP     1   /* samples sharded (the reference's scheme, neural_admixture.py:287,315-319): gradients summed over ranks,
                              * optimizer SHARDED -- reduce-scatter -> Adam (grad_scale 1/world = DDP's mean) + restrict_P on this rank's
                              * 1/world slice of the parameters and ITS moments only -> all-gather of the updated parameters.  Same wire
                              * bytes as the all-reduce, optimizer traffic and Adam-moment memory / world.  Message A (all P) travels on a
                              * side stream underneath the MLP backward, pass 3 and the next step's pass 1; message B (small | V) on the
                              * compute stream behind pass 3 (n_buckets <= 1, the default: the next pass 1 needs all of V, nothing is left
                              * to hide it under) or, n_buckets > 1, as SNP ranges on a second side stream: pass 3 is launched range by
                              * range, behind each range its bucket is reduce-scattered, updated and all-gathered, and the NEXT step's
                              * pass 1 runs as the same ranges, each waiting for its own bucket only.  What that buys is wire time hidden
                              * under pass 3 and pass 1 (~40 us each at 800 rows); what it costs a rank is measured
                              * (profiles/r05_rank_emulation.txt: every cross-stream hand-off is ~10 us on the GPU's timeline).  Issue order
                              * on the communicator (identical on every rank): reduce-scatter A, then per bucket reduce-scatter B_j,
                              * all-gather B_j, then all-gather A -- B, which the next pass 1 waits for, never queues behind A's
                              * all-gather.  comm_a != NULL gives message A a communicator of its own: A and B then share the links
                              * instead of queueing behind each other */
#define NADM_MODE_SNP    2   /* SNPs sharded (8(f)-4): every rank owns M/world SNPs of X, V, P and their Adam state and processes the
                              * GLOBAL batch; two small all-reduces per step (partial Z, partial dQ), Adam in the epilogues with 1/world */

/* Everything the step touches; every pointer is caller-owned device memory (sizes: the entry points above) */
typedef struct nadm_plan_desc {
    int32_t mode, bmax;
    int64_t M, ld;
    nadm_heads_t heads;
    const uint8_t* xp;                    /* resident packed rows (nadm_plan_set_rows replaces it)                             */
    float *params, *grads;                /* flat buffers, nadm_flat_layout(heads, M, comm world in DP mode, else 1)            */
    float *m, *v;                         /* Adam moments: flat like params (single, SNP); DP: [slice_b | slice_a] of THIS rank */
    float *zpart, *Z, *rinv, *Zn, *H, *Q, *dL, *dHpre, *dgp, *dZ, *dqpart, *losspart, *small_part;
    float *zsum, *dqsum;                  /* SNP mode: [bmax*CP], [bmax*SP]                                                     */
    void* qimg; int64_t qimg_head_bytes;  /* nadm_mlp_fwd_images (zero-filled once)                                            */
    void* dzimg; int32_t* dzcnt;          /* nadm_mlp_bwd_image  (C <= 8; counters zero-filled once)                            */
    uint8_t* xg;                          /* nadm_batch_copy_bytes(bmax, M) (C <= 8; NULL: pass 3 reads nadm_plan_set_tiles' copy)   */
    double* loss_acc;                     /* [2]: running sum, last step                                                        */
    const nadm_comm_t* comm;              /* NULL: one rank.  Must outlive the plan                                             */
    const nadm_comm_t* comm_a;            /* DP mode: a second communicator for message A (NULL: `comm` carries both)           */
    int32_t n_buckets;                    /* DP mode: buckets of message B (0, 1: one message; params / grads / m / v are laid
                                           * out by nadm_flat_layout(heads, M, world, n_buckets))                               */
    int32_t p3_whole;                     /* DP mode, n_buckets > 1: != 0 keeps pass 3 ONE launch (the buckets' collectives then
                                           * all start behind it; only the next pass 1 is pipelined against them)                */
    int32_t debug;                        /* != 0: every step asks the communicators for asynchronous errors (a host call each)  */
    int32_t reserved;                     /* 0 */
    float* p2_slab;                       /* pass 2 in sample slices (nadm_decode_bce_sliced): head h's region starts at the sum over the
                                           * heads before it of nadm_decode_slab_floats(M, kp, nadm_decode_slices_max(bmax, M, kp)); NULL (with
                                           * p2_cnt): pass 2 is never sliced                                                        */
    int32_t* p2_cnt;                      /* the heads' counters back to back, nadm_decode_chunks(M, kp) each, zero-filled once    */
    float* p3_slab;                       /* pass 3 in sample slices (nadm_encode_bwd_sliced): nadm_encode_slab_floats(M, CP,
                                           * nadm_encode_slices_max(bmax, M, CP)) floats; NULL (with p3_cnt): pass 3 is never sliced   */
    int32_t* p3_cnt;                      /* nadm_encode_bwd_chunks(M) counters, zero-filled once                                    */
} nadm_plan_desc_t;
typedef struct nadm_plan nadm_plan_t;
int  nadm_plan_create(const nadm_plan_desc_t* desc, nadm_plan_t** out);
void nadm_plan_destroy(nadm_plan_t* plan);
int  nadm_plan_set_rows(nadm_plan_t* plan, const uint8_t* xp);
/* The tiled, cleaned copy of the SAME rows (nadm_tile_packed over the plan's M; caller-owned, must outlive its use): from the next
 * nadm_step / nadm_plan_infer on, pass 1 (C <= 8) and pass 2 (padded K <= 16 with Q images) gather from it; pass3_too != 0: pass 3
 * (C <= 8) as well, and pass 2 then writes no batch copy (desc.xg may be NULL for such a plan).  Every other kernel, and every entry
 * point outside the plan, keeps reading xp.  xt == NULL: back to the row-major matrix; nadm_plan_set_rows forgets the copy too. */
int  nadm_plan_set_tiles(nadm_plan_t* plan, const uint8_t* xt, int64_t rows, int32_t pass3_too);
/* supervised mode (neural_admixture.py:460-474): class per resident row in [-1, n_classes), NADM_LABEL_NONE = no label (the row
 * stays out of the supervised term, nadm_supervised_ce); NULL switches it off */
int  nadm_plan_set_labels(nadm_plan_t* plan, const int32_t* labels, int32_t n_classes, float weight);
/* Adam step count (1-based count of completed steps; 0 after loading parameters) and whether every P entry lies in [0, 1] (true
 * after any step -- restrict_P -- and for the GMM initialisation; while false the loss path clamps the reconstruction before the
 * logarithm, nadm_decode_bce with_loss bit 1).  Callers that run optimizer steps of their own (nadm_adam) keep the count in step. */
int  nadm_plan_set_state(nadm_plan_t* plan, int32_t step_count, int32_t p_in_unit_range);
int32_t nadm_plan_p_in_unit_range(const nadm_plan_t* plan);
int32_t nadm_plan_step_count(const nadm_plan_t* plan);

/* ONE training step on the batch rows idx[0..b) -- gather/decode, forward, loss, backward, gradient exchange, Adam, restrict_P --
 * queued on `stream` (and, in DP mode, on the plan's side streams), asynchronous.  with_loss: also add the step's loss value to
 * loss_acc.  The step may leave work to the NEXT step's launches (single / SNP: the small-parameter update rides in the next
 * pass 1; DP: the messages complete underneath the next step's first launches): nadm_plan_flush makes `stream` see every
 * parameter final (and reports a collective that failed asynchronously).
 * A step that FAILS part-way (a refused launch, a transport error) leaves the plan POISONED: the Adam step count, the pending
 * hand-offs and the side streams are in no defined state, and every later nadm_step / nadm_plan_flush / nadm_plan_infer on it
 * fails fast with a message that says so.  Destroy the plan and build a new one (parameters and moments live in the caller's
 * buffers; what the failed step did to them is undefined). */
int  nadm_step(nadm_plan_t* plan, const int32_t* idx, int32_t b, float lr, int32_t with_loss, void* stream);
int  nadm_plan_flush(nadm_plan_t* plan, void* stream);
/* Encoder only (final Q, neural_admixture.py:369-383; inference.py:71-77): pass 1 + MLP forward -> Q [b, SP] */
int  nadm_plan_infer(nadm_plan_t* plan, const int32_t* idx, int32_t b, void* stream);

/* Matmul precision of the plan's nadm_step and nadm_plan_infer, from the next call on; switching between steps is allowed.
 *   NADM_PRECISION_HIGHEST (the default): fp32-class products -- P, Q, V as three bf16 pieces, dR as hi + lo.
 *   NADM_PRECISION_MEDIUM: bf16-class products, torch.set_float32_matmul_precision('medium') -- P, Q, V as hi + mid (two bf16 pieces,
 *     ~16 bits), dR as ONE bf16 piece (round to nearest even); accumulation, the loss, Adam, restrict_P, the MLP kernels and pass 3
 *     are unchanged.  Heads with padded K > 16 and C > 8 run their fp32 VALU kernels under either setting (results bit-identical);
 *     heads with padded K <= 16 need the plan's Q images (desc.qimg).
 * The plain-phase entry points (nadm_encode_fwd*, nadm_decode_bce*) always compute "highest".  The setter refuses a NULL or poisoned
 * plan and any other value. */
#define NADM_PRECISION_HIGHEST 0
#define NADM_PRECISION_MEDIUM  1
int  nadm_plan_set_precision(nadm_plan_t* plan, int32_t precision);
int32_t nadm_plan_precision(const nadm_plan_t* plan);   /* -1 for NULL */

/* Measurement: HIP events around the launches of a step on the stream they run on.  mask bit i = NADM_T_* below; the records cost
 * ~1 % of a step per bit, hence a mask.  nadm_plan_kernel_ms synchronises, writes the mean duration [ms] of every timed group since
 * the last call (0 where nothing was timed) and clears the records. */
#define NADM_T_ENCODE_FWD 0
#define NADM_T_MLP_FWD    1
#define NADM_T_DECODE_BCE 2
#define NADM_T_MLP_BWD    3
#define NADM_T_ENCODE_BWD 4
#define NADM_T_SYNC_A     5   /* DP: message A on the side stream: from its reduce-scatter to its all-gather, which is issued behind message B (a span) */
#define NADM_T_SYNC_B     6   /* DP: message B on its side stream: from the first bucket's small-gradient sum + reduce-scatter to the last bucket's all-gather (a span) */
#define NADM_T_COUNT      7
int  nadm_plan_timing(nadm_plan_t* plan, uint32_t mask);
int  nadm_plan_kernel_ms(nadm_plan_t* plan, float* ms /* [NADM_T_COUNT] */, int32_t* counts /* [NADM_T_COUNT], may be NULL */);
/* With NADM_T_SYNC_B in the mask: the mean duration [ms] of every BUCKET of message B on its side stream (reduce-scatter -> Adam ->
 * all-gather of the range), bucket j in ms[j]; returns through *n the number of buckets.  Call before nadm_plan_kernel_ms (which
 * clears the records). */
int  nadm_plan_bucket_ms(nadm_plan_t* plan, float* ms /* [NADM_MAX_BUCKETS] */, int32_t* n);
int32_t nadm_plan_poisoned(const nadm_plan_t* plan);

#ifdef NADM_TEST_HOOKS   /* the TEST build only: route nadm_mlp_fwd / nadm_mlp_bwd to the generic (any hidden width) kernels even where the
                          * register-resident ones apply, so that tests can compare the two.  Process-wide. */
void nadm_test_force_generic_mlp(int32_t on);
#endif

/* ---- 8(f)-3: log-likelihood report from the packed matrix (src/utils_c/utils.pyx:15-40, called train.py:134-146) -----
 * partial[b] (b < nadm_loglik_blocks(M) = 8 row slices x ceil(M / 1024), double, device) = sum over the block's 1024 SNPs and
 * its slice of the `rows` rows of g*log(rec) + (2-g)*log1p(-rec) over non-missing calls, rec = clip(Q_i.P_j, eps, 1-eps), g = clip(code, eps, 2-eps), all
 * in float64 like the reference.  P [M,K] float32 (unpadded, the returned Ps[i]), Q [rows, >=K] float32 with row stride
 * q_stride, both on the device; K <= 16; eps in [1e-9, 0.5) (the reference's: 1e-6).  The caller adds the partials (fixed order).
 * (The logarithms are taken of products over 16 genotypes: the same float64 sum to ~1e-15 relative.) */
int64_t nadm_loglik_blocks(int64_t M);
int nadm_loglik(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, const float* P, const float* Q, int32_t K,
                int32_t q_stride, double eps, double* partial, void* stream);

/* ---- projection: refine Q against a FIXED P with masked EM steps ------------------------------------------------------------
 * What ADMIXTURE-family tools call projection (ADMIXTURE -P): P stays as trained, every sample's Q row is fitted to its OWN
 * observed calls by maximum likelihood.  One call = one EM step of the binomial admixture model (the FRAPPE / ADMIXTURE
 * update: no step size, keeps sum(q) = 1, never lowers ll while the clip is inactive) for the rows idx[0..b) (idx == NULL:
 * rows 0..b; any order, duplicates allowed) and ONE head of k columns.  Codes g in {0, 1, 2} are observed, 3 is missing, only
 * SNPs j < M count:
 *     r_j  = clip( sum_k q_k p_jk , eps, 1 - eps )
 *     a_k  = sum over observed j of [ p_jk g_j / r_j  +  (1 - p_jk) (2 - g_j) / (1 - r_j) ]
 *     n    = number of observed j
 *     ll   = sum over observed j of [ g_j log r_j + (2 - g_j) log(1 - r_j) ]              (at the INPUT q)
 *     q'_k = q_k a_k / (2n);   q''_k = max(q'_k, qmin);   q_out = q'' / sum_k q''_k
 *     n == 0:  q_out = q_in exactly, ll = 0
 * P [M, kp] (kp = nadm_pad_k(k), pad cols 0); Qin / Qout rows of b with row stride q_stride (a multiple of 4, >= kp; Qout may
 * be Qin; padded columns k >= K come out 0); eps in [1e-9, 0.5) (the log-likelihood report's is 1e-6), qmin in [0, 1) (1e-6);
 * loglik double [b] and nobs int32 [b] may be NULL -- loglik == NULL skips the logarithms, the expensive part of a step.
 * scratch: nadm_project_scratch_floats(b, M, kp) floats.  xp, P, Qin, Qout, scratch 16-byte aligned; ld % 16 == 0, ld < 2^32.
 * A missing call and a SNP >= M enter every sum as exactly +0.0f (a sample's result does not depend on P where its call is
 * missing, nor on the pad bits of its last byte); sums are fp32 within a 256-SNP chunk, the chunks' partials are added in
 * float64 in a fixed order that depends on (M, kp) alone (a_k: contiguous ranges of chunks, each in chunk order, then the
 * ranges in order; n, ll: strided over the lanes, then a fixed butterfly); no floating-point atomics: the same inputs give
 * the same bits.  kp <= 16 is the fast path, wider
 * heads run the same kernel with P staged in pieces.  Every refusal is reported before anything is launched. */
int64_t nadm_project_scratch_floats(int32_t b, int64_t M, int32_t kp);
int nadm_project_q(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                   const float* P, int32_t k, int32_t kp, const float* Qin, float* Qout, int32_t q_stride,
                   float eps, float qmin, double* loglik, int32_t* nobs, float* scratch, void* stream);

/* ---- the weighted step and the bootstrap draw: standard errors for Q by resampling SNPs (ADMIXTURE -B) ----------------------
 * A bootstrap replicate is the same EM on the weighted likelihood sum_j w_j l_j, w_j = how often SNP j was drawn.  No resampled
 * matrix is made: nadm_project_q_w is nadm_project_q with one more operand, w: M bytes on the device, 16-byte aligned, no byte at
 * or beyond M is read.  Same two launches, same scratch (nadm_project_scratch_floats), same refusals before any launch, and a
 * refusal of w == NULL.  With wf = (float)w_j (exact), per observed j:
 *     a_k += (1 - p_jk) (wf t0) + p_jk (wf t1)        t1 = g_j / r_j, t0 = (2 - g_j) / (1 - r_j) as above
 *     n   += w_j                                       (int32, exact: the caller keeps sum_j w_j <= 2^31 - 1)
 *     ll  += wf [ g_j log r_j + (2 - g_j) log(1 - r_j) ]
 * and the fold is the unweighted one: q'_k = q_k a_k / (2n), n == 0 returns the row as it came.  w = 1 everywhere gives the bits
 * of nadm_project_q (Q, ll, n).  A SNP with w_j = 0 enters every sum as exactly +0.0f / 0: the result does not depend on P or on
 * the call there (finite P).  A 256-SNP chunk whose weights are all zero is skipped and its partials written as +0.0f / 0, the
 * bits the long way gives.  No floating-point atomics: the same inputs give the same bits.  Qout == Qin is allowed.
 * nadm_project_p needs no weights: a SNP's weight multiplies num and den alike and cancels, so a replicate's P step is the
 * unweighted one.
 *
 * The bootstrap draw (host side; bootstrap.block_weights restates it in numpy): the M SNPs are cut into nb = ceil(M / block)
 * blocks of `block` consecutive SNPs (the last may be short); for replicate r, with mix32 and row_key of the cv fold below, all
 * arithmetic in uint32, wrapping:
 *     key   = row_key(seed, r)
 *     c_t   = ( (uint64) mix32( key ^ (uint32)t ) * nb ) >> 32          the block that draw t = 0 .. nb - 1 picks
 *     cnt_c = #{ t : c_t == c }                 w_j = cnt_{j / block}
 * Refused: nb < 2, M > 2^31, any cnt > 255 (a weight is a byte).  row_key(0, 0) = 0x01FCE552, row_key(0, 1) = 0xB21C8E52; seed 0,
 * 12 blocks, replicate 0: the draws pick 8 7 0 5 2 4 11 2 4 10 11 3, so cnt = 1 0 2 1 2 1 0 1 1 0 1 2; replicate 1:
 * cnt = 2 1 1 0 1 1 2 3 0 0 0 1. */
int nadm_project_q_w(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                     const float* P, int32_t k, int32_t kp, const float* Qin, float* Qout, int32_t q_stride,
                     float eps, float qmin, double* loglik, int32_t* nobs, float* scratch, const uint8_t* w, void* stream);

/* ---- the other half: refit P against a FIXED Q with a masked EM step -------------------------------------------------------
 * With nadm_project_q this is the FRAPPE / ADMIXTURE block EM over the OBSERVED calls only.  One call = one step for the rows
 * idx[0..b) (idx == NULL: rows 0..b; any order, a duplicate counts as often as it occurs), Q [b, k] (row s belongs to idx[s],
 * row stride q_stride, a multiple of 4, >= kp, pad cols 0) and ONE head Pin [M, kp] (kp = nadm_pad_k(k), pad cols 0):
 *     rr_ij = sum_k q_ik p_jk;   r = clip(rr, eps, 1 - eps);   u = clip(1 - rr, eps, 1 - eps)       (1 - r from the UNCLIPPED product)
 *     B_jk  = sum over observed i of q_ik g_ij / r_ij          C_jk = sum over observed i of q_ik (2 - g_ij) / u_ij
 *     num   = p_jk B_jk;   den = num + (1 - p_jk) C_jk
 *     p'_jk = clip(num / den, pmin, 1 - pmin)  if den > 0,  else  p_jk with its bits unchanged (not clipped)
 *     n_j   = number of observed i
 * Pout [M, kp] may be Pin; its pad columns are written 0, rows >= M are never written; nobs_snp int32 [M] may be NULL.
 * eps in [1e-9, 0.5), pmin in [0, 0.5) (both 1e-6 by default in the Python layer).  scratch: nadm_project_p_scratch_floats(b, M, kp)
 * floats.  xp, Q, Pin, Pout, scratch 16-byte aligned; ld % 16 == 0, ld < 2^32.
 * A missing call and a SNP >= M enter every sum as exactly +0.0f.  The batch's 64-sample tiles are cut into
 * nadm_project_p_slices(b, M) slices of whole tiles (1 for b <= 64; more while M alone does not fill the chip; never more than
 * 4096 samples in one slice): sums are fp32 within a slice in sample order, the slices' partials are added in float64 in slice
 * order, num / den and the clip are float64.  The order depends on (b, M, kp) alone and there are no floating-point atomics:
 * the same inputs give the same bits.  Every refusal is reported before anything is launched. */
int32_t nadm_project_p_slices(int32_t b, int64_t M);
int64_t nadm_project_p_scratch_floats(int32_t b, int64_t M, int32_t kp);
int nadm_project_p(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                   const float* Q, int32_t q_stride, int32_t k, int32_t kp, const float* Pin, float* Pout,
                   float eps, float pmin, int32_t* nobs_snp, float* scratch, void* stream);

/* ---- admixture-aware kinship (REAP, Thornton et al. 2012) of one block of sample pairs ---------------------------------------
 * Pairwise kinship from individual-specific allele frequencies: the check of the model's assumption that the samples are
 * unrelated.  One call = the rows idxA[0..ba) against the rows idxB[0..bb) (idx == NULL: rows 0..b; any order, a duplicate row
 * is allowed, the two lists may be the same), QA [ba, k] / QB [bb, k] (row s belongs to idx[s], row stride q_stride, a multiple
 * of 4, >= kp, pad cols 0; may be the same pointer) and ONE head P [M, kp] (kp = nadm_pad_k(k), pad cols 0).  Codes g in
 * {0, 1, 2} are observed, 3 is missing:
 *     pi_ij  = sum_k q_ik p_jk                                      (fp32, fused multiply-adds, k in order)
 *     m_ij   = 1 if the call is observed, j < M and pimin <= pi_ij <= 1 - pimin (1 - pimin rounded to fp32), else 0
 *     d_ij   = m_ij (g_ij - 2 pi_ij)        s_ij = m_ij sqrt(max(pi_ij (1 - pi_ij), 0))
 *     num_ab = sum_j d_aj d_bj      den_ab = sum_j s_aj s_bj      n_ab = sum_j m_aj m_bj
 * The kinship coefficient is phi_ab = num_ab / (4 den_ab) (the caller divides; den_ab = 0 has none), the inbreeding coefficient
 * of a sample f_a = 2 phi_aa - 1.  num, den double [ba, bb], nobs int32 [ba, bb] (may be NULL), row-major.  pimin in [0, 0.5);
 * 0 lets every observed call with 0 <= pi <= 1 count -- the test on pi stays: a Q row that sums to 1 + ulp against a P of 1.0
 * gives a pi just above 1 in fp32, and that call is dropped (its s would be 0 anyway).  ba, bb in 1..NADM_KINSHIP_MAX_ROWS.  scratch: nadm_kinship_scratch_floats(ba, bb, M) floats
 * (grows with ba, bb and M).  xp, P, QA, QB, scratch 16-byte aligned; ld % 16 == 0, ld < 2^32.
 * A missing call, a SNP >= M and a masked pi enter all three sums as exactly +0.0f (the result does not depend on P where both
 * calls are missing, nor on the pad bits of a row's last byte).  d and s are carried as two round-to-nearest bf16 pieces each
 * (value to 2^-17 relative) and multiplied on the matrix pipe as hi.hi + hi.lo + lo.hi with fp32 accumulation (the dropped
 * lo.lo term is below 2^-16 of |d_a||d_b|); m is exact in one piece.  The 256-SNP chunks are cut into
 * nadm_kinship_ranges(ba, bb, M) contiguous ranges (more than one while the 64 x 64 tiles of the block alone do not fill the
 * chip); one fp32 accumulator never covers more than 2^18 SNPs, so n -- a sum of ones below 2^24 -- is exact.  The ranges'
 * partials are added in float64 in range order.  The order depends on (ba, bb, M, kp) alone and there are no floating-point
 * atomics: the same inputs give the same bits.  kp <= 16 keeps a sample's Q row in registers, wider heads re-read it.
 * Every refusal is reported before anything is launched. */
#define NADM_KINSHIP_MAX_ROWS 4096
int32_t nadm_kinship_ranges(int32_t ba, int32_t bb, int64_t M);
int64_t nadm_kinship_scratch_floats(int32_t ba, int32_t bb, int64_t M);
int nadm_kinship(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                 const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride, float pimin,
                 double* num, double* den, int32_t* nobs, float* scratch, void* stream);

/* ---- IBD-sharing sums given ancestry (PC-Relate, Conomos et al. 2016) of one block of sample pairs -------------------------------
 * What tells a parent-child pair from full siblings (both phi = 0.25): the probabilities k0, k1, k2 that a pair shares 0, 1 or 2
 * alleles identical by descent.  The estimators are PC-Relate's (Conomos et al. 2016, eqs. for k2 and k0), with the admixture
 * model's individual-specific frequencies pi in the place of its PC-predicted ones, as REAP (Thornton et al. 2012) uses them.  The
 * rows, P, QA / QB, pi and the mask m are those of nadm_kinship, word for word; fA [ba] / fB [bb] are the samples' inbreeding
 * coefficients (f_a = 2 phi_aa - 1 of nadm_kinship), an INPUT, one float per list position (may be the same pointer, as QA / QB).
 *     v_ij  = pi (1 - pi)
 *     gD_ij = pi if g = 0;  0 if g = 1;  1 - pi if g = 2            (dominance coding; E[gD] = v (1 + f))
 *     e_ij  = m (gD - v (1 + f_i))          vm_ij = m v
 *     u_ij  = m pi^2                        w_ij  = m (1 - pi)^2
 *     z0_ij = m [g = 0]                     z2_ij = m [g = 2]
 *     k2num_ab = sum_j e_a e_b              k2den_ab = sum_j vm_a vm_b
 *     ibs0_ab  = sum_j (z0_a z2_b + z2_a z0_b)                      (int32, exact)
 *     exp0_ab  = sum_j (u_a w_b + w_a u_b)                          (the expected share of opposite homozygotes with no allele IBD)
 * The caller forms, in float64, with phi_ab of nadm_kinship on the same block and pimin:
 *     k2 = k2num / k2den (none where k2den = 0);  k0 = ibs0 / exp0 if phi >= 2^-2.5 (none where exp0 = 0), else 1 - 4 phi + k2;
 *     k1 = 1 - k0 - k2.
 * Expected (k0, k1, k2): unrelated (1, 0, 0), parent-child (0, 1, 0), full sibs (1/4, 1/2, 1/4), duplicate (0, 0, 1), second degree
 * (1/2, 1/2, 0).  The estimates are unconstrained.  Only these formulas are promised, no other tool's printed digits.
 * k2num, k2den, exp0 double [ba, bb], ibs0 int32 [ba, bb], row-major, none may be NULL.  K <= 16 (a sample's Q row lives in its
 * builder thread's registers; a wider head is refused).  pimin in [0, 0.5).  ba, bb in 1..NADM_IBD_MAX_ROWS.  scratch:
 * nadm_ibd_scratch_floats(ba, bb, M) floats (grows with ba, bb and M).  xp, P, QA, QB, scratch 16-byte, the double outputs 8-byte,
 * ibs0, fA, fB and the lists 4-byte aligned; ld % 16 == 0, ld < 2^32.
 * A missing call, a SNP >= M, a row past the list and a masked pi enter every sum as exactly +0.0f WHATEVER f IS (a NaN included):
 * the terms are cleared with bit masks, never multiplied by 0.  e, vm, u and w are formed in fp32 and carried as two
 * round-to-nearest bf16 pieces each (value to 2^-17 relative), multiplied on the matrix pipe (v_mfma_f32_16x16x32_bf16) as hi.hi +
 * hi.lo + lo.hi with fp32 accumulation; z0 and z2 are exact in one piece: 14 instructions per 16 x 16 tile and 32 SNPs.  The 256-SNP
 * chunks are cut into nadm_ibd_ranges(ba, bb, M) contiguous ranges (the plan of nadm_kinship); one fp32 accumulator never covers more
 * than 2^18 SNPs, so ibs0 -- a sum of ones below 2^24 -- is exact.  The ranges' partials are added in float64 in range order.  Against
 * float64: |k2num - k2num64| <= 2^-15 sum_j mag_a mag_b with mag = m (|gD| + v (1 + |f|)) (e is a difference formed in fp32),
 * |k2den - k2den64| <= 2^-15 k2den64, |exp0 - exp0_64| <= 2^-15 exp0_64.  The order depends on (ba, bb, M, kp) alone and there are no
 * floating-point atomics: the same inputs give the same bits.  Every refusal is reported before anything is launched.  Asynchronous
 * on `stream`. */
#define NADM_IBD_MAX_ROWS 4096
int32_t nadm_ibd_ranges(int32_t ba, int32_t bb, int64_t M);
int64_t nadm_ibd_scratch_floats(int32_t ba, int32_t bb, int64_t M);
int nadm_ibd(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
             const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride,
             const float* fA, const float* fB, float pimin,
             double* k2num, double* k2den, int32_t* ibs0, double* exp0, float* scratch, void* stream);

/* ---- KING-robust kinship (Manichaikul et al. 2010) of one block of sample pairs, from the genotypes alone -----------------------
 * The check of the "unrelated samples" assumption BEFORE a fit: it needs no allele frequencies and no model, and it is robust to
 * population structure.  One call = the rows idxA[0..ba) against the rows idxB[0..bb) (idx == NULL: rows 0..b; any order, a
 * duplicate row is allowed, the two lists may be the same).  Codes 0, 1, 2 are observed, 3 is missing.  For samples a, b, over the
 * SNPs j < M at which BOTH are observed:
 *     n      = the number of such SNPs
 *     hethet = #(g_a = 1 and g_b = 1)
 *     ibs0   = #(g_a = 0, g_b = 2) + #(g_a = 2, g_b = 0)
 *     het_a  = #(g_a = 1),   het_b = #(g_b = 1)                     (each among the jointly observed SNPs)
 *     phi_ab = 1/2 - (het_a + het_b - 2 hethet + 4 ibs0) / (4 min(het_a, het_b))
 * phi_ab is NaN where min(het_a, het_b) = 0.  The library returns the five counts; the caller forms the numerator as an integer and
 * divides once, in float64.  Expected: 0.5 for a duplicate (exactly 0.5 on the diagonal whenever the sample has a heterozygous
 * call), 0.25 for first degree, 0.125 for second degree, 0 for an unrelated pair from one population, NEGATIVE for unrelated pairs
 * from different populations (the estimator's known behaviour, harmless for a cutoff).  The statistic does not change under the
 * reader's 0 <-> 2 flip.  This is the between-family "robust" estimator with the min denominator; neither KING's nor plink2's
 * printed digits are promised, only this formula.
 * counts int32 [5, ba, bb], row-major: n, hethet, ibs0, het_a, het_b.  ba, bb in 1..NADM_KING_MAX_ROWS, 0 < M < 2^31 (the counts are
 * int32).  scratch: nadm_king_scratch_ints(ba, bb, M) int32 (grows with ba, bb and M; <= 0: the shape is refused).  xp and scratch
 * 16-byte, idxA, idxB and counts 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32.
 * The sums run on the matrix pipe (v_mfma_i32_16x16x64_i8, the SNP axis on its k): per side a call enters as the four 0 / 1 int8
 * indicators h (code 1), z0 (code 0), z2 (code 2) and o (observed); six products per tile -- h.h, z0.z2 + z2.z0, h.o, o.h, o.o --
 * give the five counts, int32 and EXACT.  SNPs >= M, the pad fields of a row's last byte, the bytes behind it and rows past the
 * list enter as the missing code: exactly 0 in every count.  The 256-SNP chunks are cut into nadm_king_ranges(ba, bb, M) contiguous
 * ranges (more than one while the 64 x 64 tiles of the block alone do not fill the chip); a second launch adds the ranges'
 * partials in range order.  No floating point and no atomics on the device: the same inputs give the same bits.  Every refusal is
 * reported before anything is launched.  Asynchronous on `stream`. */
#define NADM_KING_MAX_ROWS 4096
int32_t nadm_king_ranges(int32_t ba, int32_t bb, int64_t M);
int64_t nadm_king_scratch_ints(int32_t ba, int32_t bb, int64_t M);
int nadm_king(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
              int32_t* counts, int32_t* scratch, void* stream);

/* ---- LD pruning: windowed r^2 of neighbouring SNPs on the matrix pipe, and the keep-list ---------------------------------------
 * ADMIXTURE-type models assume SNPs in linkage equilibrium; the usual preparation is plink's --indep-pairwise.  These entries do it
 * on the packed matrix already in HBM.  Codes g in {0, 1, 2} are observed, 3 is missing; o = 1 where a call is observed, else 0.
 * Rows: idx[0..rows) (idx == NULL: rows 0..rows; any order, a duplicate counts as often as it occurs), rows in 1..2^24.
 *
 * nadm_snp_counts: per SNP j < M over those rows, cnt[j] = { n_obs = sum o, sum g o, sum g^2 o } (int32 [M, 3], zeroed here).  A
 * plain vector kernel, row slices added with integer atomics: exact, the same bits whatever the order.
 *
 * nadm_ld_band: entry (j - m0, d) of r2 [m1 - m0, W] (and of mom [m1 - m0, W, 6], which may be NULL) is the pair
 * (a, b) = (j, j + 1 + d) for m0 <= j < m1, 0 <= d < W.  The six moments, over the rows where BOTH calls are observed (every term
 * is masked to 0 where its own call is missing):
 *     n   = sum o_a o_b        Sa  = sum g_a o_b        Sb  = sum o_a g_b
 *     Sab = sum g_a g_b        Saa = sum g_a^2 o_b      Sbb = sum o_a g_b^2
 * and, in int64,   cov = n Sab - Sa Sb,   va = n Saa - Sa^2,   vb = n Sbb - Sb^2,
 *     r2 = ((double)cov * (double)cov) / ((double)va * (double)vb)        (two products and a division, each one IEEE operation)
 * r2 is exactly 0.0 where va == 0, vb == 0 or b >= M; the moments are 0 where b >= M.  rows <= 2^24 keeps cov, va, vb below 2^53.
 * The products run on the matrix pipe (v_mfma_i32_16x16x64_i8, samples on its k axis): per side a SNP enters as the three int8
 * pieces o in {0,1}, g o in {0,1,2} and g^2 o in {0,1,4}; the sums are int32 and EXACT (at most 4 rows <= 2^26).  The pad bits of
 * a row's last byte, rows beyond `rows` and SNPs >= M enter as exactly 0.  Integer sums: the same inputs give the same bits, no
 * floating-point atomics, no scratch.  W in 1..NADM_LD_MAX_WINDOW, 0 <= m0 < m1 <= M.
 * Both: ld >= ceil(M/4), ld % 16 == 0, ld < 2^32; xp 16-byte, idx / cnt / mom 4-byte, r2 8-byte aligned.
 *
 * nadm_select_snps: out[r, j'] = the code of xp[r, keep[j']] for r < rows, j' < M_out; flip != 0 exchanges the codes 0 and 2 (3
 * stays 3).  keep int64 [M_out] on the device, ascending, values in [0, M_in) (M_in <= 4 ld_in: the caller's; a value outside the
 * row is not followed); out [rows, ld_out], ld_out >= ceil(M_out/4), the row padding is written as zeros.  keep 8-byte aligned.
 *
 * Every refusal of the three is reported before anything is launched.  Asynchronous on `stream`.
 *
 * nadm_ld_sweep (host code, synchronous, no GPU): the greedy pass that turns the band of [m0, m1) into removals.  r2 [m1 - m0, W]
 * as written by nadm_ld_band (host copy), maf double [M], chrom int32 [M] (may be NULL: one chromosome), kept uint8 [M] in/out:
 *     for i = m0 .. m1 - 1 ascending, if kept[i]:
 *       for d = 0 .. W - 1 ascending, j = i + 1 + d < M:
 *         stop at the first j with chrom[j] != chrom[i];  skip a j with kept[j] == 0;
 *         if r2[i - m0, d] > thr: remove the SNP with the smaller maf -- j on a tie; if i was removed, go on with the next i.
 * Calls over consecutive ranges [m0, m1) with the same `kept` equal ONE call over [0, M): the caller holds one range of the band
 * at a time.  maf_j = min(S, 2 n - S) / (2.0 n) from nadm_snp_counts (n = n_obs, S = sum g o), 0 where n = 0.  This is plink's
 * --indep-pairwise with a step of 1 and without its window bookkeeping; plink's list is not promised. */
#define NADM_LD_MAX_WINDOW 1024
int nadm_snp_counts(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int32_t* cnt, void* stream);
int nadm_ld_band(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int64_t m0, int64_t m1, int32_t W,
                 double* r2, int32_t* mom, void* stream);
int nadm_select_snps(const uint8_t* xp, int64_t ld_in, int64_t rows, const int64_t* keep, int64_t M_out, int32_t flip,
                     uint8_t* out, int64_t ld_out, void* stream);
int nadm_ld_sweep(const double* r2, int64_t m0, int64_t m1, int32_t W, int64_t M, const double* maf, const int32_t* chrom,
                  double thr, uint8_t* kept);

/* ---- Admixture dating: weighted admixture LD summed into bins of genetic distance -------------------------------------------------
 * The covariance of the genotypes at two SNPs, weighted at each SNP by the allele-frequency difference of the two sources, decays
 * as exp(-n d) with the genetic distance d for an admixture n generations ago (ROLLOFF, Moorjani et al. 2011; ALDER, Loh et al.
 * 2013).  nadm_wld sums that statistic over EVERY pair of SNPs within reach, exactly, on the packed matrix already in HBM; the
 * binning grid, the weights, the fit and its jackknife are the caller's (admixdate.py).
 *
 * Rows: idx[0..rows) (idx == NULL: rows 0..rows; any order, a duplicate counts as often as it occurs), rows in 2..2^24.
 * Pairs: every (a, b) with m0 <= a < b < m1 and b - a <= W.  cell int32 [M], values >= 0 and nondecreasing: a SNP's genetic
 * position on a grid of one bin width; the bin of a pair is cell[b] - cell[a], a pair with a bin >= nbins is dropped.  (A caller
 * with several chromosomes calls once per chromosome range and leaves a gap of more than nbins cells between them.)
 * wt double [C, M], curve-major, C in 1..NADM_WLD_MAX_CURVES; nmin >= 2.
 *
 * Moments, over the rows where BOTH calls are observed, as nadm_ld_band defines them:
 *     n = sum o_a o_b      Sa = sum g_a o_b      Sb = sum o_a g_b      Sab = sum g_a g_b
 * on the matrix pipe (v_mfma_i32_16x16x64_i8, samples on its k axis; per side the two int8 pieces o and g o), int32 and EXACT.  The
 * pad bits of a row's last byte, rows beyond `rows` and SNPs >= M enter as the missing code.  A pair with n < nmin is skipped.
 * Per counted pair, in this order, every step ONE IEEE float64 operation, nothing contracted:
 *     v = (double)(n Sab - Sa Sb) / (double)(n (n - 1))          numerator and denominator formed in int64: the unbiased covariance
 *     t = ((v * wt[c][a]) * wt[c][b]) * 2^32                       for every curve c
 *     q = llrint(t)                                               round to nearest, ties to even
 * Outputs: sum int64 [C, nbins], sum[c][bin] = the sum of q over the bin's pairs; cnt int64 [nbins], the pairs counted per bin.
 * Both are zeroed here.  The sums are integers added with 64-bit integer atomics: the same inputs give the same bits in any order;
 * no floating-point atomics, no scratch.
 * Overflow: |v| <= 2 always, and the caller promises |wt| <= 1, so |q| <= 2^33: ONE call may add at most 2^29 pairs to one bin
 * (check cnt after the call); the rounding moves a bin's mean, sum / cnt / 2^32, by less than 2^-33.
 * The reader's 0 <-> 2 flip of a SNP leaves the statistic unchanged when the weights are taken from frequencies of the same
 * orientation: the covariance changes sign and so does that SNP's weight.
 * W in 1..NADM_WLD_MAX_SPAN, nbins in 1..NADM_WLD_MAX_BINS, 0 <= m0 < m1 <= M; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32; xp 16-byte,
 * wt / sum / cnt 8-byte, cell / idx 4-byte aligned.  Every refusal is reported before anything is launched.  Asynchronous on `stream`. */
#define NADM_WLD_MAX_CURVES 32
#define NADM_WLD_MAX_BINS 4096
#define NADM_WLD_MAX_SPAN 65536
int nadm_wld(const uint8_t* xp, int64_t ld, const int32_t* idx, int64_t rows, int64_t M, int64_t m0, int64_t m1, int32_t W,
             const int32_t* cell, const double* wt, int32_t C, int32_t nbins, int32_t nmin, int64_t* sum, int64_t* cnt, void* stream);

/* ---- Hardy-Weinberg proportions given ancestry: the per-SNP score test of an inbreeding coefficient ----------------------------
 * The likelihood itself is the model's third assumption: a genotype is binomial(2, pi_ij), i.e. Hardy-Weinberg proportions GIVEN the
 * sample's ancestry.  SNPs that break it (heterozygote drop-out, paralogs, batch effects) bias P and Q; plink's plain --hwe rejects
 * good SNPs of a structured panel through the Wahlund effect.  One call = the rows idx[0..b) (idx == NULL: rows 0..b; any order, a
 * duplicate counts as often as it occurs), Q [b, k] (row s belongs to idx[s], row stride q_stride, a multiple of 4, >= kp, pad cols
 * 0) and ONE head P [M, kp] (kp = nadm_pad_k(k), pad cols 0).  Codes g in {0, 1, 2} are observed, 3 is missing:
 *     pi_ij  = sum_k q_ik p_jk                                      (fp32, fused multiply-adds, k in order, as nadm_kinship)
 *     m_ij   = 1 if the call is observed, j < M and pimin <= pi_ij <= 1 - pimin (1 - pimin rounded to fp32), else 0
 *     r = clip(pi, eps, 1 - eps);   u = clip(1 - pi, eps, 1 - eps)  (u from the UNCLIPPED pi, as nadm_project_p)
 *     t_ij   = r / u if g = 0;   -1 if g = 1;   u / r if g = 2
 *     U_j    = sum_i m_ij t_ij                  Hexp_j = sum_i m_ij 2 pi_ij (1 - pi_ij)
 *     n_j    = sum_i m_ij                       Hobs_j = sum_i m_ij [g_ij == 1]
 * t is the score of a per-SNP inbreeding coefficient F at F = 0 in P(g = 0) = (1 - pi)^2 + F pi (1 - pi), P(g = 1) = 2 pi (1 - pi)
 * (1 - F), P(g = 2) = pi^2 + F pi (1 - pi): E t = 0 and Var t = 1 for every pi, and the cross information of F with pi is 0.  The
 * caller forms Z_j = U_j / sqrt(n_j) (N(0, 1) under the model, positive: excess homozygotes), F_j = U_j / n_j and 1 - Hobs_j /
 * Hexp_j; the only divisions by sums are the caller's.  U, Hexp double [M], nobs, Hobs int32 [M]; Hexp and Hobs may be NULL.
 * eps in [1e-9, 0.5), pimin in [0, 0.5) (t is heavy-tailed for pi near 0 or 1: pimin is the guard).  scratch:
 * nadm_snp_hwe_scratch_floats(b, M) floats (grows with b and with M).  xp, Q, P, scratch 16-byte, U, Hexp 8-byte, nobs, Hobs, idx
 * 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32.
 * A missing call, a row past the list, a SNP >= M and a masked pi enter every sum as exactly +0.0f / 0 (the result does not depend
 * on the pad bits of a row's last byte, nor on P at a SNP nobody observes).  t is num * rcp(den) with the hardware's 1-ulp
 * reciprocal.  The batch's 64-sample tiles are cut into nadm_snp_hwe_slices(b, M) slices of whole tiles (1 for b <= 64; more while
 * M alone does not fill the chip; never more than 4096 samples in one slice): U and Hexp are fp32 sums within a slice in sample
 * order, the slices' partials are added in float64 in slice order; n and Hobs are integer sums, exact.  The order depends on (b, M)
 * alone and there are no floating-point atomics: the same inputs give the same bits.  Every refusal is reported before anything is
 * launched. */
int32_t nadm_snp_hwe_slices(int32_t b, int64_t M);
int64_t nadm_snp_hwe_scratch_floats(int32_t b, int64_t M);
int nadm_snp_hwe(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                 const float* Q, int32_t q_stride, int32_t k, int32_t kp, const float* P,
                 float eps, float pimin, double* U, double* Hexp, int32_t* nobs, int32_t* Hobs,
                 float* scratch, void* stream);

/* ---- Cross-validation over held-out CALLS: the fold of a call, the masked copy, the held-out deviance ----------------------------
 * ADMIXTURE's --cv: hide a random fold of the observed genotype calls, refit on the rest (nadm_project_q / nadm_project_p on the
 * masked copy, unchanged), score how well the refit predicts the hidden calls by the binomial deviance; the K with the lowest
 * error per held-out call is the one to take.
 *
 * The fold of a call is a fixed function of (seed, matrix row i, SNP j), all arithmetic in uint32, wrapping:
 *     mix32(x):          x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *     row_key(seed, i) = mix32( mix32( (uint32)i ^ (uint32)(seed >> 32) ) + (uint32)seed + 0x9E3779B9 )
 *     fold(seed, i, j) = ( (uint64) mix32( row_key(seed, i) ^ (uint32)j ) * folds ) >> 32                 in 0 .. folds - 1
 * i is the row's index in the WHOLE matrix: row0 + the row within the call, so that calls over row ranges agree with one call over
 * all rows.  Both entries refuse row0 < 0, row0 + rows > 2^31, M > 2^31, folds outside 2..NADM_CV_MAX_FOLDS and fold outside
 * 0..folds-1.  mix32(0, 1, 2, 0xFFFFFFFF) = 0x0, 0x688990C0, 0xD1132181, 0x6768824A; seed 0, 5 folds, row 0, SNPs 0..11:
 * 3 3 0 2 0 1 4 1 1 4 4 1.
 *
 * nadm_cv_mask: xo [rows, ld] = xp [rows, ld] with every call j < M that is observed (code 0, 1 or 2) and whose fold equals `fold`
 * replaced by code 3 (missing).  Everything else is copied bit for bit: missing calls, the unused fields of a row's last SNP byte,
 * the bytes from ceil(M/4) to ld.  xo == xp is allowed (in place); any other overlap of the two [rows, ld] ranges is refused.  A
 * plain vector kernel (16-byte loads and stores, 64 calls per thread), no scratch.  Exact: the same inputs give the same bytes.
 * xp, xo 16-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32.  The EM entries then run on xo as on any packed matrix.
 *
 * nadm_cv_deviance: rows 0..b of xp (the ORIGINAL matrix; no gather list: the fold belongs to the matrix row), Q [b, k] (row s
 * belongs to row s, row stride q_stride, a multiple of 4, >= kp, pad cols 0) and ONE head P [M, kp] (kp = nadm_pad_k(k), pad cols
 * 0).  Over the calls with j < M, code g != 3 and fold(seed, row0 + i, j) == fold:
 *     pi_ij  = sum_k q_ik p_jk                                      (fp32, fused multiply-adds, k in order, as nadm_snp_hwe)
 *     r = clip(pi, eps, 1 - eps);   u = clip(1 - pi, eps, 1 - eps)  (u from the UNCLIPPED pi, as nadm_project_p)
 *     d_ij   = -2 [ g ln r + (2 - g) ln u ] - 4 ln 2 [g == 1]       (the binomial deviance: 0 for a perfect prediction)
 *     dev_j  = sum_i d_ij                       nheld_j = the number of such calls
 * dev double [M], nheld int32 [M].  eps in [1e-9, 0.5): an impossible call (g = 2 where pi = 0) costs -4 ln eps, finite.  scratch:
 * nadm_cv_deviance_scratch_floats(b, M) floats (grows with b and with M).  xp, Q, P, scratch 16-byte, dev 8-byte, nheld 4-byte
 * aligned; ld as above.
 * The sum runs in log2 units: s_ij = (g log2 r + (2 - g) log2 u) + 2 [g == 1] in fp32 with the hardware's 1-ulp v_log_f32 (a
 * heterozygote at pi = 1/2 gives exactly 0), and dev_j = 2 ln 2 (0 - sum s) with the factor applied once, in float64.  A missing
 * call, a call of another fold, a row >= b and a SNP >= M enter both sums as exactly +0.0f / 0 (the result does not depend on the
 * pad bits of a row's last byte, nor on P at a SNP nobody observes); a SNP without a held-out call gives dev = +0.0, nheld = 0.
 * The batch's 64-sample tiles are cut into nadm_cv_deviance_slices(b, M) slices of whole tiles (the rule of nadm_snp_hwe_slices;
 * never more than 4096 samples in one slice): s is an fp32 sum within a slice in sample order, the slices' partials are added in
 * float64 in slice order; nheld is an integer sum, exact.  The order depends on (b, M) alone and there are no floating-point
 * atomics: the same inputs give the same bits.  Every refusal of both entries is reported before anything is launched.
 * Asynchronous on `stream`. */
#define NADM_CV_MAX_FOLDS 64
int nadm_cv_mask(const uint8_t* xp, int64_t ld, int64_t rows, int64_t row0, int64_t M,
                 uint64_t seed, int32_t folds, int32_t fold, uint8_t* xo, void* stream);
int32_t nadm_cv_deviance_slices(int32_t b, int64_t M);
int64_t nadm_cv_deviance_scratch_floats(int32_t b, int64_t M);
int nadm_cv_deviance(const uint8_t* xp, int64_t ld, int32_t b, int64_t row0, int64_t M,
                     const float* Q, int32_t q_stride, int32_t k, int32_t kp, const float* P, float eps,
                     uint64_t seed, int32_t folds, int32_t fold,
                     double* dev, int32_t* nheld, float* scratch, void* stream);

/* ---- Standard errors of P: the per-SNP Fisher information of a SNP's frequency row GIVEN the ancestry fractions ------------------
 * The sampling error of p_jk comes from the sample axis: from how many allele copies of ancestry k were observed at SNP j.  One
 * call = the rows idx[0..b) (idx == NULL: rows 0..b; any order, a duplicate counts as often as it occurs), Q [b, k] (row s belongs
 * to idx[s], row stride q_stride, a multiple of 4, >= kp, pad cols 0) and ONE head P [M, kp] (kp = nadm_pad_k(k), pad cols 0).
 * Codes g in {0, 1, 2} are observed, 3 is missing:
 *     pi_ij  = sum_k q_ik p_jk                                      (fp32, fused multiply-adds, k in order, as nadm_snp_hwe)
 *     m_ij   = 1 if the call is observed and j < M, else 0
 *     r = clip(pi, eps, 1 - eps);   u = clip(1 - pi, eps, 1 - eps)  (u from the UNCLIPPED pi, as nadm_project_p)
 *     w_ij   = m_ij 2 / (r u)                                       (the Fisher information of pi in one binomial(2, pi) call)
 *     I_j[a][c] = sum_i w_ij q_ia q_ic   for a <= c < k             n_j = sum_i m_ij
 * This is the EXPECTED information of the row p_j., not the observed one (weight g / pi^2 + (2 - g) / (1 - pi)^2): its weight does
 * not depend on the call's value -- replacing observed codes by other observed codes leaves every output bit unchanged -- and it is
 * bounded by 2 / eps where the observed weight reaches 1 / eps^2, which an fp32 running sum needs; the two calibrate alike (DESIGN.md
 * 4.14).  The caller inverts I_j over the SNP's free components in float64: SE_jk = sqrt((I_j^-1)_kk), CONDITIONAL on Q.
 * info double [M, k (k + 1) / 2]: the pairs a <= c of the real columns, a-major ((0,0), (0,1), .., (0,k-1), (1,1), ..); nobs int32
 * [M].  k <= 16 (kp in {4, 8, 12, 16}): the kp (kp + 1) / 2 running sums of a SNP live in one thread's registers; a wider head is
 * refused.  eps in [1e-9, 0.5).  scratch: nadm_snp_info_scratch_floats(b, M, kp) floats (grows with b, with M and with kp; 0 for a
 * kp without a kernel).  xp, Q, P, scratch 16-byte, info 8-byte, nobs, idx 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32.
 * A missing call, a row past the list and a SNP >= M enter every sum as exactly +0.0f / 0 (the result does not depend on the pad
 * bits of a row's last byte, nor on P at a SNP nobody observes -- a NaN there included); an entry whose every term is 0 comes out as
 * +0.0.  1 / (r u) is one multiplication and the hardware's 1-ulp reciprocal; w q_a is rounded once, then fused multiply-adds.  The
 * batch's 64-sample tiles are cut into nadm_snp_info_slices(b, M) slices of whole tiles (the rule of nadm_snp_hwe_slices; never more
 * than 4096 samples in one slice): the sums are fp32 within a slice in sample order, the slices' partials are added in float64 in
 * slice order and the factor 2 is applied once, there (exact); n is an integer sum, exact.  The order depends on (b, M) alone and
 * there are no floating-point atomics: the same inputs give the same bits.  Every refusal -- a null pointer, an empty block, ld, k
 * and kp, q_stride, eps, k > 16, alignment -- is reported before anything is launched.  Asynchronous on `stream`.
 *
 * nadm_snp_info_se: the float64 inverse, one thread per SNP.  info [M, k (k + 1) / 2] and nobs [M] as nadm_snp_info writes them, drop
 * uint8 [M, k] (nonzero: the component is not free -- fixed at the boundary or unseen; the caller's rule), se double [M, k] out, all
 * on the device.  The rows and columns of a SNP's dropped components are replaced by those of the identity, the block is factored
 * as L L^T (a pivot s is accepted if s > 0, as LAPACK's potrf does) and (I^-1)_cc = |L^-1 e_c|^2 comes from one forward substitution
 * per column; se_jc = sqrt of it.  NaN: a dropped component; every entry of a SNP with nobs = 0 or with a pivot that is not > 0
 * (the free block is not positive definite in float64).  Plain IEEE float64 arithmetic in a fixed order: the same inputs give the
 * same bits.  1 <= k <= 16; info, se 8-byte, nobs 4-byte aligned; refusals are reported before the launch. */
int32_t nadm_snp_info_slices(int32_t b, int64_t M);
int64_t nadm_snp_info_scratch_floats(int32_t b, int64_t M, int32_t kp);
int nadm_snp_info(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                  const float* Q, int32_t q_stride, int32_t k, int32_t kp, const float* P,
                  float eps, double* info, int32_t* nobs, float* scratch, void* stream);
int nadm_snp_info_se(const double* info, const uint8_t* drop, const int32_t* nobs, int64_t M, int32_t k, double* se, void* stream);

/* ---- Standard errors of Q given P: the per-SAMPLE Fisher information of a sample's row of ancestry fractions GIVEN the frequencies -
 * The mirror image of nadm_snp_info: how sure is a sample's q_i. when P is held fixed -- a projected sample (nadm_project_q), whose
 * error comes from the SNP axis: from how many of its calls were observed and how far apart the columns of P are there.  One call
 * = the rows idx[0..b) (idx == NULL: rows 0..b; any order, a duplicate is a sample of its own), ONE head P [M, kp] (kp =
 * nadm_pad_k(k), pad cols 0) and Q [b, k] (row s belongs to idx[s], row stride q_stride, a multiple of 4, >= kp, pad cols 0).
 * Codes g in {0, 1, 2} are observed, 3 is missing:
 *     pi_ij  = sum_k q_ik p_jk                                      (fp32, fused multiply-adds, k in order, as nadm_project_q)
 *     o_ij   = 1 if the call is observed and j < M, else 0
 *     r = clip(pi, eps, 1 - eps);   u = clip(1 - pi, eps, 1 - eps)  (u from the UNCLIPPED pi, as nadm_project_p)
 *     w_ij   = o_ij 2 / (r u)                                       (the Fisher information of pi in one binomial(2, pi) call)
 *     A_i[a][c] = sum_j w_ij p_ja p_jc   for a <= c < k             n_i = sum_j o_ij
 * The EXPECTED information of the row q_i., for the reasons given at nadm_snp_info: the weight does not depend on the call's value
 * and is bounded by 2 / eps.  The caller inverts A_i under the constraint sum_k q_ik = 1 in float64 (neural_admixture_amd/qse.py):
 * the result is CONDITIONAL on P.  info double [b, k (k + 1) / 2]: the pairs a <= c of the real columns, a-major ((0,0), (0,1), ..,
 * (0,k-1), (1,1), ..); nobs int32 [b].  k <= 16 (kp in {4, 8, 12, 16}): the kp (kp + 1) / 2 running sums of a sample live in one
 * thread's registers; a wider head is refused.  eps in [1e-9, 0.5).  scratch: nadm_sample_info_scratch_floats(b, M, kp) floats (grows
 * with b, with M and with kp; 0 for a kp without a kernel).  xp, P, Q, scratch 16-byte, info 8-byte, nobs, idx 4-byte aligned; ld >=
 * ceil(M/4), ld % 16 == 0, ld < 2^32; the address of row r is r * ld in 64 bits.
 * A missing call, a row past the list and a SNP >= M enter every sum as exactly +0.0f / 0: the result does not depend on the pad
 * bits of a row's last byte, nor on the values of P at the SNPs where the sample's call is missing (P must be finite: a masked term
 * is still multiplied by that 0); a sample without an observed call gets n = 0 and +0.0 throughout.  1 / (r u) is one multiplication
 * and the hardware's 1-ulp reciprocal; w p_a is rounded once, then fused multiply-adds.  The 256-SNP chunks are cut into
 * nadm_sample_info_ranges(b, M) contiguous ranges (more than one while the block's 256-sample tiles alone do not fill the chip); a
 * lane's fp32 running sums cover one range in SNP order and never more than 2^18 SNPs (1024 chunks, as nadm_kinship and
 * nadm_obs_project: 2^18 terms of one sign lose at most 2^18 x 2^-24 = 1.6 % in the worst case and about sqrt(2^18) x 2^-24 = 3e-5
 * where the roundings do not line up); the ranges' partials are added in float64 in range order and the factor 2 is applied once, there (exact); n is an
 * integer sum, exact.  The order depends on (b, M) alone and there are no floating-point atomics: the same inputs give the same
 * bits.  Every refusal -- a null pointer, an empty batch, ld, k and kp, q_stride, eps, k > 16, alignment -- is reported before
 * anything is launched.  Asynchronous on `stream`. */
int32_t nadm_sample_info_ranges(int32_t b, int64_t M);
int64_t nadm_sample_info_scratch_floats(int32_t b, int64_t M, int32_t kp);
int nadm_sample_info(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                     const float* P, int32_t k, int32_t kp, const float* Q, int32_t q_stride,
                     float eps, double* info, int32_t* nobs, float* scratch, void* stream);

/* ---- Local ancestry: the linkage model's forward-backward recursion along the genome ------------------------------------------------
 * Which stretches of a sample's genome come from which component.  The linkage model of STRUCTURE (Falush, Stephens & Pritchard
 * 2003), unphased as in ancestry_HMM (Corbett-Detig & Nielsen 2017): each of a sample's two haplotypes carries an ancestry, redrawn
 * from the sample's q_i. with probability rho[j] between SNP j - 1 and j (the caller's 1 - exp(-n d): n generations, d Morgans,
 * ONE rate for all components), and the call is emitted from the two ancestries' frequencies.  The hidden state is the unordered
 * pair of ancestries: K (K + 1) / 2 states per sample, a dependent step per SNP, N M K^2 work.
 * Rows, idx, P [M, kp], Q [b, k], q_stride, eps, the alignment and the ld rules are those of nadm_sample_info.  A segment s is the SNP
 * range [seg[s], seg[s + 1]) (normally one chromosome); segments are independent and their bounds need not be multiples of 4 or 256;
 * an empty one has ll = 0.  rho float [M] in [0, 1]; rho at a segment's first SNP is ignored (a restart).  out_snp int32 [n_out]
 * strictly ascending: the SNPs at which the posterior is wanted; oseg int32 [n_seg + 1]: segment s owns out_snp[oseg[s] .. oseg[s + 1]),
 * each inside the segment.  seg, oseg and out_snp live on the device and CANNOT be checked here: the caller validates them on the host
 * before the upload (neural_admixture_amd/localanc.py: seg ascending within 0..M, out_snp strictly ascending, every slice inside its
 * segment, oseg ascending from 0 to n_out); a slice that leaves 0..n_out is cut to it, so nothing is written outside the buffers.
 * Per SNP j, all fp32, the symmetric a(x, y) held as its upper triangle x <= y < kp, a-major:
 *     p_x = clip(P[j,x], eps, 1 - eps);   c_x = clip(1 - P[j,x], eps, 1 - eps)      (c from the UNCLIPPED value, as nadm_project_p)
 *     e(x,y) = fma(u_x, v_y, u_y w_x):  code 0: c_x c_y;  code 1: fma(p_x, c_y, p_y c_x);  code 2: p_x p_y;  missing, j >= M: exactly 1
 *     s = 1 - rho;  c0 = s s;  c1 = rho s;  c2 = rho rho              (a segment's first SNP: rho = 1 and a^ = 0, so pr = q_x q_y exactly)
 *   forward, j ascending:
 *     G_x = fma(c1, R_x, (c2 / 2) q_x);   pr(x,y) = fma(c0, a^(x,y), fma(q_y, G_x, q_x G_y))    (= c0 a^ + c1 (q_y R_x + q_x R_y) + c2 q_x q_y)
 *     a = pr e;   R'_x = sum_y a(x,y), y ascending;   S = sum_x R'_x, x ascending (the sum over ORDERED pairs);
 *     a^ = a rcp(S);   R_x = R'_x rcp(S);   ll += ln S;   at an output point a^ goes to the checkpoints
 *   backward, j descending from the segment's last SNP, where b^ = sup, sup(x,y) = 1 where q_x q_y > 0, else 0:
 *     at an output point  g = a^ b^;  D_x = sum_y g(x,y), y ascending;  Z = sum_x D_x;  dosage_x = min(2 (D_x rcp(Z)), 2);
 *         the mass of the unordered pair is g(x,x) or 2 g(x,y); call = the a-major index over x <= y < k of the largest mass
 *         (strictly: the lowest index wins a tie), post = that mass times rcp(Z)
 *     from j to j - 1:  h = b^ e_j;  H_x = sum_y q_y h(x,y) (multiply-adds, y ascending);  Tt = sum_x q_x H_x;
 *         J_x = fma(c1, H_x, (c2 / 2) Tt);  b(x,y) = sup (fma(c0, h, J_x + J_y)) with rho[j]    (= sup (c0 h + c1 (H_x + H_y) + c2 Tt));
 *         b^ = b rcp(diagonal sum + 2 x upper sum, each a-major)
 * The sup mask is part of the contract: without it a sample whose q has exact zeros and whose calls disagree with it over a long
 * stretch underflows the supported states against the unsupported ones and ends in 0 / 0.  Where Z is 0 or not finite the point's
 * dosage and post are NaN and call is 255; nothing is clipped silently.  rcp is the hardware's 1-ulp reciprocal; ln S is log2 S
 * (v_log_f32) summed in fp32 within a 256-SNP chunk of the matrix, times ln 2 and summed in float64 across chunks.  The recursion
 * forgets: the rounding error does not grow with the chain.
 * Outputs: dosage float [b, n_out, kp] in [0, 2] (pad columns +0.0), call uint8 [b, n_out], post float [b, n_out], ll double
 * [b, n_seg] (the segment's log-likelihood of the sample's calls).  dosage == NULL runs the forward pass only (n_out may be 0; call,
 * post, out_snp, oseg and scratch are not touched): the scan over the number of generations.  scratch:
 * nadm_local_anc_scratch_floats(b, n_out, kp) floats, the checkpoints [n_out][kp (kp + 1) / 2][256 ceil(b / 256)] (0 for a kp without
 * a kernel); the caller blocks its rows to bound it.  k <= 16 (kp in {4, 8, 12, 16}): the states of a sample live in one thread's
 * registers; a wider head is refused.  Two launches, one 256-thread block per (256-sample tile, segment), no atomics: a sample's
 * outputs depend on its own row, q, P, rho and the segment alone -- not on its position in the batch, the other rows or the other
 * segments -- and the same inputs give the same bits.  Every refusal -- a null pointer, an empty batch, M >= 2^31, ld, k and kp,
 * q_stride, eps, k > 16, n_seg < 1, n_out < 0, alignment (dosage and scratch 16-byte, ll 8-byte, the others 4-byte), too many blocks
 * -- is reported before anything is launched.  Asynchronous on `stream`.  Not built: phased input, per-component rates, Viterbi paths. */
int64_t nadm_local_anc_scratch_floats(int32_t b, int64_t n_out, int32_t kp);
int nadm_local_anc(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                   const float* P, int32_t k, int32_t kp, const float* Q, int32_t q_stride, float eps,
                   const float* rho, const int32_t* seg, int32_t n_seg,
                   const int32_t* out_snp, const int32_t* oseg, int64_t n_out,
                   float* dosage, uint8_t* call, float* post, double* ll, float* scratch, void* stream);

/* ---- Model-fit check: the pairwise correlation of leave-one-out residuals (evalAdmix, Garcia-Erill & Albrechtsen 2020) -----------
 * Does the model describe these samples, and if not, which ones?  Under a good fit the residuals g - 2 pi of two samples are
 * uncorrelated; where the model is wrong the correlation is positive inside the groups it merged or mis-modelled and negative
 * between them.  A sample's own genotype sits in the frequencies its residual is taken against, which biases a pair inside a group of
 * n unadmixed samples by about -1/n; the correction refits the frequencies WITHOUT one sample of the pair -- one EM step of P from
 * the sums nadm_project_p forms -- and takes BOTH residuals against that refit.
 *
 * nadm_em_sums: the sums themselves, in nadm_project_p's notation and with its arguments: for the rows idx[0..b) (idx == NULL: rows
 * 0..b; a duplicate counts as often as it occurs), Q [b, k] and ONE head P [M, kp],
 *     B_jk = sum over observed i of q_ik g_ij / r_ij          C_jk = sum over observed i of q_ik (2 - g_ij) / u_ij
 * written as float [M, kp] each (pad columns 0; rows >= M are never written); nobs_snp int32 [M] may be NULL.  The accumulation is
 * nadm_project_p's own (one body, csrc/nadm_em_accum.h): fp32 within each of nadm_em_sums_slices(b, M) slices of whole 64-sample
 * tiles in sample order, the slices' partials added in float64 in slice order and rounded to fp32 ONCE.  Each term is
 * fma(q_ik, t, sum) with t1 = g * rcp(r), t0 = (2 - g) * rcp(u) (the hardware's 1-ulp reciprocal); a missing call and a SNP >= M
 * enter as exactly +0.0f.  scratch: nadm_em_sums_scratch_floats(b, M, kp) floats.  xp, Q, P, B, C, scratch 16-byte aligned.
 *
 * nadm_resid_cor: one block of ORDERED pairs, the rows idxA[0..ba) against the LEFT-OUT rows idxB[0..bb) (idx == NULL: rows 0..b; any
 * order, duplicates allowed, the lists may overlap or be the same), QA [ba, k] / QB [bb, k] as in nadm_kinship, ONE head P [M, kp],
 * and B, C float [M, kp] as nadm_em_sums wrote them over ALL rows of the fit (the rows of idxB among them).  For a left-out sample
 * b observed at SNP j (t1, t0 of b's own call as above: its terms as they entered the sums), all in fp32, every operation rounded
 * on its own (no contraction) unless written fma:
 *     beta_k = q_bk * t1                 gamma_k = q_bk * t0
 *     num'   = p_jk * max(B_jk - beta_k, 0)
 *     den'   = num' + (1 - p_jk) * max(C_jk - gamma_k, 0)
 *     den    = p_jk * B_jk + (1 - p_jk) * C_jk
 *     f_jk   = num' / den'  (IEEE division)  if den' >= NADM_LOO_MIN_SHARE * den and den > 0 and den' > 0,   else p_jk
 * one EM step of P without sample b.  The fallback covers a frequency whose information is mostly b's own (a component that b alone
 * carries: B - beta = 0): without it the quotient loses all its digits.  NADM_LOO_MIN_SHARE = 1/8 is a design constant, not a
 * measurement; the three comparisons above, on those fp32 values, decide the branch (den' > 0 differs from the first only where
 * den / 8 underflows; a NaN compares false and keeps p).  Where b is missing at j, beta = gamma = 0 and nothing of the SNP enters
 * the pair.  Then for every sample a of the block (a = b included), o = 1 where the call is observed and j < M, else 0:
 *     pi_aj = sum_k q_ak f_jk   (fused multiply-adds, k in order)        d_aj = o_aj fma(-2, pi_aj, g_aj)
 *     S_ab  = sum_j d_aj d_bj     Ta_ab = sum_j d_aj^2 o_bj     Tb_ab = sum_j d_bj^2 o_aj     n_ab = sum_j o_aj o_bj
 * S, Ta, Tb double [ba, bb], n int32 [ba, bb] (may be NULL), row-major.  The caller forms c_ab = S / sqrt(Ta Tb) (none where Ta Tb
 * = 0) and symmetrises (c_ab + c_ba) / 2: c_ab and c_ba are different computations.  ba, bb in 1..NADM_RESID_COR_MAX_ROWS; k <= 16
 * (kp in {4, 8, 12, 16}), a wider head is refused; eps in [1e-9, 0.5).  scratch: nadm_resid_cor_scratch_floats(ba, bb, M, kp)
 * floats, bounded by ranges x ba x bb (padded to tiles), never per chunk.  xp, P, QA, QB, B, C, scratch 16-byte, S, Ta, Tb 8-byte,
 * n, idxA, idxB 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32.
 * A missing call and a SNP >= M enter every sum as exactly +0.0f (the result does not depend on the pad bits of a row's last
 * byte, nor on P at a SNP nobody observes); n is exact.  The 256-SNP chunks are cut into nadm_resid_cor_ranges(ba, bb, M, kp)
 * contiguous ranges (more than one while the block's tiles alone do not fill the chip); a lane's fp32 running sums cover one
 * range in SNP order and never more than 2^18 SNPs; the ranges' partials are added in float64 in range order.  The order depends
 * on (ba, bb, M, kp) alone and there are no floating-point atomics: the same inputs give the same bits.  Every refusal is reported
 * before anything is launched.  Asynchronous on `stream`. */
#define NADM_RESID_COR_MAX_ROWS 4096
#define NADM_LOO_MIN_SHARE 0.125f   /* the refit without b is used while it keeps at least this share of the SNP-component's den */
int32_t nadm_em_sums_slices(int32_t b, int64_t M);
int64_t nadm_em_sums_scratch_floats(int32_t b, int64_t M, int32_t kp);
int nadm_em_sums(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                 const float* Q, int32_t q_stride, int32_t k, int32_t kp, const float* P,
                 float eps, float* B, float* C, int32_t* nobs_snp, float* scratch, void* stream);
int32_t nadm_resid_cor_ranges(int32_t ba, int32_t bb, int64_t M, int32_t kp);
int64_t nadm_resid_cor_scratch_floats(int32_t ba, int32_t bb, int64_t M, int32_t kp);
int nadm_resid_cor(const uint8_t* xp, int64_t ld, const int32_t* idxA, int32_t ba, const int32_t* idxB, int32_t bb, int64_t M,
                   const float* P, int32_t k, int32_t kp, const float* QA, const float* QB, int32_t q_stride,
                   const float* B, const float* C, float eps, double* S, double* Ta, double* Tb, int32_t* nobs,
                   float* scratch, void* stream);

/* ---- the observed-calls pair products: what a centred, scaled, missing-aware PCA of the packed matrix is made of ----------------
 * nadm_pca_project* restate the reference's initialisation (raw codes, missing = 3, no centring); a PCA anyone would plot
 * (smartpca, plink --pca, FastPCA) standardises each SNP and leaves a missing call at the mean.  That product cannot be had from
 * them by algebra: it needs the product with the observation indicator as well.  One call = the rows idx[0..b) (idx == NULL: rows
 * 0..b; any order, a duplicate counts as often as it occurs).  Codes g in {0, 1, 2} are observed, 3 is missing; o_sj = 1 where the
 * call is observed and j < M, else 0:
 *     nadm_obs_project     Y[s, c]  = sum_j (g o)_sj W1[j, c] + o_sj W2[j, c]                      Y  float [b, CP]
 *     nadm_obs_project_t   O1[j, c] = sum_s (g o)_sj Yin[s, c]      O2[j, c] = sum_s o_sj Yin[s, c]        O1, O2 float [M, CP]
 * W1, W2 float [M, CP], Yin float [b, CP] (row s belongs to idx[s]).  C in 1..CP columns are in use, CP in {16, 32} is the column
 * stride; pad columns are zero on input and are written as zero.  The centring and scaling are the caller's: W1 = s o W and
 * W2 = -c o s o W give sum_j o (g - c_j) s_j W_j, and s_j (O1_j - c_j O2_j) is the transposed product (neural_admixture_amd/pca.py).
 * b in 1..NADM_OBS_MAX_ROWS.  scratch: nadm_obs_project_scratch_floats(b, M, CP) / nadm_obs_project_t_scratch_floats(b, M, CP)
 * floats (both grow with b and M).  xp, W1, W2, Yin, Y, O1, O2, scratch 16-byte, idx 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0,
 * ld < 2^32; the address of row r is r * ld in 64 bits.
 * Arithmetic: g o in {0, 1, 2} and o in {0, 1} are exact in one bf16 piece; an fp32 operand value is cut into three
 * round-to-nearest bf16 pieces (exact: 3 x 8 significand bits) and multiplied on the matrix pipe (v_mfma_f32_16x16x32_bf16), lo, mid,
 * hi piece in that order, every product exact, the sums fp32.  Forward: the 256-SNP chunks are cut into nadm_obs_project_ranges(b, M)
 * contiguous ranges of nadm_obs_project_chunks(b, M) chunks (more than one range while the 256-sample tiles of the block alone do
 * not fill the chip); both terms of a SNP go into ONE fp32 accumulator, which never covers more than 2^18 SNPs.  Transposed: the
 * batch's 64-sample tiles are cut into nadm_obs_project_t_slices(b, M) slices of whole tiles -- the rule of nadm_snp_hwe_slices:
 * never more than 4096 samples in one fp32 accumulator.  The ranges' / slices' partials are added in float64 in range / slice
 * order and rounded to fp32 once.  The order depends on (b, M, CP) alone and there are no floating-point atomics: the same inputs
 * give the same bits.
 * A missing call, a SNP >= M, a row past the list, the pad bits of a row's last byte and the bytes behind it enter every sum as
 * exactly +0.0f: an all-missing row gives a Y row of +0.0, and rows >= M of W1 / W2 are never read.  (Where a call is missing the
 * operand value is still multiplied by that 0: operands must be finite.)
 * Every refusal -- a null pointer, an empty block, ld, C / CP, alignment, b -- is reported before anything is launched. */
#define NADM_OBS_MAX_ROWS (1 << 24)
int32_t nadm_obs_project_chunks(int32_t b, int64_t M);
int32_t nadm_obs_project_ranges(int32_t b, int64_t M);
int64_t nadm_obs_project_scratch_floats(int32_t b, int64_t M, int32_t CP);
int nadm_obs_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* W1, const float* W2,
                     int32_t C, int32_t CP, float* Y, float* scratch, void* stream);
int32_t nadm_obs_project_t_slices(int32_t b, int64_t M);
int64_t nadm_obs_project_t_scratch_floats(int32_t b, int64_t M, int32_t CP);
int nadm_obs_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M, const float* Yin, int32_t C,
                       int32_t CP, float* O1, float* O2, float* scratch, void* stream);

/* ---- Residual PCA given Q and P: the two products of the model's standardised (Pearson) residuals ---------------------------------
 * What structure is left in the data once the K components are taken out, and which samples carry it?  nadm_resid_cor answers for
 * pairs at O(N^2 M K); the principal components of the standardised residuals answer at O(N M (K + columns)) per product.  One call
 * = the rows idx[0..b) (idx == NULL: rows 0..b; any order, a duplicate counts as often as it occurs), Q [b, k] (row s belongs to
 * idx[s], row stride q_stride, a multiple of 4, >= kp, pad cols 0) and ONE head P [M, kp] (kp = nadm_pad_k(k), pad cols 0).  Codes
 * g in {0, 1, 2} are observed, 3 is missing.  Per call, in fp32:
 *     pi_ij  = sum_k q_ik p_jk                                      (fused multiply-adds, k in order, as nadm_snp_hwe)
 *     m_ij   = 1 if the call is observed, j < M and pimin <= pi_ij <= 1 - pimin (1 - pimin rounded to fp32), else 0
 *     r = clip(pi, eps, 1 - eps);   u = clip(1 - pi, eps, 1 - eps)  (u from the UNCLIPPED pi, as nadm_snp_hwe)
 *     a_ij   = m_ij (g_ij - 2 pi_ij) / sqrt(2 r u)                  (mean 0 and variance 1 under the model)
 *     nadm_resid_project     Y[i, c] = sum_j a_ij W[j, c]      ss_i = sum_j a_ij^2      nobs_i = sum_j m_ij
 *     nadm_resid_project_t   O[j, c] = sum_i a_ij Yin[i, c]                             nobs_snp_j = sum_i m_ij
 * W float [M, CP], Y float [b, CP], Yin float [b, CP] (row s belongs to idx[s]), O float [M, CP]; ss double [b], nobs int32 [b],
 * nobs_snp int32 [M].  C in 1..CP columns are in use, CP in {16, 32} is the column stride; pad columns are written as +0.0
 * (nadm_obs_project's contract: the subspace iteration of neural_admixture_amd/pca.py runs on either pair).  The scale depends on
 * sample and SNP jointly, so no operand of nadm_obs_project carries it.  k <= 16 (kp in {4, 8, 12, 16}); eps in [1e-9, 0.5), pimin in
 * [0, 0.5).  scratch: nadm_resid_project_scratch_floats(b, M, CP) / nadm_resid_project_t_scratch_floats(b, M, kp, CP) floats (both
 * grow with b and with M; 0 for a width without a kernel).  xp, P, Q, W, Yin, Y, O, scratch 16-byte, ss 8-byte, nobs, nobs_snp, idx
 * 4-byte aligned; ld >= ceil(M/4), ld % 16 == 0, ld < 2^32; the address of row r is r * ld in 64 bits.
 * Arithmetic: g - 2 pi is ONE fused multiply-add fma(-2, pi, g); the scale is the hardware's 1-ulp reciprocal square root of
 * (r + r) u; their product is rounded once; every column sum and ss take a by fused multiply-adds on the vector ALU (no matrix pipe,
 * no operand splitting).  A missing call, a row past the list, a SNP >= M and a masked pi give a = +0.0f exactly: the result does
 * not depend on the pad bits of a row's last byte nor on the finite values of W at SNPs where a is 0 (rows >= M of P and W are never
 * read), and an output whose every term is masked is +0.0.  Forward: the 256-SNP chunks are cut into nadm_resid_project_ranges(b, M)
 * contiguous ranges of nadm_resid_project_chunks(b, M) chunks (the plan of nadm_sample_info); a lane's fp32 column sums cover one
 * range in SNP order and never more than 2^18 SNPs; ss is an fp32 sum within a chunk and a float64 sum over chunks.  Transposed: the
 * batch's 64-sample tiles are cut into nadm_resid_project_t_slices(b, M) slices of whole tiles (the rule of nadm_snp_hwe_slices;
 * never more than 4096 samples in one fp32 sum).  The ranges' / slices' partials are added in float64 in range / slice order and
 * rounded to fp32 once; the counts are integer sums, exact.  The order depends on (b, M) alone and there are no floating-point
 * atomics: the same inputs give the same bits.  Every refusal -- a null pointer, an empty block, ld, k and kp, q_stride, eps, pimin,
 * k > 16, C / CP, alignment -- is reported before anything is launched.  Asynchronous on `stream`. */
int32_t nadm_resid_project_chunks(int32_t b, int64_t M);
int32_t nadm_resid_project_ranges(int32_t b, int64_t M);
int64_t nadm_resid_project_scratch_floats(int32_t b, int64_t M, int32_t CP);
int nadm_resid_project(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                       const float* P, int32_t k, int32_t kp, const float* Q, int32_t q_stride, float eps, float pimin,
                       const float* W, int32_t C, int32_t CP, float* Y, double* ss, int32_t* nobs, float* scratch, void* stream);
int32_t nadm_resid_project_t_slices(int32_t b, int64_t M);
int64_t nadm_resid_project_t_scratch_floats(int32_t b, int64_t M, int32_t kp, int32_t CP);
int nadm_resid_project_t(const uint8_t* xp, int64_t ld, const int32_t* idx, int32_t b, int64_t M,
                         const float* P, int32_t k, int32_t kp, const float* Q, int32_t q_stride, float eps, float pimin,
                         const float* Yin, int32_t C, int32_t CP, float* O, int32_t* nobs_snp, float* scratch, void* stream);

/* ---- 8(f)-3: decoder init, the means of the mixture the reference fits in the PCA subspace (model/train.py:61-66, scikit-learn's
 * GaussianMixture(n_components=K, n_init=5, init_params='k-means++', tol=1e-4, covariance_type='full', max_iter=100,
 * random_state=seed).fit(X).means_): the EM iterations of that call in float64 on the host (csrc/nadm_gmm.cpp restates the
 * algorithm and the library's conventions).  X [N, d] row-major; picks [n_init, K] = the k-means++ seed rows of every restart,
 * drawn by the caller from the library's own random stream (gmm.kmeanspp_picks); means [K, d] out; lower_bound / n_iter (may be
 * NULL) = the winning restart's objective and iteration count.  Host code, one thread per restart, synchronous. */
int nadm_gmm_fit_means(const double* X, int64_t N, int32_t d, int32_t K, const int32_t* picks, int32_t n_init, double tol,
                       int32_t max_iter, double reg_covar, double* means, double* lower_bound, int32_t* n_iter);
/* The same fit with the sums over the samples on the device (csrc/nadm_gmm_dev.hip: the restarts side by side in one grid, five small
 * launches per EM iteration, float64, fixed summation order): for inputs where the host form is a visible part of a run (0.77 s at
 * N = 100k, here ~0.03 s).  d == 8 (the reference's --pca_components default) and K <= 16 only.  X, picks, means are HOST pointers
 * like above (X is uploaded: 64 B per sample); synchronous; work is queued on `stream`.  Equal to the host form up to the order of
 * the sums (means to ~1e-12). */
int nadm_gmm_fit_means_dev(const double* X, int64_t N, int32_t d, int32_t K, const int32_t* picks, int32_t n_init, double tol,
                           int32_t max_iter, double reg_covar, double* means, double* lower_bound, int32_t* n_iter, void* stream);

/* ---- VCF genotypes (src/snp_reader.py:73-87: scikit-allel read_vcf, calldata/GT as int8 with -1 fills, summed over the two
 * alleles, negative sums -> 3).  buf = the whole decompressed file; out == NULL only counts samples and variant lines;
 * out = uint8 [n_samples, n_variants], sample-major like the reference's matrix.  Host code (threads), no GPU. */
int nadm_vcf_parse_gt(const char* buf, int64_t len, int64_t* n_samples, int64_t* n_variants, uint8_t* out);

/* ---- 8(f)-4: ADMIXTURE-compatible text output ------------------------------------------------------------
 * np.savetxt(path, A, delimiter=' ') for a float32 host matrix, byte for byte ('%.18e' of the value widened to
 * double, src/utils.py:56-66); multi-threaded.  a [rows, cols] with row stride row_stride (elements). */
int nadm_savetxt_f32(const char* path, const float* a, int64_t rows, int64_t cols, int64_t row_stride);

/* ---- measurement helpers ------------------------------------------------------------------ */
/* Synthetic admixture-model genotypes written directly as packed bytes:
 * G ~ Binomial(2, Qt.F), `missing` fraction set to 3.  Qt [rows,K], Fq [K,M] float32 on device;
 * counter-based RNG keyed by (seed, row0 + r, SNP) so shards generated on different ranks agree. */
int nadm_synth_packed(uint8_t* xp, int64_t rows, int64_t row0, int64_t M, int64_t ld,
                      const float* Qt, const float* Fq, int32_t K, float missing, uint64_t seed, void* stream);

/* Box fingerprint (bench.py "box"; csrc/nadm_calib.hip): a fixed stream of packed-f32 VALU chains + bf16 matrix instructions, three
 * waves per SIMD on every CU, `iters` rounds.  Block i writes out[2i] = shader cycles (s_memtime) and out[2i+1] = constant-rate ticks
 * (s_memrealtime, nadm_wall_clock_khz) it took: cycles / ticks x rate = the shader clock the box sustains under an issue-bound load.
 * Returns the number of reporting blocks (<= max_blocks), or a negative status.  `sink`: one float, never written. */
/* Measurement only: with a non-NULL device pointer every following S = 1 launch of the matrix-core pass 2 has the block in the middle of its
 * grid write out2[0] = shader cycles (s_memtime) and out2[1] = constant-rate ticks (s_memrealtime) it took: the clock the DOMINANT kernel
 * itself ran at in this run.  NULL switches it off.  Process-wide (one process per GPU); a few scalar instructions in one block. */
void nadm_clock_probe(uint64_t* out2_dev);
int nadm_calib_clock(int32_t iters, uint64_t* out /* device [2 * max_blocks] */, int32_t max_blocks, float* sink, void* stream);
int64_t nadm_wall_clock_khz(void);

#ifdef __cplusplus
}
#endif
#endif /* NADM_H */
