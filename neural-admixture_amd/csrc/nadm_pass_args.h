// What the host side and the kernel units of the genotype passes and the MLP pair share: the shape constants the host rules need, and one
// plain struct per launch -- what the caller passed plus what the host side decided (nadm_passes_host.cpp), handed to the unit that holds
// the kernels (launch_pass1 .. launch_mlp_bwd).  Plain C++, no HIP header, like nadm_err.h: the host unit builds with any C++ compiler.
// (The constexpr functions carry no __host__ __device__: in the kernel units a constexpr function is callable from both sides as it is.)
#pragma once
#include <stdint.h>
#include "../../include/nadm.h"

namespace nadm {

// ---- pass 1, the matrix-core kernel (encode_fwd_mfma_kernel): 8 waves x 256 SNPs = the 2048-SNP chunk both pass-1 kernels write
constexpr int EM_WAVES = 8;
constexpr int EM_SLICE = 256;                         // SNPs per wave
constexpr int EM_CHUNK_SNPS = EM_WAVES * EM_SLICE;    // 2048
constexpr int EM_TILES_PER_BLOCK = 52;                // upper bound of 16-sample tiles per block (grid.y splits the batch)

// ---- pass 2, the bf16 matrix-core kernel (KP <= 16).  Shape tuned on MI355X with bench.py (b=800, M=500k, K=8; decode time
// with / without the loss):  8 waves x 4 tiles, occupancy 2: 435 / 373 us;  8 x 2, occ. 4: 401 / 331;  4 x 2, occ. 4:
// 400 / 334;  4 waves x 4 tiles at <= 168 VGPRs (3 blocks = 3 waves per SIMD, 42 KB LDS each): 388 / 310  <- default.
#ifndef NADM_BF_WAVES
#define NADM_BF_WAVES 4      // waves per block; chunk = WAVES * NTW * 16 SNPs
#endif
#ifndef NADM_BF_NTW
#define NADM_BF_NTW 4        // 16-SNP tiles per wave (2 or 4)
#endif
#ifndef NADM_BF_TS
#define NADM_BF_TS 64        // samples per LDS tile
#endif
constexpr int mf_waves(int kp) { return NADM_BF_WAVES; }   // waves per block
constexpr int mf_ntw(int kp) { return NADM_BF_NTW; }       // 16-SNP tiles per wave
constexpr int mf_chunk_snps(int kp) { return mf_waves(kp) * 16 * mf_ntw(kp); }
// floats one (sample slice, SNP chunk) block of pass 2 parks for the block that adds the slices up: the chunk's [SNPs x KP] partial of dP +
// its loss partial (+ 3 pad)
constexpr int p2_slab_floats(int kp) { return NADM_BF_WAVES * 16 * NADM_BF_NTW * kp + 4; }
// SNPs per lane in the VALU pass 2 as a function of the padded head width (register budget ~128)
constexpr int dec_spl(int kp) { return kp <= 8 ? 8 : (kp <= 16 ? 4 : (kp <= 32 ? 2 : 1)); }
// the batch copy pass 2 leaves for pass 3 (nadm_decode_bce_gather): byte `col` of batch row `row` lives in tile col / 128 of
// [b rows][128 bytes]
constexpr int XG_TILE_COLS = 128;
// Where a pass reads X.  Byte column c of row r lives at  base + (c / 128) * tile_stride + r * row_stride + c % 128:
//   the caller's row-major matrix   row_stride = ld,  tile_stride = 128,        raw codes (a missing call is code 3)
//   a tiled copy of `rows` rows     row_stride = 128, tile_stride = rows * 128, clean: missing calls and the bytes past SNP M are 0, the last
//                                   tile is 128 bytes wide (nadm_tile_packed: the whole matrix, rows = N; pass 2's batch copy: rows = b)
// An SNP sub-range launch advances `base` by whole tiles (x_from_snp); on a tiled source it ends on a tile boundary or at the matrix's end.
struct XSource {
    const uint8_t* base;
    int64_t row_stride, tile_stride;
    bool clean;
};
constexpr XSource x_rows(const uint8_t* xp, int64_t ld) { return XSource{xp, ld, XG_TILE_COLS, false}; }
constexpr XSource x_tiled(const uint8_t* xt, int64_t rows) { return XSource{xt, XG_TILE_COLS, rows * XG_TILE_COLS, true}; }
// the same source from SNP m0 on (m0 a multiple of 512: a whole number of tiles)
constexpr XSource x_from_snp(XSource x, int64_t m0) { return XSource{x.base + (m0 / (4 * XG_TILE_COLS)) * x.tile_stride, x.row_stride, x.tile_stride, x.clean}; }
// Q as the operand images of the bf16 pass 2 (layout: nadm_common.h)
constexpr int QI_TS = 64;                                  // samples per tile (= NADM_BF_TS of the pass-2 build)
constexpr int QI_TILE_U4 = 768;                            // uint4 per tile image in global memory (K <= 8 uses the first 640)

// ---- pass 3, the FP4 x FP6 kernel (CP <= 8)
constexpr int EB_G = 2;                   // groups of 16 byte columns (64 SNPs) per wave
constexpr int EB_COLS = 4 * EB_G * 16;    // packed byte columns per block (128)
constexpr int EB_CHUNK_SNPS = EB_COLS * 4;
// floats one (sample slice, SNP chunk) block of pass 3 parks for the block that adds the slices up: the chunk's [512 SNPs x CP] partial of dV
constexpr int p3_slab_floats(int cp) { return EB_CHUNK_SNPS * cp; }
// dZ as pass 3's operand image (layout: nadm_common.h): per tile of 128 samples 7 x 64 uint4
constexpr int DZI_TS = 128;
constexpr int DZI_TILE_U4 = 7 * 64;

// ---- sample slices of the sliced passes 2 and 3: ONE rule for the kernels and for the host code that chooses and checks n_slices ----------
// Slice s walks tiles [s tps, min(tiles, s tps + tps)), tps = ceil(tiles / n_slices).  The host refuses a count that leaves the last slice
// empty: it would never be counted and the hand-off (nadm_common.h) would never complete.
struct TileRange { int lo, hi; };
constexpr int slice_tps(int tiles, int n_slices) { return (tiles + n_slices - 1) / n_slices; }
constexpr TileRange slice_tiles(int tiles, int n_slices, int slice) {
    const int tps = slice_tps(tiles, n_slices), lo = slice * tps;
    return TileRange{lo, tiles < lo + tps ? tiles : lo + tps};
}
constexpr bool slices_leave_one_empty(int tiles, int n_slices) { return slice_tiles(tiles, n_slices, n_slices - 1).lo >= tiles; }
// the largest count <= min(s, tiles) that leaves no slice empty; 1 = unsliced
constexpr int slices_without_empty(int tiles, int s) { return s < 2 || tiles < 2 ? 1 : slice_tps(tiles, slice_tps(tiles, s < tiles ? s : tiles)); }

// ---- kernel arguments the host side fills
// the fused Adam epilogue of passes 2 and 3 (adam_element, nadm_common.h); scalars: adam_scalars (nadm_host_rules.h)
struct AdamFused {            // m == nullptr: no fused update
    float* m;
    float* v;
    float step_size, inv_bc2, grad_scale;
};
// The sum of the MLP weight-gradient partials of the PREVIOUS step + Adam on the small parameters (what nadm_small_grads does
// as a launch of its own: 4.7 us + a launch gap at the end of every step) as side blocks of pass 1: pass 1 reads none of the
// small parameters, the MLP forward behind it reads all of them.  part == nullptr: no side blocks.
struct SmallSide {
    const float* part;
    float *out, *p, *m, *v;
    int splits, n;
    float step_size, inv_bc2, grad_scale;
};

// ---- one struct per launch.  The first block of each is what the caller passed; "decided" is what the checked path of the host unit
// (pass1 .. mlp_bwd) adds before it calls the launcher.  The launchers check nothing.
struct Pass1Launch {
    XSource x; const int32_t* idx; int32_t b; int64_t M;
    const float* V; int32_t CP; float* zpart;
    int64_t total_chunks;           // > 0: the launch is one part of a pass of that many chunks (nadm_encode_fwd_part)
    uint32_t missing_bf16;          // a missing call as a bf16 pattern: 0, or 0x3FC0 = 1.5 (nadm_pca_project)
    bool medium;                    // precision "medium" (the plan's step only); decided: cleared for CP > 8
    SmallSide ss;                   // the side blocks (nadm_encode_fwd_small), Adam scalars folded in
    void* stream;
    // decided, for the matrix-core kernel (CP <= 8; the VALU kernel's grid is the launcher's own)
    int64_t chunks;                 // SNP chunks of this launch
    int gy, tpb;                    // batch splits and 16-sample tiles per block (pass1_batch_splits)
    int side_blocks;
};

struct Pass2Launch {
    XSource x; const int32_t* idx; int32_t b; int64_t M;
    float* P; int32_t kp; const float* Q; int32_t SP; float* dP; float* dqpart; float* losspart;
    int32_t with_loss;              // the caller's bit set
    uint8_t* xg; const void* qimg;
    int32_t n_slices; float* slab; int32_t* counters;
    bool medium;                    // precision "medium" (the plan's step only)
    void* stream;
    // decided
    AdamFused ad;
    bool loss, unit_p;              // the loss value is wanted; P lies in [0, 1] (the fast loss form)
    bool sliced;                    // n_slices > 1
};

struct Pass3Launch {
    XSource x; const int32_t* idx; int32_t b; int64_t M;
    const float* dZ; const void* dzimg; int32_t CP; float* V; float* dV;
    const nadm_mlp_weights_t* weights;      // the MLP weight-gradient partials as side work, or NULL
    int32_t flags; uint32_t missing_bf16;
    int32_t n_slices; float* slab; int32_t* counters;
    void* stream;
    // decided
    AdamFused ad;
    bool clean;                     // x is a tiled clean copy and a missing call is 0: the loader neither cleans nor, past the edges, masks columns
    bool gather;                    // clean: the copy's rows are the matrix's (idx selects them); false: pass 2's batch copy, rows in batch order
    bool sliced;                    // n_slices > 1
};

constexpr int MLP_JMAX = 8;     // hidden units per thread in the fast MLP kernels: JH = 4 (Hd <= 1024) or 8 (Hd <= 2048)
enum MlpForm { MLP_FAST = 0, MLP_GENERIC4 = 1, MLP_GENERIC1 = 2 };   // the fast kernels (Hd <= 2048, C <= 8); the generic one, 4 samples or 1 per block

struct MlpFwdLaunch {
    const nadm_heads_t* hd; const float* small; const float* zpart; int64_t n_chunks; int32_t b;
    float *Z, *rinv, *Zn, *H, *Q;
    bool images;                    // the form that writes pass 2's Q images (nadm_mlp_fwd_images)
    void* qimg; int64_t qimg_head_bytes;
    void* stream;
    // decided
    MlpForm form; int jh; bool c8;  // hidden units per thread (4 / 8) and "W1 rows as float4 pairs", for the fast kernels
};

struct MlpBwdLaunch {
    const nadm_heads_t* hd; const float* small; float* dqpart; int64_t M; int32_t b;
    const float *Z, *rinv, *Zn, *H, *Q;
    float *dL, *dHpre, *dgp, *small_part, *dZ, *grad_small;
    const float* losspart; int64_t n_loss; double* loss_acc;
    bool image;                     // the form that builds pass 3's dZ image (nadm_mlp_bwd_image)
    void* dzimg; int32_t* dz_counters;
    void* stream;
    // decided
    MlpForm form; int jh; bool c8;
};

}  // namespace nadm
