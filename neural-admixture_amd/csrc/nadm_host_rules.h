// Host-side rules shared by the C-ABI translation units: argument checks, the dispatch from run-time values to template arguments, the
// split rule, the Adam scalars, the test hooks, and the seam between the host unit of the genotype passes (nadm_passes_host.cpp) and the
// units that hold their kernels.  Plain C++, no HIP header (nadm_host.h adds check_launch for the units that launch).
#pragma once
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "nadm_err.h"
#include "nadm_pass_args.h"

namespace nadm {

// ---- argument checks shared by the entry points that read the packed matrix and one head's Q and P.  Each sets the message
// "<who>: <what>" and returns 1, or returns 0
inline int failf(const char* who, const char* what) {
    snprintf(err_buf(), 512, "%s: %s", who, what);
    return 1;
}
inline int check_packed(const char* who, int64_t ld, int64_t M) {
    if (ld * 4 < M) return failf(who, "ld < ceil(M/4)");
    if (ld % 16 != 0 || ld >= (1ll << 32)) return failf(who, "ld must be a multiple of 16 and < 2^32");
    return 0;
}
inline int check_head(const char* who, int32_t k, int32_t kp, int32_t q_stride) {
    if (k < 1 || k > NADM_MAX_K) return failf(who, "K must be in 1..NADM_MAX_K");
    if (kp != nadm_pad_k(k)) return failf(who, "kp must be nadm_pad_k(k)");
    if (q_stride < kp) return failf(who, "q_stride < kp");
    if (q_stride % 4 != 0) return failf(who, "q_stride must be a multiple of 4");
    return 0;
}
inline int check_eps(const char* who, float eps) {
    return (eps >= 1e-9f && eps < 0.5f) ? 0 : failf(who, "eps must be in [1e-9, 0.5)");
}

// the block of sample pairs (ba rows x bb rows over M SNPs) of nadm_kinship, nadm_king, nadm_ibd and nadm_resid_cor: the predicate behind
// their *_ranges / *_scratch_* queries and the refusal of their entries, one rule.  PAIR_MAX_ROWS(NADM_X_MAX_ROWS) passes the bound and
// the name the message gives it
#define PAIR_MAX_ROWS(macro) macro, #macro
inline bool pair_block_ok(int ba, int bb, int64_t M, int max_rows) { return ba > 0 && bb > 0 && ba <= max_rows && bb <= max_rows && M > 0; }
inline int check_pair_block(const char* who, int ba, int bb, int64_t M, int max_rows, const char* max_name) {
    if (pair_block_ok(ba, bb, M, max_rows)) return 0;
    if (ba <= 0 || bb <= 0 || M <= 0) return failf(who, "empty block (need ba > 0, bb > 0 and M > 0)");
    snprintf(err_buf(), 512, "%s: ba and bb must be <= %s", who, max_name);
    return 1;
}

// f(std::integral_constant<int, KP>{}) for kp = KP, one of the eight padded widths of a head (nadm_pad_k)
template <class F>
inline int dispatch_kp(const char* who, int kp, F&& f) {
    switch (kp) {
        case 4: f(std::integral_constant<int, 4>{}); return 0;
        case 8: f(std::integral_constant<int, 8>{}); return 0;
        case 12: f(std::integral_constant<int, 12>{}); return 0;
        case 16: f(std::integral_constant<int, 16>{}); return 0;
        case 24: f(std::integral_constant<int, 24>{}); return 0;
        case 32: f(std::integral_constant<int, 32>{}); return 0;
        case 48: f(std::integral_constant<int, 48>{}); return 0;
        case 64: f(std::integral_constant<int, 64>{}); return 0;
        default: return failf(who, "unsupported padded K (use nadm_pad_k)");
    }
}

// f(c1, c2, ...) with ci = std::true_type{} or std::false_type{} for each of the bools that follow f;
// f(std::integral_constant<int, V>{}) for the V of the list that v equals (false: none does)
template <class F>
inline void dispatch_bool(F&& f) { f(); }
template <class F, class... Bs>
inline void dispatch_bool(F&& f, bool v, Bs... rest) {
    if (v) dispatch_bool([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else dispatch_bool([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <int... Vs, class F>
inline bool dispatch_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- the split rule of the kernels that cut one axis of their work into parts whose partial sums a second launch folds: the axis of
// `units` units (tiles of samples, chunks of SNPs) is cut into as many parts as it takes to put `want_blocks` blocks on the chip, given
// the `other` axis' block count, while there are units to split, and never more than `max_units` units go into one part (what one fp32
// running sum may cover).  A rule of the shape alone.  Returns the units per part; the parts are ceil(units / that).
inline int64_t split_per_part(int64_t units, int64_t other, int64_t want_blocks, int64_t max_units) {
    int64_t want = (want_blocks + other - 1) / other;
    if (want > units) want = units;
    const int64_t least = (units + max_units - 1) / max_units;
    if (want < least) want = least;
    return (units + want - 1) / want;
}
// a bound of parts x other for sizing the partials that grows with units and with other (the product itself does not:
// ceil(want_blocks / other) other wobbles with other)
inline int64_t split_blocks_bound(int64_t units, int64_t other, int64_t want_blocks, int64_t max_units) {
    const int64_t least = (units + max_units - 1) / max_units;
    int64_t blocks = other * units < want_blocks - 1 + other ? other * units : want_blocks - 1 + other;
    if (blocks < other * least) blocks = other * least;
    return blocks;
}

// step-dependent scalars of the Adam update (bias corrections folded in): step_size = lr / (1 - b1^t), inv_bc2 = 1 / sqrt(1 - b2^t)
inline void adam_scalars(float lr, int step, float* step_size, float* inv_bc2) {
    const double bc1 = 1.0 - pow(0.9, (double)step);
    const double bc2 = 1.0 - pow(0.95, (double)step);
    *step_size = (float)((double)lr / bc1);
    *inv_bc2 = (float)(1.0 / sqrt(bc2));
}

// The test hooks (nadm_hooks.cpp): 0 = the library's own rule.  In libnadm.so they always return 0; in libnadm_testhooks.so they return
// what nadm_test_force_slices / nadm_test_force_p3_slices / nadm_test_force_generic_mlp last set.
int hook_p2_slices();
int hook_p3_slices();
int hook_generic_mlp();

// ---- the genotype passes and the MLP pair.  pass1 .. mlp_bwd (nadm_passes_host.cpp) are the one checked path of each launch: they refuse
// what every public form refuses, in the public forms' words, decide the rest of the struct and call the launcher.  The *_step_args fold
// the optional Adam state (and pass 3's side work) in first, naming `who` in the refusals: the public form, or "nadm_step".
int pass1_small_args(Pass1Launch& a, const float* small_part, int32_t splits, int32_t n_small, float* grad_small, float* small, const nadm_adam_t* adam);
int pass1(Pass1Launch a);
int pass2_step_args(Pass2Launch& a, const char* who, const nadm_adam_t* adam, bool p_aligned_without_adam);
int pass2(Pass2Launch a);
int pass3_step_args(Pass3Launch& a, const char* who, const nadm_adam_t* adam, bool sliced_form);
int pass3(Pass3Launch a);
int mlp_fwd(MlpFwdLaunch a);
int mlp_bwd(MlpBwdLaunch a);
// pass 1's batch-split rule: grid.y for b rows and `chunks` SNP chunks (`total_chunks` when the launch is one part of a larger pass) on a
// device of cu_count compute units; *tpb = the 16-sample tiles per block
int pass1_batch_splits(int32_t b, int64_t chunks, int64_t total_chunks, int cu_count, int* tpb);

// The launchers (nadm_genotype_passes.hip, nadm_small_kernels.hip): template selection, the launches and check_launch, nothing refused
// but what only the runtime can refuse.
int launch_pass1(const Pass1Launch& a);
int launch_pass2(const Pass2Launch& a);
int launch_pass3(const Pass3Launch& a);
int launch_mlp_fwd(const MlpFwdLaunch& a);
int launch_mlp_bwd(const MlpBwdLaunch& a);
int launch_tile_packed(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, uint8_t* xt, void* stream);
int launch_dz_image(const float* dZ, int32_t b, int32_t CP, void* dzimg, void* stream);
int device_cu_count();              // compute units of the current device (256 if the runtime cannot say)

// the partial sums only (the first kernel of nadm_mlp_bwd_weights): used by the variants of pass 3 that cannot host them
int mlp_bwd_weight_parts(const nadm_heads_t* hd, int32_t b, const float* Zn, const float* H, const float* dL, const float* dHpre,
                         const float* dgp, float* small_part, void* stream);

}  // namespace nadm
