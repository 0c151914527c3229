// The flat parameter layout (include/nadm.h): the head table (nadm_pad_k, nadm_heads_init) says where each small parameter and each
// head's columns sit, nadm_flat_layout places [small | V | all P] and cuts it into the messages of a sample-sharded step.
// Plain C++, host only.
#include "nadm_err.h"

using namespace nadm;

// ------------------------------------------------------------------------------------------------- head table
extern "C" int nadm_pad_k(int k) {
    if (k <= 0 || k > NADM_MAX_K) return -1;
    if (k <= 16) return (k + 3) & ~3;
    if (k <= 24) return 24;
    if (k <= 32) return 32;
    if (k <= 48) return 48;
    return 64;
}
static int pad_c(int c) {
    if (c <= 0 || c > 32) return -1;
    if (c <= 16) return (c + 3) & ~3;
    return c <= 24 ? 24 : 32;
}

extern "C" int nadm_heads_init(nadm_heads_t* out, int C, int Hd, const int32_t* ks, int n) {
    if (!out || !ks) return fail("nadm_heads_init: null pointer");
    if (n <= 0 || n > NADM_MAX_HEADS) return fail("nadm_heads_init: 1..32 heads supported");
    if (pad_c(C) < 0) return fail("nadm_heads_init: n_components must be in 1..32");
    if (Hd <= 0 || Hd > 8192) return fail("nadm_heads_init: hidden size must be in 1..8192");
    memset(out, 0, sizeof(*out));
    out->n_heads = n; out->C = C; out->CP = pad_c(C); out->Hd = Hd;
    int off = 0;
    out->g_off = off; off += C;
    out->w1_off = off; off += Hd * C;
    out->b1_off = off; off += Hd;
    int q = 0;
    for (int h = 0; h < n; ++h) {
        const int kp = nadm_pad_k(ks[h]);
        if (kp < 0) return fail("nadm_heads_init: K must be in 1..64");
        if (h > 0 && ks[h] <= ks[h - 1]) return fail("nadm_heads_init: ks must be strictly ascending");
        out->k[h] = ks[h]; out->kp[h] = kp; out->qoff[h] = q; q += kp;
        out->wk_off[h] = off; off += ks[h] * Hd;
        out->bk_off[h] = off; off += ks[h];
    }
    out->SP = q;
    out->n_small = off;
    return 0;
}

// ------------------------------------------------------------------------------------------------- flat layout
static int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
static int64_t lcm64(int64_t a, int64_t b) { return a / gcd64(a, b) * b; }

extern "C" int nadm_flat_layout(const nadm_heads_t* hd, int64_t M, int32_t world, int32_t n_buckets, nadm_flat_layout_t* out) {
    if (!hd || !out) return fail("nadm_flat_layout: null pointer");
    if (M <= 0 || world < 1 || hd->n_heads < 1 || hd->n_heads > NADM_MAX_HEADS) return fail("nadm_flat_layout: M, world >= 1 and 1..32 heads");
    if (n_buckets < 0 || n_buckets > NADM_MAX_BUCKETS) return fail("nadm_flat_layout: at most 8 buckets");
    memset(out, 0, sizeof(*out));
    const int64_t q = 4 * (int64_t)world;                               // a rank's slice is a multiple of 4 floats (16 bytes: the Adam kernel's vector accesses)
    out->off_v = round_up(hd->n_small, lcm64(64, q));
    // range boundaries of message B's buckets: multiples of U SNPs = a multiple of every pass's chunk (pass 1: 2048, pass 3: 512) whose
    // V rows are a multiple of q floats, so that every bucket but the last is `world` slices without a gap
    const int64_t U = lcm64(2048, q / gcd64(q, hd->CP));
    const int64_t units = (M + U - 1) / U;
    int64_t nb = n_buckets < 1 ? 1 : n_buckets;
    if (nb > units) nb = units;
    out->n_buckets = (int32_t)nb;
    const int64_t b_end = round_up(out->off_v + M * hd->CP, q);
    for (int64_t j = 0; j <= nb; ++j) {
        const int64_t m = j == nb ? M : U * (j * units / nb);
        out->bkt_m0[j] = m;
        out->bkt_off[j] = j == 0 ? 0 : (j == nb ? b_end : out->off_v + m * hd->CP);
    }
    for (int64_t j = 0; j < nb; ++j) {
        out->bkt_slice[j] = (out->bkt_off[j + 1] - out->bkt_off[j]) / world;
        out->bkt_mom[j] = out->slice_b;
        out->slice_b += out->bkt_slice[j];
    }
    out->msg_a_off = b_end;
    int64_t off = out->msg_a_off;
    for (int h = 0; h < hd->n_heads; ++h) {
        out->off_p[h] = off;
        off += M * hd->kp[h];
    }
    out->slice_a = round_up(off - out->msg_a_off, q) / world;
    out->n_flat = out->msg_a_off + out->slice_a * world;
    return 0;
}
