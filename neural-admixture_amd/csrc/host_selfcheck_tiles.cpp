// Stand-alone self-check of the host side of the tiled, cleaned copy of the matrix (nadm_tile_packed, XSource: nadm_pass_args.h), in the
// manner of host_selfcheck.cpp and with the same units: nadm_passes_host.cpp is linked against launchers defined HERE, which record what
// they are given.  Covered: the size query at ragged M, nadm_tile_packed's refusals and their order, the source descriptor's checks in the
// three passes (what a tiled source may and may not be combined with, each refusal before any launch), what the host side decides for a
// tiled source, and that a row-major source is still refused and launched as before.  Needs no GPU; tests/test_resident_tiles.py runs it.
#include "../../include/nadm.h"
#include "nadm_host_rules.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_selfcheck_tiles: line %d: %s  [%s]\n", __LINE__, #c, nadm_last_error()); exit(1); } } while (0)

static struct Recorded {
    int launches;
    nadm::Pass1Launch p1; nadm::Pass2Launch p2; nadm::Pass3Launch p3;
    const uint8_t* tp_xp; int64_t tp_ld, tp_rows, tp_M; uint8_t* tp_xt;
} rec;
int nadm::launch_pass1(const Pass1Launch& a) { rec.p1 = a; ++rec.launches; return 0; }
int nadm::launch_pass2(const Pass2Launch& a) { rec.p2 = a; ++rec.launches; return 0; }
int nadm::launch_pass3(const Pass3Launch& a) { rec.p3 = a; ++rec.launches; return 0; }
int nadm::launch_mlp_fwd(const MlpFwdLaunch&) { ++rec.launches; return 0; }
int nadm::launch_mlp_bwd(const MlpBwdLaunch&) { ++rec.launches; return 0; }
int nadm::launch_dz_image(const float*, int32_t, int32_t, void*, void*) { ++rec.launches; return 0; }
int nadm::launch_tile_packed(const uint8_t* xp, int64_t ld, int64_t rows, int64_t M, uint8_t* xt, void*) {
    rec.tp_xp = xp; rec.tp_ld = ld; rec.tp_rows = rows; rec.tp_M = M; rec.tp_xt = xt; ++rec.launches; return 0;
}
int nadm::device_cu_count() { return 256; }

#define REFUSED(call, text) do { const int n0_ = rec.launches; CHECK((call) == 1 && strstr(nadm_last_error(), text) && rec.launches == n0_); } while (0)
#define LAUNCHED(call) do { const int n0_ = rec.launches; CHECK((call) == 0 && rec.launches == n0_ + 1); } while (0)

// pointers that are never dereferenced: the host unit only tests them for NULL, alignment and overlap
template <class T> static T* fake(uintptr_t at = 0x10000) { return reinterpret_cast<T*>(at); }
static uint8_t* const X = fake<uint8_t>();
static uint8_t* const T = fake<uint8_t>(0x1000000000);
static int32_t* const I = fake<int32_t>();
static float* const Fp = fake<float>();
static void* const Vp = fake<void>();

static void check_size_query() {
    CHECK(nadm_tiled_bytes(37, 1000) == 2 * 37 * 128);                   // 250 B rows: the second tile is partial and still 128 B wide
    CHECK(nadm_tiled_bytes(5, 1) == 5 * 128 && nadm_tiled_bytes(5, 512) == 5 * 128 && nadm_tiled_bytes(5, 513) == 2 * 5 * 128);
    CHECK(nadm_tiled_bytes(300, 5003) == 10 * 300 * 128);
    CHECK(nadm_tiled_bytes(100000, 500000) == (int64_t)977 * 100000 * 128);
    CHECK(nadm_tiled_bytes(0, 100) == 0 && nadm_tiled_bytes(-1, 100) == 0 && nadm_tiled_bytes(3, 0) == 0);
    // the batch copy is the same layout with b rows
    for (int64_t M : {1, 511, 512, 513, 5003, 500000}) CHECK(nadm_tiled_bytes(800, M) == nadm_batch_copy_bytes(800, M));
    // pass 2's chunks (64 B) and pass 3's (128 B) never reach past the copy's last tile; pass 1's (512 B) may, and its loader clamps
    for (int64_t M : {1, 255, 256, 257, 1000, 5003}) {
        const int64_t tiles = nadm_tiled_bytes(1, M) / 128;
        CHECK((nadm_decode_chunks(M, 8) - 1) * 64 / 128 < tiles && nadm_encode_bwd_chunks(M) == tiles && nadm_encode_chunks(M) * 4 >= tiles);
    }
}

static void check_tile_packed() {
    const int64_t M = 1000, ld = 272, rows = 37;
    // the refusals in their order: every call below has all the later faults as well
    REFUSED(nadm_tile_packed(nullptr, 8, 0, 0, X + 4, Vp), "nadm_tile_packed: null pointer");
    REFUSED(nadm_tile_packed(X + 4, 8, rows, M, nullptr, Vp), "nadm_tile_packed: null pointer");
    REFUSED(nadm_tile_packed(X + 4, 8, 0, M, X + 4, Vp), "nadm_tile_packed: empty matrix");
    REFUSED(nadm_tile_packed(X + 4, 8, rows, 0, X + 4, Vp), "nadm_tile_packed: empty matrix");
    REFUSED(nadm_tile_packed(X + 4, 240, (int64_t)1 << 31, M, X + 4, Vp), "nadm_tile_packed: ld < ceil(M/4)");
    REFUSED(nadm_tile_packed(X + 4, 250, (int64_t)1 << 31, M, X + 4, Vp), "nadm_tile_packed: ld must be a multiple of 16 and < 2^32");
    REFUSED(nadm_tile_packed(X + 4, (int64_t)1 << 32, (int64_t)1 << 31, M, X + 4, Vp), "nadm_tile_packed: ld must be a multiple of 16 and < 2^32");
    REFUSED(nadm_tile_packed(X + 4, ld, (int64_t)1 << 31, M, X + 4, Vp), "nadm_tile_packed: at most 2^31 - 1 rows");
    REFUSED(nadm_tile_packed(X + 4, ld, rows, M, X + 4, Vp), "nadm_tile_packed: xp and xt must be 16-byte aligned");
    REFUSED(nadm_tile_packed(X, ld, rows, M, T + 8, Vp), "nadm_tile_packed: xp and xt must be 16-byte aligned");
    REFUSED(nadm_tile_packed(X, ld, rows, M, X, Vp), "nadm_tile_packed: xt overlaps xp");
    REFUSED(nadm_tile_packed(X, ld, rows, M, X + rows * ld - 16, Vp), "nadm_tile_packed: xt overlaps xp");                 // the copy starts inside the matrix
    REFUSED(nadm_tile_packed(X + 2 * rows * 128 - 16, ld, rows, M, X, Vp), "nadm_tile_packed: xt overlaps xp");          // the matrix starts inside the copy
    LAUNCHED(nadm_tile_packed(X, ld, rows, M, X + rows * ld, Vp));                                                           // back to back is no overlap
    LAUNCHED(nadm_tile_packed(X + 2 * rows * 128, ld, rows, M, X, Vp));
    LAUNCHED(nadm_tile_packed(X, ld, rows, M, T, Vp));
    CHECK(rec.tp_xp == X && rec.tp_ld == ld && rec.tp_rows == rows && rec.tp_M == M && rec.tp_xt == T);
    LAUNCHED(nadm_tile_packed(X, 125008, 100000, 500000, T, Vp));                                                           // the headline matrix: 12.5 GB
}

static void check_descriptor() {
    using namespace nadm;
    const XSource r = x_rows(X, 1024), t = x_tiled(T, 70000);
    CHECK(r.base == X && r.row_stride == 1024 && r.tile_stride == 128 && !r.clean);
    CHECK(t.base == T && t.row_stride == 128 && t.tile_stride == (int64_t)70000 * 128 && t.clean);
    // an SNP sub-range: whole tiles in, the strides as they were; past 4 GiB in 64 bits
    const XSource t2 = x_from_snp(t, 512 * 480);
    CHECK(t2.base == T + (int64_t)480 * 70000 * 128 && (int64_t)480 * 70000 * 128 > ((int64_t)1 << 32) && t2.row_stride == 128 && t2.tile_stride == t.tile_stride && t2.clean);
    CHECK(x_from_snp(r, 2048).base == X + 512);
}

static void check_passes() {
    using namespace nadm;
    const int64_t M = 5003, N = 300;
    const int32_t b = 130;
    const XSource t = x_tiled(T, N);
    const nadm_adam_t ad{Fp, Fp, 1e-3f, 3, 1.f, 0};
    auto p1 = [&](XSource x, int32_t cp, uint32_t miss) { return pass1(Pass1Launch{x, I, b, M, Fp, cp, Fp, 0, miss, false, SmallSide{}, Vp}); };
    auto p2 = [&](XSource x, int32_t kp, const void* qimg, int32_t ns) {
        Pass2Launch a{x, I, b, M, Fp, kp, Fp, 16, Fp, Fp, Fp, 1, nullptr, qimg, ns, ns > 1 ? Fp : nullptr, ns > 1 ? I : nullptr, false, Vp};
        return pass2_step_args(a, "nadm_step", &ad, false) || pass2(a) ? 1 : 0;
    };
    auto p3 = [&](XSource x, int32_t cp, int32_t flags, uint32_t miss, int32_t ns) {
        Pass3Launch a{x, I, b, M, Fp, cp <= 8 ? Vp : nullptr, cp, Fp, Fp, nullptr, flags, miss, ns, ns > 1 ? Fp : nullptr, ns > 1 ? I : nullptr, Vp};
        return pass3_step_args(a, "nadm_step", &ad, false) || pass3(a) ? 1 : 0;
    };
    // ---- a malformed tiled source is refused by every pass, in the pass's name
    XSource bad = t;
    bad.row_stride = 256;
    REFUSED(p1(bad, 8, 0u), "nadm_encode_fwd: a tiled source has rows of 128 bytes");
    REFUSED(p2(bad, 8, Vp, 1), "nadm_decode_bce: a tiled source has rows of 128 bytes");
    REFUSED(p3(bad, 8, 0, 0u, 1), "nadm_encode_bwd: a tiled source has rows of 128 bytes");
    bad = t; bad.tile_stride = 100;
    REFUSED(p1(bad, 8, 0u), "a tiled source has rows of 128 bytes");
    bad = t; bad.tile_stride = 0;
    REFUSED(p2(bad, 8, Vp, 1), "a tiled source has rows of 128 bytes");
    bad = t; bad.base = T + 8;
    REFUSED(p1(bad, 8, 0u), "nadm_encode_fwd: a tiled source must be 16-byte aligned");
    REFUSED(p3(bad, 8, 0, 0u, 1), "nadm_encode_bwd: a tiled source must be 16-byte aligned");
    bad = t; bad.base = nullptr;
    REFUSED(p1(bad, 8, 0u), "nadm_encode_fwd: null pointer");
    REFUSED(p2(bad, 8, Vp, 1), "nadm_decode_bce: null pointer");
    REFUSED(p3(bad, 8, 0, 0u, 1), "nadm_encode_bwd: null pointer");
    // ---- what the copy cannot feed: missing = 1.5 (it holds no code 3), the VALU kernels, pass 2 without the Q images
    REFUSED(p1(t, 8, 0x3FC0u), "a missing call read as 1.5 needs the row-major matrix");
    REFUSED(p3(t, 8, 0, 0x3FC0u, 1), "a missing call read as 1.5 needs the row-major matrix");
    REFUSED(p1(t, 16, 0u), "the tiled copy feeds the matrix-core pass only (C <= 8)");
    REFUSED(p3(t, 16, 0, 0u, 1), "tiled for the matrix-core pass, C <= 8");
    REFUSED(p2(t, 24, nullptr, 1), "the tiled copy feeds the matrix-core pass from the Q images only");
    REFUSED(p2(t, 8, nullptr, 1), "the tiled copy feeds the matrix-core pass from the Q images only");
    REFUSED(p3(t, 8, NADM_X_CLEAN, 0u, 1), "NADM_X_CLEAN names pass 2's batch copy");
    // order: the empty batch comes before the descriptor in pass 1 and after it in pass 3, as for ld
    bad = t; bad.row_stride = 256;
    REFUSED(pass1(Pass1Launch{bad, I, 0, M, Fp, 8, Fp, 0, 0u, false, SmallSide{}, Vp}), "nadm_encode_fwd: empty batch or M");
    // ---- what is launched
    for (int32_t cp : {4, 8}) {
        LAUNCHED(p1(t, cp, 0u));
        CHECK(rec.p1.x.clean && rec.p1.x.base == T && rec.p1.x.tile_stride == N * 128 && rec.p1.chunks == 3 && rec.p1.CP == cp);
    }
    for (int32_t kp : {4, 8, 12, 16})
        for (int32_t ns : {1, 2}) {
            LAUNCHED(p2(t, kp, Vp, ns));
            CHECK(rec.p2.x.clean && rec.p2.x.row_stride == 128 && rec.p2.sliced == (ns > 1) && rec.p2.xg == nullptr && rec.p2.qimg == Vp && rec.p2.ad.m == Fp);
        }
    for (int32_t ns : {1, 2}) {
        LAUNCHED(p3(t, 8, 0, 0u, ns));
        CHECK(rec.p3.clean && rec.p3.gather && rec.p3.x.base == T && rec.p3.x.tile_stride == N * 128 && rec.p3.sliced == (ns > 1));
    }
    // pass 2's batch copy, handed over like a matrix: tiles of b rows, rows in batch order
    LAUNCHED(p3(x_rows(X, 1264), 8, NADM_X_CLEAN, 0u, 1));
    CHECK(rec.p3.clean && !rec.p3.gather && rec.p3.x.base == X && rec.p3.x.row_stride == 128 && rec.p3.x.tile_stride == (int64_t)b * 128);
    // ---- the row-major source: refused and launched as before
    REFUSED(p1(x_rows(X, 1256), 8, 0u), "nadm_encode_fwd: ld must be a multiple of 16 and >= ceil(M/4)");
    REFUSED(p1(x_rows(X, (int64_t)1 << 32), 8, 0u), "nadm_encode_fwd: rows of 4 GiB and more");
    REFUSED(p2(x_rows(X, (int64_t)1 << 32), 8, Vp, 1), "nadm_decode_bce: rows of 4 GiB and more");
    REFUSED(p2(x_rows(X, 1200), 8, Vp, 1), "nadm_decode_bce: ld must be a multiple of 16 and >= ceil(M/4)");
    REFUSED(p3(x_rows(X, 1200), 8, 0, 0u, 1), "nadm_encode_bwd: ld must be a multiple of 16 and >= ceil(M/4)");
    LAUNCHED(p1(x_rows(X, 1264), 8, 0x3FC0u));
    CHECK(!rec.p1.x.clean && rec.p1.x.row_stride == 1264 && rec.p1.missing_bf16 == 0x3FC0u);
    LAUNCHED(p2(x_rows(X, 1264), 8, nullptr, 1));
    CHECK(!rec.p2.x.clean && rec.p2.x.tile_stride == 128);
    LAUNCHED(p3(x_rows(X, 1264), 8, 0, 0u, 1));
    CHECK(!rec.p3.clean && !rec.p3.gather && rec.p3.x.row_stride == 1264);
    LAUNCHED(nadm_encode_fwd(X, 1264, I, b, M, Fp, 8, Fp, Vp));
    CHECK(!rec.p1.x.clean && rec.p1.x.base == X && rec.p1.x.row_stride == 1264);
}

int main() {
    check_size_query();
    check_tile_packed();
    check_descriptor();
    check_passes();
    printf("host_selfcheck_tiles ok\n");
    return 0;
}
