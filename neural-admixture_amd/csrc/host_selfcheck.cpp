// Stand-alone self-check of the host-only units (nadm_host_io.cpp, nadm_layout.cpp, nadm_passes_host.cpp with nadm_hooks.cpp), meant to be
// built with a sanitizer: it calls every entry point on the smallest inputs that reach its edge paths, from exactly-sized heap buffers, so
// that a read or write past an end is a finding.  The asserts on the first two are light (return codes, monotone offsets, equal slices);
// the exact values are pinned by tests/test_abi_and_host.py.  The passes' host unit is linked against launchers defined HERE, which record
// the struct they are given and return 0: which form, grid split and slice count the host side decides, and that a refusal comes before
// any launch, are checked without a GPU.  Needs no GPU; the build-and-run line is in tools/README.md, tests/test_abi_and_host.py runs the
// plain build.
#include "../../include/nadm.h"
#include "nadm_host_rules.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <initializer_list>
#include <memory>
#include <string>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_selfcheck: line %d: %s  [%s]\n", __LINE__, #c, nadm_last_error()); exit(1); } } while (0)

typedef std::unique_ptr<uint8_t[]> bytes;
static bytes filled(int64_t n, uint32_t seed) {           // n bytes exactly (n == 0: a valid pointer to nothing)
    bytes p(new uint8_t[n]);
    for (int64_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; p[i] = (uint8_t)(seed >> 24); }
    return p;
}

static void check_pack(int64_t N, int64_t M, int64_t extra) {
    const int64_t mp = (M + 3) / 4, ld = mp + extra;
    bytes g = filled(N * M, 1), out = filled(N * ld, 2);
    CHECK(nadm_pack2bit_host(g.get(), out.get(), N, M, ld) == 0);
    for (int64_t r = 0; r < N; ++r) {
        for (int64_t m = 0; m < M; ++m) CHECK(((out[r * ld + m / 4] >> (2 * (m & 3))) & 3) == (g[r * M + m] & 3));
        for (int64_t c = mp; c < ld; ++c) CHECK(out[r * ld + c] == 0);
    }
    if (M > 4) CHECK(nadm_pack2bit_host(g.get(), out.get(), N, M, mp - 1) != 0 && strstr(nadm_last_error(), "ld < ceil(M/4)"));
}

static void check_bed(int64_t N, int64_t M, bool zeros) {   // an all-zero .bed is all genotype 2: the flip applies
    const int64_t nb = (N + 3) / 4, ld = (M + 3) / 4 + 3;
    bytes bed = filled(M * nb, 3);
    if (zeros) memset(bed.get(), 0, (size_t)(M * nb));
    for (int flip = 0; flip < 2; ++flip) {
        bytes out = filled(N * ld, 4);
        int64_t counts[4];
        int32_t flipped = -1;
        CHECK(nadm_bed_to_packed(bed.get(), N, M, out.get(), ld, counts, flip, &flipped) == 0);
        CHECK(counts[0] + counts[1] + counts[2] + counts[3] == N * M);
        CHECK(flipped == (flip && counts[1] + 2 * counts[2] + 3 * counts[3] >= N * M ? 1 : 0));
        if (zeros) CHECK(counts[2] == N * M && (out[0] & 3) == (flip ? 0 : 2));
        for (int64_t r = 0; r < N; ++r)
            for (int64_t c = (M + 3) / 4; c < ld; ++c) CHECK(out[r * ld + c] == 0);
    }
    CHECK(nadm_bed_to_packed(bed.get(), N, M, nullptr, ld, nullptr, 0, nullptr) != 0);
}

static void check_vcf() {
    const std::string fixed = "\t.\tA\tC\t.\t.\t.\t";
    const std::string text = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
                             "1\t10" + fixed + "GT\t./.\t0|1\n1\t20" + fixed + "GT:DP\t0/1:35\t10/2:7\n1\t30" + fixed + "GT\t1/1\t0/0";   // no last newline
    const int64_t len = (int64_t)text.size();
    std::unique_ptr<char[]> buf(new char[len]);            // no terminator behind the text
    memcpy(buf.get(), text.data(), (size_t)len);
    int64_t n = -1, m = -1;
    CHECK(nadm_vcf_parse_gt(buf.get(), len, &n, &m, nullptr) == 0 && n == 2 && m == 3);          // counting mode
    bytes out = filled(n * m, 5);
    CHECK(nadm_vcf_parse_gt(buf.get(), len, &n, &m, out.get()) == 0 && n == 2 && m == 3);        // filling mode
    const uint8_t want[6] = {3, 1, 2, 1, 12, 0};
    CHECK(memcmp(out.get(), want, 6) == 0);
    CHECK(nadm_vcf_parse_gt(buf.get(), 21, &n, &m, nullptr) != 0 && strstr(nadm_last_error(), "no #CHROM header line"));
}

static void check_savetxt() {
    char dir[] = "/tmp/nadm_selfcheck_XXXXXX";
    CHECK(mkdtemp(dir) != nullptr);
    const std::string path = std::string(dir) + "/a.txt";
    std::unique_ptr<float[]> a(new float[7]);              // 2 x 3 with row stride 4: the last row is 3 floats long
    for (int i = 0; i < 7; ++i) a[i] = 0.1f * (float)(i - 3);
    CHECK(nadm_savetxt_f32(path.c_str(), a.get(), 2, 3, 4) == 0);
    FILE* f = fopen(path.c_str(), "rb");
    CHECK(f != nullptr);
    int lines = 0, spaces = 0;
    for (int c; (c = fgetc(f)) != EOF;) { lines += c == '\n'; spaces += c == ' '; }
    fclose(f);
    CHECK(lines == 2 && spaces == 4);
    CHECK(nadm_savetxt_f32((std::string(dir) + "/no_such_dir/a.txt").c_str(), a.get(), 2, 3, 4) != 0 && strstr(nadm_last_error(), "cannot open"));
    CHECK(nadm_savetxt_f32(path.c_str(), a.get(), 2, 3, 2) != 0 && strstr(nadm_last_error(), "bad shape"));
    CHECK(unlink(path.c_str()) == 0 && rmdir(dir) == 0);
}

static void check_layout(int64_t M, int C, const int32_t* ks, int n, int32_t world, int32_t buckets) {
    nadm_heads_t hd;
    nadm_flat_layout_t fl;
    CHECK(nadm_heads_init(&hd, C, 128, ks, n) == 0);
    CHECK(hd.g_off < hd.w1_off && hd.w1_off < hd.b1_off && hd.b1_off < hd.wk_off[0] && hd.bk_off[n - 1] + ks[n - 1] == hd.n_small);
    for (int h = 0; h < n; ++h) CHECK(hd.kp[h] == nadm_pad_k(ks[h]) && hd.wk_off[h] < hd.bk_off[h] && (h == 0 || hd.qoff[h] == hd.qoff[h - 1] + hd.kp[h - 1]));
    CHECK(nadm_flat_layout(&hd, M, world, buckets, &fl) == 0);
    CHECK(fl.n_buckets >= 1 && fl.n_buckets <= buckets && fl.bkt_off[0] == 0 && fl.bkt_m0[fl.n_buckets] == M);
    int64_t sum = 0;
    for (int j = 0; j < fl.n_buckets; ++j) {
        CHECK(fl.bkt_off[j] < fl.bkt_off[j + 1] && fl.bkt_m0[j] < fl.bkt_m0[j + 1]);
        CHECK(fl.bkt_slice[j] * world == fl.bkt_off[j + 1] - fl.bkt_off[j] && fl.bkt_slice[j] % 4 == 0 && fl.bkt_mom[j] == sum);
        sum += fl.bkt_slice[j];
    }
    CHECK(sum == fl.slice_b && fl.slice_b * world == fl.msg_a_off && fl.bkt_off[fl.n_buckets] == fl.msg_a_off);
    CHECK(hd.n_small <= fl.off_v && fl.off_v + M * hd.CP <= fl.msg_a_off && fl.off_p[0] == fl.msg_a_off);
    for (int h = 1; h < n; ++h) CHECK(fl.off_p[h] == fl.off_p[h - 1] + M * hd.kp[h - 1]);
    CHECK(fl.off_p[n - 1] + M * hd.kp[n - 1] <= fl.n_flat && fl.n_flat == fl.msg_a_off + fl.slice_a * world && fl.slice_a % 4 == 0);
    CHECK(nadm_flat_layout(&hd, M, world, 9, &fl) != 0 && strstr(nadm_last_error(), "at most 8 buckets"));
}

// ---- the launchers of the passes' host unit, as recorders
static struct Recorded {
    int launches;
    nadm::Pass1Launch p1; nadm::Pass2Launch p2; nadm::Pass3Launch p3; nadm::MlpFwdLaunch mf; nadm::MlpBwdLaunch mb;
} rec;
static int g_cus = 256;
int nadm::launch_pass1(const Pass1Launch& a) { rec.p1 = a; ++rec.launches; return 0; }
int nadm::launch_pass2(const Pass2Launch& a) { rec.p2 = a; ++rec.launches; return 0; }
int nadm::launch_pass3(const Pass3Launch& a) { rec.p3 = a; ++rec.launches; return 0; }
int nadm::launch_mlp_fwd(const MlpFwdLaunch& a) { rec.mf = a; ++rec.launches; return 0; }
int nadm::launch_mlp_bwd(const MlpBwdLaunch& a) { rec.mb = a; ++rec.launches; return 0; }
int nadm::launch_tile_packed(const uint8_t*, int64_t, int64_t, int64_t, uint8_t*, void*) { ++rec.launches; return 0; }
int nadm::launch_dz_image(const float*, int32_t, int32_t, void*, void*) { ++rec.launches; return 0; }
int nadm::device_cu_count() { return g_cus; }

// status 1 with `text` in the message, and no launcher reached
#define REFUSED(call, text) do { const int n0_ = rec.launches; CHECK((call) == 1 && strstr(nadm_last_error(), text) && rec.launches == n0_); } while (0)
// status 0 and exactly one launch
#define LAUNCHED(call) do { const int n0_ = rec.launches; CHECK((call) == 0 && rec.launches == n0_ + 1); } while (0)

// pointers that are never dereferenced: the host unit only tests them for NULL and alignment
template <class T> static T* fake(uintptr_t at = 0x10000) { return reinterpret_cast<T*>(at); }
static uint8_t* const X = fake<uint8_t>();
static int32_t* const I = fake<int32_t>();
static float* const Fp = fake<float>();
static void* const Vp = fake<void>();

static void check_pass2_forms() {
    const int64_t M = 4096, ld = 1024;
    const int32_t b = 320;                                   // 5 tiles of 64: two slices leave none empty, four do
    const nadm_adam_t ad{Fp, Fp, 1e-3f, 3, 1.f, 0};
    for (int32_t kp : {4, 8, 16, 24})
        for (int qi = 0; qi < 2; ++qi)
            for (int32_t wl : {0, 1, 2, 3})
                for (int32_t ns : {1, 2})
                    for (int med = 0; med < 2; ++med) {
                        const void* qimg = qi ? Vp : nullptr;
                        nadm::Pass2Launch a{nadm::x_rows(X, ld), I, b, M, Fp, kp, Fp, 8, Fp, Fp, Fp, wl, X, qimg, ns, ns > 1 ? Fp : nullptr, ns > 1 ? I : nullptr, med != 0, Vp};
                        auto call = [&] {                       // the plan's step under "medium", the public sliced form under "highest"
                            if (med) return nadm::pass2_step_args(a, "nadm_step", &ad, false) || nadm::pass2(a) ? 1 : 0;
                            return nadm_decode_bce_sliced(X, ld, I, b, M, Fp, kp, Fp, 8, Fp, Fp, Fp, wl, X, &ad, qimg, ns, a.slab, a.counters, Vp);
                        };
                        if (med && kp <= 16 && !qi) { REFUSED(call(), "nadm_step: precision \"medium\" runs pass 2 from the Q images"); continue; }
                        if (kp > 16 && ns > 1) { REFUSED(call(), "sample slices exist for padded K <= 16 only"); continue; }
                        if (kp > 16 && qi) { REFUSED(call(), "Q images exist for padded K <= 16 only"); continue; }
                        LAUNCHED(call());
                        const nadm::Pass2Launch& r = rec.p2;
                        CHECK(r.kp == kp && r.loss == ((wl & 1) != 0) && r.unit_p == (wl != 3) && r.sliced == (ns > 1) && r.n_slices == ns);
                        CHECK(r.medium == (med != 0) && r.qimg == qimg && r.ad.m == Fp && r.ad.step_size > 0.f && r.stream == Vp && r.xg == X);
                    }
    LAUNCHED(nadm_decode_bce(X, ld, I, b, M, Fp, 8, Fp, 8, Fp, Fp, nullptr, 0, Vp));
    CHECK(!rec.p2.loss && rec.p2.unit_p && !rec.p2.sliced && !rec.p2.ad.m && !rec.p2.xg && !rec.p2.qimg && rec.p2.n_slices == 1);
    REFUSED(nadm_decode_bce(X, ld, I, b, M, Fp, 20, Fp, 8, Fp, Fp, nullptr, 0, Vp), "unsupported padded K");
    REFUSED(nadm_decode_bce(X, ld, I, b, M, Fp, 8, Fp, 8, Fp, Fp, nullptr, 1, Vp), "with_loss needs losspart");
    REFUSED(nadm_decode_bce_step(X, ld, I, b, M, fake<float>(0x10008), 8, Fp, 8, Fp, Fp, nullptr, 0, X, nullptr, Vp), "nadm_decode_bce_step: P must be 16-byte aligned");
    REFUSED(nadm_decode_bce_images(X, ld, I, b, M, Fp, 8, Fp, 8, Fp, Fp, nullptr, 0, X, nullptr, nullptr, Vp), "qimg is NULL");
}

static void check_pass3_forms() {
    const int64_t M = 4096, ld = 1024;
    const int32_t b = 640;                                   // 5 tiles of 128
    const nadm_adam_t ad{Fp, Fp, 1e-3f, 3, 1.f, 0};
    for (int32_t cp : {4, 8, 12})
        for (int32_t flags : {0, (int32_t)NADM_X_CLEAN})
            for (int32_t ns : {1, 2}) {
                auto sliced = [&] { return nadm_encode_bwd_sliced(X, ld, I, b, M, Fp, Vp, cp, Fp, Fp, &ad, nullptr, flags, ns, ns > 1 ? Fp : nullptr, ns > 1 ? I : nullptr, Vp); };
                if (cp > 8) {
                    REFUSED(sliced(), "nadm_encode_bwd_sliced: the matrix-core pass only (C <= 8)");
                    if (flags) { REFUSED(nadm_encode_bwd_step(X, ld, I, b, M, Fp, nullptr, cp, Fp, Fp, &ad, nullptr, flags, Vp), "tiled for the matrix-core pass"); continue; }
                    LAUNCHED(nadm_encode_bwd_step(X, ld, I, b, M, Fp, nullptr, cp, Fp, Fp, &ad, nullptr, flags, Vp));
                    CHECK(rec.p3.CP == cp && !rec.p3.clean && !rec.p3.sliced && rec.p3.n_slices == 1 && rec.p3.ad.m == Fp);
                    continue;
                }
                LAUNCHED(sliced());
                CHECK(rec.p3.CP == cp && rec.p3.clean == (flags != 0) && rec.p3.sliced == (ns > 1) && rec.p3.n_slices == ns && rec.p3.ad.m == Fp && rec.p3.missing_bf16 == 0u);
            }
    LAUNCHED(nadm_pca_project_t(X, ld, I, b, M, Fp, Vp, 8, Fp, Vp));
    CHECK(rec.p3.missing_bf16 == 0x3FC0u && !rec.p3.clean && !rec.p3.ad.m && !rec.p3.weights);
    LAUNCHED(nadm_encode_bwd(X, ld, I, b, M, Fp, Vp, 8, Fp, NADM_X_CLEAN, Vp));
    CHECK(rec.p3.clean && !rec.p3.sliced);
    REFUSED(nadm_encode_bwd(X, ld, I, b, M, Fp, nullptr, 13, Fp, 0, Vp), "unsupported CP");
    const nadm_mlp_weights_t half{nullptr, Fp, Fp, Fp, Fp, Fp, Fp};
    REFUSED(nadm_encode_bwd_step(X, ld, I, b, M, Fp, Vp, 8, Fp, Fp, nullptr, &half, 0, Vp), "nadm_encode_bwd_step: null pointer in the MLP weight-gradient arguments");
    LAUNCHED(nadm_dz_image(Fp, b, 8, Vp, Vp));
}

static void check_pass1_forms() {
    const int64_t ld = 1 << 18;
    const nadm_adam_t ad{Fp, Fp, 1e-3f, 3, 1.f, 0};
    // the batch splits the measurements chose (800 rows on 256 CUs): 2 at 500k SNPs, 3 at 600k, 1 at 800k and 1M
    int tpb = 0;
    CHECK(nadm::pass1_batch_splits(800, nadm_encode_chunks(500000), 0, 256, &tpb) == 2 && tpb == 25);
    CHECK(nadm::pass1_batch_splits(800, nadm_encode_chunks(600000), 0, 256, &tpb) == 3 && tpb == 17);
    CHECK(nadm::pass1_batch_splits(800, nadm_encode_chunks(800000), 0, 256, &tpb) == 1 && tpb == 50);
    CHECK(nadm::pass1_batch_splits(800, nadm_encode_chunks(1000000), 0, 256, &tpb) == 1);
    CHECK(nadm::pass1_batch_splits(800, 10, nadm_encode_chunks(1000000), 256, &tpb) == 1);              // a part of a pass splits like the whole pass
    CHECK(nadm::pass1_batch_splits(1, 1, 0, 256, &tpb) == 1 && tpb == 1);
    for (int32_t b : {1, 16, 833, 6400, 100000})                                                        // every tile is covered, no block holds more than the kernel's LDS does
        for (int64_t chunks : {1, 30, 245, 489}) {
            const int gy = nadm::pass1_batch_splits(b, chunks, 0, 256, &tpb);
            CHECK(gy >= 1 && tpb >= 1 && tpb <= nadm::EM_TILES_PER_BLOCK && (int64_t)gy * tpb >= (b + 15) / 16 && (int64_t)(gy - 1) * tpb < (b + 15) / 16);
        }
    const int32_t b = 800;
    const int64_t M = 500000;
    for (int32_t cp : {4, 8, 12}) {
        LAUNCHED(nadm_encode_fwd(X, ld, I, b, M, Fp, cp, Fp, Vp));
        CHECK(rec.p1.CP == cp && rec.p1.chunks == 245 && !rec.p1.medium && rec.p1.missing_bf16 == 0u && !rec.p1.ss.part && rec.p1.total_chunks == 0);
        if (cp <= 8) CHECK(rec.p1.gy == 2 && rec.p1.tpb == 25 && rec.p1.side_blocks == 0);
        LAUNCHED(nadm_encode_fwd_part(X, ld, I, b, 100000, Fp, cp, Fp, 245, Vp));
        CHECK(rec.p1.chunks == 49 && rec.p1.total_chunks == 245);
        if (cp <= 8) CHECK(rec.p1.gy == 2);                                                              // (49 chunks on their own would be cut finer)
        auto small = [&](const nadm_adam_t* adam) { return nadm_encode_fwd_small(X, ld, I, b, M, Fp, cp, Fp, Fp, 50, 1300, Fp, Fp, adam, Vp); };
        if (cp > 8) {
            REFUSED(small(&ad), "only the matrix-core pass (CP <= 8) hosts the side blocks");
            REFUSED(nadm_pca_project(X, ld, I, b, M, Fp, cp, Fp, Vp), "CP <= 8");
            nadm::Pass1Launch a{nadm::x_rows(X, ld), I, b, M, Fp, cp, Fp, 0, 0u, true, nadm::SmallSide{}, Vp};
            LAUNCHED(nadm::pass1(a));
            CHECK(!rec.p1.medium);                                                                       // the VALU kernel is the same under either precision
            continue;
        }
        LAUNCHED(small(&ad));
        CHECK(rec.p1.ss.part == Fp && rec.p1.ss.n == 1300 && rec.p1.ss.splits == 50 && rec.p1.side_blocks == 3 && rec.p1.ss.m == Fp && rec.p1.ss.step_size > 0.f);
        LAUNCHED(small(nullptr));
        CHECK(rec.p1.ss.part == Fp && !rec.p1.ss.m && rec.p1.side_blocks == 3);
        LAUNCHED(nadm_pca_project(X, ld, I, b, M, Fp, cp, Fp, Vp));
        CHECK(rec.p1.missing_bf16 == 0x3FC0u && !rec.p1.medium);
        nadm::Pass1Launch a{nadm::x_rows(X, ld), I, b, M, Fp, cp, Fp, 0, 0u, true, nadm::SmallSide{}, Vp};
        LAUNCHED(nadm::pass1(a));
        CHECK(rec.p1.medium && rec.p1.gy == 2);
    }
    g_cus = 64;                                                                                          // a partition of the chip reports its own CU count
    LAUNCHED(nadm_encode_fwd(X, ld, I, b, M, Fp, 8, Fp, Vp));
    CHECK(rec.p1.gy == nadm::pass1_batch_splits(b, 245, 0, 64, &tpb) && rec.p1.tpb == tpb);
    g_cus = 256;
    REFUSED(nadm_encode_fwd(X, ld, I, b, M, Fp, 20, Fp, Vp), "unsupported CP");
    REFUSED(nadm_encode_fwd_small(X, ld, I, b, M, Fp, 8, Fp, nullptr, 50, 1300, Fp, Fp, &ad, Vp), "nadm_encode_fwd_small: null pointer");
}

static void check_mlp_forms() {
    const int32_t k8[1] = {8};
    nadm_heads_t hd, wide, huge;
    CHECK(nadm_heads_init(&hd, 8, 128, k8, 1) == 0 && nadm_heads_init(&wide, 8, 2048, k8, 1) == 0 && nadm_heads_init(&huge, 8, 4096, k8, 1) == 0);
    const int32_t b = 100;
    const int64_t qbytes = nadm_q_image_bytes(b);
    CHECK(qbytes == 2 * 768 * 16);
    for (int img = 0; img < 2; ++img) {
        auto fwd = [&](const nadm_heads_t* h) {
            return img ? nadm_mlp_fwd_images(h, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, Vp, qbytes, Vp) : nadm_mlp_fwd(h, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, Vp);
        };
        auto bwd = [&](const nadm_heads_t* h) {
            return img ? nadm_mlp_bwd_image(h, Fp, Fp, 4096, b, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, nullptr, Fp, 16, fake<double>(), Vp, I, Vp)
                       : nadm_mlp_bwd(h, Fp, Fp, 4096, b, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, nullptr, Fp, 16, fake<double>(), Vp);
        };
        LAUNCHED(fwd(&hd));
        CHECK(rec.mf.form == nadm::MLP_FAST && rec.mf.jh == 4 && rec.mf.images == (img != 0) && rec.mf.qimg == (img ? Vp : nullptr) && rec.mf.qimg_head_bytes == (img ? qbytes : 0));
        CHECK(rec.mf.c8 == ((hd.w1_off & 3) == 0));
        LAUNCHED(fwd(&wide));
        CHECK(rec.mf.form == nadm::MLP_FAST && rec.mf.jh == 8);
        LAUNCHED(fwd(&huge));
        CHECK(rec.mf.form == nadm::MLP_GENERIC1);
        LAUNCHED(bwd(&hd));
        CHECK(rec.mb.form == nadm::MLP_FAST && rec.mb.jh == 4 && rec.mb.image == (img != 0) && rec.mb.dzimg == (img ? Vp : nullptr) && rec.mb.dz_counters == (img ? I : nullptr) && rec.mb.n_loss == 16);
        LAUNCHED(bwd(&wide));
        CHECK(rec.mb.form == nadm::MLP_FAST && rec.mb.jh == 8);
        LAUNCHED(bwd(&huge));
        CHECK(rec.mb.form == nadm::MLP_GENERIC1);
    }
    REFUSED(nadm_mlp_fwd_images(&hd, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, nullptr, qbytes, Vp), "qimg is NULL");
    REFUSED(nadm_mlp_fwd_images(&hd, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, Vp, qbytes - 16, Vp), "head stride smaller than nadm_q_image_bytes(b)");
    REFUSED(nadm_mlp_fwd(nullptr, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, Vp), "nadm_mlp_fwd: null pointer");
    REFUSED(nadm_mlp_bwd_image(&hd, Fp, Fp, 4096, b, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, nullptr, Fp, 0, nullptr, Vp, nullptr, Vp), "nadm_mlp_bwd_image: null pointer");
    REFUSED(nadm_mlp_bwd(&hd, Fp, Fp, 4096, b, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, Fp, nullptr, nullptr, 16, nullptr, Vp), "n_loss > 0 needs losspart and loss_acc");
#ifdef NADM_TEST_HOOKS
    nadm_test_force_generic_mlp(1);
    LAUNCHED(nadm_mlp_fwd(&hd, Fp, Fp, 3, b, Fp, Fp, Fp, Fp, Fp, Vp));
    CHECK(rec.mf.form == nadm::MLP_GENERIC4);
    nadm_test_force_generic_mlp(0);
#endif
}

// the slice rules at their edges, and the bound that sizes the slabs against every batch it has to cover
static void check_slice_rules() {
    CHECK(nadm_decode_chunks(130816, 8) == 511 && nadm_decode_slices(800, 130816, 8) == 2 && nadm_decode_slices(800, 130817, 8) == 1);     // chunks >= 512: whole
    CHECK(nadm_decode_slices(448, 25000, 8) == 1 && nadm_decode_slices(449, 25000, 8) == 2);                                                 // tiles < 8: whole
    CHECK(nadm_decode_slices(6400, 2301, 8) == NADM_MAX_P2_SLICES && nadm_decode_slices(100000, 2301, 16) == NADM_MAX_P2_SLICES);             // the cap
    CHECK(nadm_decode_slices(800, 25000, 24) == 1 && nadm_decode_slices(0, 25000, 8) == 1 && nadm_decode_slices(800, 0, 8) == 1);
    CHECK(nadm_encode_bwd_chunks(97792) == 191 && nadm_encode_slices(4096, 97792, 8) == 2 && nadm_encode_slices(4096, 97793, 8) == 1);      // chunks >= 192: whole
    CHECK(nadm_encode_slices(3968, 62500, 8) == 1 && nadm_encode_slices(3969, 62500, 8) == 2 && nadm_encode_slices(3969, 62500, 12) == 1);    // tiles < 32: whole
    for (int64_t M : {2301, 6200, 25000, 62500, 100000, 130000})
        for (int32_t bmax : {449, 800, 1603, 6400}) {
            int32_t mx = 1;
            for (int32_t b = 1; b <= bmax; ++b) { const int32_t s = nadm_decode_slices(b, M, 16); if (s > mx) mx = s; }
            CHECK(nadm_decode_slices_max(bmax, M, 16) == mx);
        }
    for (int64_t M : {1100, 3000, 62500, 125000, 190000})
        for (int32_t bmax : {1025, 1600, 6400}) {
            int32_t mx = 1;
            for (int32_t b = 1; b <= bmax; ++b) { const int32_t s = nadm_encode_slices(b, M, 8); if (s > mx) mx = s; }
            CHECK(nadm_encode_slices_max(bmax, M, 8) == mx);
        }
    CHECK(nadm_decode_slab_floats(50000, 8, 3) == 3 * nadm_decode_chunks(50000, 8) * (256 * 8 + 4) && nadm_decode_slab_floats(50000, 24, 3) == 0);
    CHECK(nadm_encode_slab_floats(62500, 8, 2) == 2 * 123 * 512 * 8 && nadm_encode_slab_floats(62500, 8, 1) == 0);
    CHECK(nadm_dz_image_bytes(800) == 7 * 7 * 64 * 16 && nadm_batch_copy_bytes(37, 2301) == 5 * 37 * 128 && nadm_decode_chunk_snps(24) == 512);
#ifdef NADM_TEST_HOOKS
    nadm_test_force_slices(3);                               // the forced count replaces the rule and is still kept from leaving a slice empty
    CHECK(nadm_decode_slices(800, 500000, 8) == 3 && nadm_decode_slices(128, 500000, 8) == 2 && nadm_decode_slices(800, 500000, 24) == 1);
    nadm_test_force_slices(0);
    CHECK(nadm_decode_slices(800, 500000, 8) == 1);
    nadm_test_force_p3_slices(4);
    CHECK(nadm_encode_slices(640, 500000, 8) == 3 && nadm_encode_slices(100, 500000, 8) == 1);             // 5 tiles in 4 slices of 2 would leave the fourth empty
    nadm_test_force_p3_slices(0);
    CHECK(nadm_encode_slices(640, 500000, 8) == 1);
#endif
}

// every refusal tests/test_abi_and_host.py asserts for these entry points comes before a launcher is reached
static void check_refusals() {
    float* const odd = fake<float>(0x1008);
    REFUSED(nadm_encode_fwd(nullptr, 16, nullptr, 1, 4, nullptr, 8, nullptr, nullptr), "null pointer");
    auto pass2 = [&](int32_t ns, float* slab, int32_t* cnt, int32_t kp) {     // (M = 0: whatever the slice checks let through is refused after them)
        return nadm_decode_bce_sliced(X, 16, I, 320, 0, Fp, kp, Fp, 8, Fp, Fp, nullptr, 0, nullptr, nullptr, nullptr, ns, slab, cnt, nullptr);
    };
    auto pass3 = [&](int32_t ns, float* slab, int32_t* cnt, int32_t cp) {
        return nadm_encode_bwd_sliced(X, 16, I, 640, 64, Fp, Vp, cp, nullptr, Fp, nullptr, nullptr, 0, ns, slab, cnt, nullptr);
    };
    REFUSED(pass2(0, Fp, I, 8), "nadm_decode_bce_sliced: n_slices must be in 1..8");
    REFUSED(pass2(9, Fp, I, 8), "nadm_decode_bce_sliced: n_slices must be in 1..8");
    REFUSED(pass2(2, nullptr, I, 8), "nadm_decode_bce_sliced: n_slices > 1 needs the slab (16-byte aligned) and the counters");
    REFUSED(pass2(2, Fp, nullptr, 8), "nadm_decode_bce_sliced: n_slices > 1 needs the slab (16-byte aligned) and the counters");
    REFUSED(pass2(2, odd, I, 8), "nadm_decode_bce_sliced: n_slices > 1 needs the slab (16-byte aligned) and the counters");
    REFUSED(pass2(4, Fp, I, 8), "nadm_decode_bce_sliced: a slice would be empty (take n_slices from nadm_decode_slices)");
    REFUSED(pass2(2, Fp, I, 24), "nadm_decode_bce_sliced: sample slices exist for padded K <= 16 only");
    REFUSED(pass2(1, Fp, I, 8), "nadm_decode_bce: empty batch or M");
    REFUSED(pass3(0, Fp, I, 8), "nadm_encode_bwd_sliced: n_slices must be in 1..8");
    REFUSED(pass3(9, Fp, I, 8), "nadm_encode_bwd_sliced: n_slices must be in 1..8");
    REFUSED(pass3(2, nullptr, I, 8), "nadm_encode_bwd_sliced: the slab (16-byte aligned) and the counters are NULL");
    REFUSED(pass3(2, Fp, nullptr, 8), "nadm_encode_bwd_sliced: the slab (16-byte aligned) and the counters are NULL");
    REFUSED(pass3(2, odd, I, 8), "nadm_encode_bwd_sliced: the slab (16-byte aligned) and the counters are NULL");
    REFUSED(pass3(4, Fp, I, 8), "nadm_encode_bwd_sliced: an empty sample slice");
    REFUSED(pass3(2, Fp, I, 12), "nadm_encode_bwd_sliced: the matrix-core pass only (C <= 8)");
    REFUSED(nadm_pca_project(X, 16, I, 4, 8, Fp, 12, Fp, nullptr), "CP <= 8");
    REFUSED(nadm_pca_project_t(X, 16, I, 4, 8, Fp, Vp, 12, Fp, nullptr), "CP <= 8");
    REFUSED(nadm_encode_bwd(X, 16, I, 4, 8, Fp, nullptr, 8, Fp, 0, nullptr), "operand image of dZ");
    REFUSED(nadm_dz_image(Fp, 4, 12, Vp, nullptr), "0 < CP <= 8");
    const int64_t ld = 1ll << 32;
    REFUSED(nadm_encode_fwd(X, ld, I, 16, 4 * ld, Fp, 8, Fp, nullptr), "4 GiB");
    REFUSED(nadm_decode_bce(X, ld, I, 16, 4 * ld, Fp, 8, Fp, 8, Fp, Fp, Fp, 1, nullptr), "4 GiB");
}

// the pair analyses' block rule: the predicate and the refusal agree, and the messages are the entries' own, byte for byte
static void check_pair_block_rule() {
    using namespace nadm;
    const int R = NADM_KINSHIP_MAX_ROWS;
    CHECK(check_pair_block("nadm_kinship", 1, R, 1, PAIR_MAX_ROWS(NADM_KINSHIP_MAX_ROWS)) == 0 && pair_block_ok(1, R, 1, R));
    const int64_t empty[4][3] = {{0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {-1, R + 1, 5}};        // (empty comes before too large)
    for (const auto& s : empty) {
        CHECK(!pair_block_ok((int)s[0], (int)s[1], s[2], R));
        CHECK(check_pair_block("nadm_ibd", (int)s[0], (int)s[1], s[2], PAIR_MAX_ROWS(NADM_IBD_MAX_ROWS)) == 1);
        CHECK(!strcmp(nadm_last_error(), "nadm_ibd: empty block (need ba > 0, bb > 0 and M > 0)"));
    }
    for (int side = 0; side < 2; ++side) {
        CHECK(!pair_block_ok(side ? 1 : R + 1, side ? R + 1 : 1, 9, R));
        CHECK(check_pair_block("nadm_king", side ? 1 : R + 1, side ? R + 1 : 1, 9, PAIR_MAX_ROWS(NADM_KING_MAX_ROWS)) == 1);
        CHECK(!strcmp(nadm_last_error(), "nadm_king: ba and bb must be <= NADM_KING_MAX_ROWS"));
    }
}

int main() {
    CHECK(nadm_abi_version() == NADM_ABI_VERSION);
    check_pair_block_rule();
    check_pack(5, 11, 0); check_pack(1, 1, 0); check_pack(0, 7, 0); check_pack(4, 0, 0); check_pack(5, 11, 5);
    check_bed(7, 5, false); check_bed(1, 3, false); check_bed(13, 1030, false); check_bed(7, 5, true); check_bed(13, 1030, true);
    check_vcf();
    check_savetxt();
    const int32_t k234[3] = {2, 3, 4}, k20[1] = {20}, k8[1] = {8}, down[2] = {5, 4}, k65[1] = {65};
    check_layout(509, 8, k234, 3, 3, 1); check_layout(77, 5, k20, 1, 5, 1); check_layout(500000, 8, k8, 1, 8, 4);
    nadm_heads_t hd;
    CHECK(nadm_heads_init(&hd, 8, 128, down, 2) != 0 && strstr(nadm_last_error(), "strictly ascending"));
    CHECK(nadm_heads_init(&hd, 8, 128, k65, 1) != 0 && strstr(nadm_last_error(), "K must be in 1..64") && nadm_pad_k(65) < 0);
    check_pass1_forms(); check_pass2_forms(); check_pass3_forms(); check_mlp_forms();
    check_slice_rules();
    check_refusals();
    printf("host_selfcheck ok\n");
    return 0;
}
