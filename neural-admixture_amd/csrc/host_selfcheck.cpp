// Stand-alone self-check of the host-only units (nadm_host_io.cpp, nadm_layout.cpp), meant to be built with a sanitizer: it calls every
// entry point on the smallest inputs that reach its edge paths, from exactly-sized heap buffers, so that a read or write past an end
// is a finding.  The asserts are light (return codes, monotone offsets, equal slices); the exact values are pinned by
// tests/test_abi_and_host.py.  Not a pytest, needs no GPU; the build-and-run line is in tools/README.md.
#include "../../include/nadm.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
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

int main() {
    CHECK(nadm_abi_version() == NADM_ABI_VERSION);
    check_pack(5, 11, 0); check_pack(1, 1, 0); check_pack(0, 7, 0); check_pack(4, 0, 0); check_pack(5, 11, 5);
    check_bed(7, 5, false); check_bed(1, 3, false); check_bed(13, 1030, false); check_bed(7, 5, true); check_bed(13, 1030, true);
    check_vcf();
    check_savetxt();
    const int32_t k234[3] = {2, 3, 4}, k20[1] = {20}, k8[1] = {8}, down[2] = {5, 4}, k65[1] = {65};
    check_layout(509, 8, k234, 3, 3, 1); check_layout(77, 5, k20, 1, 5, 1); check_layout(500000, 8, k8, 1, 8, 4);
    nadm_heads_t hd;
    CHECK(nadm_heads_init(&hd, 8, 128, down, 2) != 0 && strstr(nadm_last_error(), "strictly ascending"));
    CHECK(nadm_heads_init(&hd, 8, 128, k65, 1) != 0 && strstr(nadm_last_error(), "K must be in 1..64") && nadm_pad_k(65) < 0);
    printf("host_selfcheck ok\n");
    return 0;
}
