// Host-only entry points that read or write data from outside the program (include/nadm.h): the host packer, the PLINK .bed
// converter, the VCF genotype parser and the savetxt writer, plus nadm_abi_version / nadm_last_error.  Plain C++: nothing here
// launches a kernel or includes a HIP header, so this unit also builds on its own under a sanitizer (host_selfcheck.cpp).
#include "nadm_err.h"
#include <stdlib.h>
#include <array>
#include <thread>
#include <vector>

using namespace nadm;

// -------------------------------------------------------------------------------------------------
extern "C" int nadm_abi_version(void) { return NADM_ABI_VERSION; }
extern "C" const char* nadm_last_error(void) { return err_buf(); }

extern "C" int nadm_pack2bit_host(const uint8_t* g, uint8_t* out, int64_t N, int64_t M, int64_t ld) {
    if (!g || !out) return fail("nadm_pack2bit_host: null pointer");
    if (ld * 4 < M) return fail("nadm_pack2bit_host: ld < ceil(M/4)");
    auto work = [=](int64_t r_begin, int64_t r_end) {
        for (int64_t r = r_begin; r < r_end; ++r) {
            const uint8_t* src = g + r * M;
            uint8_t* dst = out + r * ld;
            const int64_t full = M / 4;
            for (int64_t c = 0; c < full; ++c) {
                const uint8_t* s = src + 4 * c;
                dst[c] = (uint8_t)((s[0] & 3) | ((s[1] & 3) << 2) | ((s[2] & 3) << 4) | ((s[3] & 3) << 6));
            }
            if (full * 4 < M) {
                uint8_t v = 0;
                for (int64_t s = full * 4; s < M; ++s) v |= (uint8_t)((src[s] & 3) << (2 * (s - full * 4)));
                dst[full] = v;
            }
            for (int64_t c = (M + 3) / 4; c < ld; ++c) dst[c] = 0;
        }
    };
    int nt = (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 32) nt = 32;
    if ((int64_t)nt > N) nt = (int)(N > 0 ? N : 1);
    if (N * M < (1 << 22)) nt = 1;
    if (nt == 1) {
        work(0, N);
    } else {
        std::vector<std::thread> th;
        const int64_t per = (N + nt - 1) / nt;
        for (int t = 0; t < nt; ++t) {
            const int64_t r0 = t * per, r1 = r0 + per < N ? r0 + per : N;
            if (r0 < r1) th.emplace_back(work, r0, r1);
        }
        for (auto& t : th) t.join();
    }
    return 0;
}

// -------------------------------------------------------------------------------------------------
// PLINK .bed (SNP-major, 4 samples/byte) -> sample-major packed (4 SNPs/byte): a 2-bit matrix transpose
// with the reference's recode table [2,3,1,0] (utils.pyx:52).  Each worker owns blocks of 256 SNPs so that
// it writes 64 contiguous bytes per sample row.
// -------------------------------------------------------------------------------------------------
extern "C" int nadm_bed_to_packed(const uint8_t* bed, int64_t N, int64_t M, uint8_t* out, int64_t ld, int64_t* counts,
                                  int32_t flip_if_mean_ge1, int32_t* flipped) {
    if (!bed || !out || !counts) return fail("nadm_bed_to_packed: null pointer");
    if (ld * 4 < M) return fail("nadm_bed_to_packed: ld < ceil(M/4)");
    const int64_t nb = (N + 3) / 4;                       // bytes per SNP in the .bed
    int nt = (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 64) nt = 64;
    const int64_t nblk = (M + 255) / 256;
    if (nblk < nt) nt = (int)(nblk > 0 ? nblk : 1);
    std::vector<std::array<int64_t, 4>> cnt(nt, std::array<int64_t, 4>{0, 0, 0, 0});
    // word-level version of the device kernel: the bytes of 4 consecutive SNPs at one sample-byte column form a 4 x 4 block
    // of 2-bit fields; recode bitwise, transpose with two delta swaps, one output byte per sample
    auto tr = [](uint32_t w) -> uint32_t {
        uint32_t t = ((w >> 6) ^ w) & 0x00CC00CCu;
        w ^= t ^ (t << 6);
        t = ((w >> 12) ^ w) & 0x0000F0F0u;
        return w ^ t ^ (t << 12);
    };
    auto work = [&](int t) {
        uint8_t rows[4][64];
        for (int64_t blk = t; blk < nblk; blk += nt) {
            const int64_t m0 = blk * 256;
            const int64_t nm = (M - m0 < 256) ? (M - m0) : 256;
            const int64_t ncol = (nm + 3) / 4;            // output bytes per row in this block
            for (int64_t bi = 0; bi < nb; ++bi) {
                const int ns = (int)((N - 4 * bi < 4) ? (N - 4 * bi) : 4);
                const uint32_t smask = ns == 4 ? 0xFFu : ((1u << (2 * ns)) - 1u);
                for (int64_t g = 0; g < ncol; ++g) {
                    uint32_t w = 0, valid = 0;
                    for (int r = 0; r < 4; ++r)
                        if (4 * g + r < nm) {
                            w |= (uint32_t)bed[(m0 + 4 * g + r) * nb + bi] << (8 * r);
                            valid |= smask << (8 * r);
                        }
                    const uint32_t hi = w & 0xAAAAAAAAu, lo = w & 0x55555555u;
                    const uint32_t gq = (((~hi) & 0xAAAAAAAAu) | (lo ^ (hi >> 1))) & valid;
                    const uint32_t gl = gq & 0x55555555u, gh = (gq >> 1) & 0x55555555u;
                    const int c3 = __builtin_popcount(gl & gh), c2 = __builtin_popcount(gh & ~gl), c1 = __builtin_popcount(gl & ~gh);
                    cnt[t][3] += c3; cnt[t][2] += c2; cnt[t][1] += c1;
                    cnt[t][0] += __builtin_popcount(valid & 0x55555555u) - c1 - c2 - c3;
                    const uint32_t q = tr(gq);
                    rows[0][g] = (uint8_t)q; rows[1][g] = (uint8_t)(q >> 8); rows[2][g] = (uint8_t)(q >> 16); rows[3][g] = (uint8_t)(q >> 24);
                }
                for (int s4 = 0; s4 < ns; ++s4) memcpy(out + (4 * bi + s4) * ld + (m0 >> 2), rows[s4], (size_t)ncol);
            }
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    for (int c = 0; c < 4; ++c) { counts[c] = 0; for (int t = 0; t < nt; ++t) counts[c] += cnt[t][c]; }
    // zero the row padding
    const int64_t mp = (M + 3) / 4;
    if (ld > mp)
        for (int64_t r = 0; r < N; ++r) memset(out + r * ld + mp, 0, (size_t)(ld - mp));
    int did = 0;
    if (flip_if_mean_ge1 && N > 0 && M > 0) {
        const double mean = (double)(counts[1] + 2 * counts[2] + 3 * counts[3]) / ((double)N * (double)M);
        if (mean >= 1.0) {
            did = 1;                                      // 0 <-> 2, 1 and 3 unchanged: c ^= ((~c & 1) << 1) on every 2-bit field
            const int64_t tail_fields = M & 3;
            for (int64_t r = 0; r < N; ++r) {
                uint8_t* row = out + r * ld;
                for (int64_t c = 0; c < mp; ++c) row[c] ^= (uint8_t)((~row[c] & 0x55) << 1);
                if (tail_fields) row[mp - 1] &= (uint8_t)((1u << (2 * tail_fields)) - 1);    // keep the tail bits zero
            }
        }
    }
    if (flipped) *flipped = did;
    return 0;
}

// VCF text -> genotype codes, the semantics of the reference's reader (src/snp_reader.py:73-87): scikit-allel's
// read_vcf(fields=["calldata/GT"], types i1, fills -1) gives two allele indices per call (a missing or absent allele is -1),
// the reader sums them and maps negative sums to 3.  So 0/0 -> 0, 0/1 -> 1, 1|1 -> 2, ./. -> 3, and -- as there -- a
// half-missing call ./1 or a haploid call 1 sums to 0.  buf holds the whole (decompressed) file; out == NULL: only count.
// Output is sample-major uint8 [n_samples, n_variants] like the reference's G.  Variant lines are parsed by std::threads.
extern "C" int nadm_vcf_parse_gt(const char* buf, int64_t len, int64_t* n_samples, int64_t* n_variants, uint8_t* out) {
    if (!buf || !n_samples || !n_variants) return fail("nadm_vcf_parse_gt: null pointer");
    std::vector<int64_t> starts;                       // offsets of the variant lines
    int64_t N = -1;
    for (int64_t p = 0; p < len;) {
        const char* nl = (const char*)memchr(buf + p, '\n', (size_t)(len - p));
        const int64_t e = nl ? (nl - buf) : len;
        if (e > p && buf[p] != '#') starts.push_back(p);
        else if (e > p + 6 && memcmp(buf + p, "#CHROM", 6) == 0) {
            int tabs = 0;
            for (int64_t q = p; q < e; ++q) tabs += buf[q] == '\t';
            N = tabs >= 9 ? tabs - 8 : 0;
        }
        p = e + 1;
    }
    if (N < 0) return fail("nadm_vcf_parse_gt: no #CHROM header line");
    const int64_t M = (int64_t)starts.size();
    *n_samples = N; *n_variants = M;
    if (!out) return 0;
    int bad = 0;
    auto work = [&](int64_t v0, int64_t v1) {
        for (int64_t v = v0; v < v1; ++v) {
            int64_t p = starts[v];
            int col = 0;
            bool gt_first = false;
            while (p < len && buf[p] != '\n' && col < 9) {          // skip the 9 fixed columns; FORMAT must start with GT
                if (col == 8) gt_first = (p + 1 < len && buf[p] == 'G' && buf[p + 1] == 'T' && (p + 2 >= len || buf[p + 2] == ':' || buf[p + 2] == '\t'));
                while (p < len && buf[p] != '\t' && buf[p] != '\n') ++p;
                if (p < len && buf[p] == '\t') ++p;
                ++col;
            }
            for (int64_t s = 0; s < N; ++s) {
                int a[2] = {-1, -1}, na = 0;
                if (p < len && buf[p] != '\n') {
                    if (gt_first) {
                        while (p < len && buf[p] != '\t' && buf[p] != '\n' && buf[p] != ':') {
                            if (buf[p] == '/' || buf[p] == '|') { ++p; continue; }
                            int val = -1;
                            if (buf[p] == '.') ++p;
                            else if (buf[p] >= '0' && buf[p] <= '9') { val = 0; while (p < len && buf[p] >= '0' && buf[p] <= '9') val = val * 10 + (buf[p++] - '0'); }
                            else { __atomic_store_n(&bad, 1, __ATOMIC_RELAXED); ++p; }
                            if (na < 2) a[na] = val;
                            ++na;
                        }
                    }
                    while (p < len && buf[p] != '\t' && buf[p] != '\n') ++p;
                    if (p < len && buf[p] == '\t') ++p;
                }
                const int sum = a[0] + a[1];
                out[s * M + v] = (uint8_t)(sum < 0 ? 3 : (sum > 255 ? 255 : sum));
            }
        }
    };
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (nt > 32) nt = 32;
    if ((int64_t)nt > M) nt = (unsigned)(M > 0 ? M : 1);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, M * t / nt, M * (t + 1) / nt);
    for (auto& t : th) t.join();
    return bad ? fail("nadm_vcf_parse_gt: unexpected character in a GT field") : 0;
}

// np.savetxt(path, A, delimiter=' ') for a float32 matrix, byte for byte: numpy formats every element with
// '%.18e' applied to the value widened to double, one row per line, '\n' line ends (reference: src/utils.py:56-66).
// Rows are formatted by std::threads into per-thread buffers and written in order.
extern "C" int nadm_savetxt_f32(const char* path, const float* a, int64_t rows, int64_t cols, int64_t row_stride) {
    if (!path || (!a && rows * cols > 0)) return fail("nadm_savetxt_f32: null pointer");
    if (rows < 0 || cols < 0 || row_stride < cols) return fail("nadm_savetxt_f32: bad shape");
    FILE* f = fopen(path, "wb");
    if (!f) return fail("nadm_savetxt_f32: cannot open output file");
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? (hw > 32 ? 32 : hw) : 4);
    const int64_t block_rows = 2048;                      // rows per thread per round
    std::vector<std::vector<char>> bufs(nt);
    bool ok = true;
    for (int64_t r0 = 0; r0 < rows && ok; r0 += block_rows * nt) {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) {
            const int64_t b0 = r0 + t * block_rows, b1 = b0 + block_rows < rows ? b0 + block_rows : rows;
            bufs[t].clear();
            if (b0 >= rows) continue;
            th.emplace_back([&, t, b0, b1] {
                std::vector<char>& o = bufs[t];
                o.resize((size_t)(b1 - b0) * (size_t)(cols * 26 + 1));
                char* w = o.data();
                for (int64_t r = b0; r < b1; ++r) {
                    const float* row = a + r * row_stride;
                    for (int64_t c = 0; c < cols; ++c) {
                        w += snprintf(w, 27, "%.18e", (double)row[c]);
                        *w++ = (c + 1 < cols) ? ' ' : '\n';
                    }
                    if (cols == 0) *w++ = '\n';
                }
                o.resize((size_t)(w - o.data()));
            });
        }
        for (auto& x : th) x.join();
        for (int t = 0; t < nt && ok; ++t)
            if (!bufs[t].empty() && fwrite(bufs[t].data(), 1, bufs[t].size(), f) != bufs[t].size()) ok = false;
    }
    if (fclose(f) != 0) ok = false;
    return ok ? 0 : fail("nadm_savetxt_f32: write failed");
}
