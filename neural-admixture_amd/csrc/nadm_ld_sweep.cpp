// The greedy sweep of LD pruning (include/nadm.h, nadm_ld_sweep): host code, no GPU.  It turns one range of the r^2 band
// (nadm_ld_band) into removals from the keep-list; the rule is stated in the header and restated line by line below.
#include <stdint.h>
#include "nadm_err.h"

using namespace nadm;

extern "C" int nadm_ld_sweep(const double* r2, int64_t m0, int64_t m1, int32_t W, int64_t M, const double* maf, const int32_t* chrom,
                             double thr, uint8_t* kept) {
    if (!r2 || !maf || !kept) return fail("nadm_ld_sweep: null pointer");
    if (W < 1 || W > NADM_LD_MAX_WINDOW) return fail("nadm_ld_sweep: W must be in 1..NADM_LD_MAX_WINDOW");
    if (M < 1 || m0 < 0 || m0 >= m1 || m1 > M) return fail("nadm_ld_sweep: need 0 <= m0 < m1 <= M");
    if (!(thr == thr)) return fail("nadm_ld_sweep: thr must be a number");
    for (int64_t i = m0; i < m1; ++i) {
        if (!kept[i]) continue;
        const double* row = r2 + (i - m0) * W;
        for (int64_t d = 0; d < W; ++d) {
            const int64_t j = i + 1 + d;
            if (j >= M) break;
            if (chrom && chrom[j] != chrom[i]) break;             // pairs across a chromosome boundary are never compared
            if (!kept[j]) continue;
            if (row[d] > thr) {
                if (maf[i] < maf[j]) {                            // i is the rarer one: it goes, and its row ends
                    kept[i] = 0;
                    break;
                }
                kept[j] = 0;                                      // j is the rarer one, or a tie
            }
        }
    }
    return 0;
}
