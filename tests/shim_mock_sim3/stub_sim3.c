/* stub_sim3.c -- TEST STUB of qsp_sim3_optimize_batch for the CPU-only check of OptimizerHip::OptimizeSim3(Batch): it appends
 * everything it receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible.  Per candidate:
 * the pair at position e of the candidate is dropped when e % 3 == 1; fewer than 12 matches is "the early return" (0 inliers,
 * Sim3 as it came, no second pass), otherwise tx += 0.5, s *= 2 and the survivors are counted.  $QSP_STUB_FAIL=sim3 fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

int qsp_sim3_optimize_batch(int device, int32_t n_cand, const int32_t* off, const double* K1, const double* K2, const double* S,
                            const double* P1, const double* P2, const double* o1, const double* o2, const double* i1,
                            const double* i2, double th2, int32_t fix_scale, double* out, uint8_t* inlier, int32_t* n_in,
                            qsp_sim3_trace* tr) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "sim3") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nm = off[n_cand];
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %.17g %d\noff", n_cand, nm, th2, fix_scale);
        for (int c = 0; c <= n_cand; ++c) fprintf(d, " %d", off[c]);
        const double* a[9] = {K1, K2, S, P1, P2, o1, o2, i1, i2};
        const char* nm_[9] = {"K1", "K2", "S", "P1", "P2", "o1", "o2", "i1", "i2"};
        const int w[9] = {4 * n_cand, 4 * n_cand, 8 * n_cand, 3 * nm, 3 * nm, 2 * nm, 2 * nm, nm, nm};
        for (int k = 0; k < 9; ++k) {
            fprintf(d, "\n%s", nm_[k]);
            for (int j = 0; j < w[k]; ++j) fprintf(d, " %.17g", a[k][j]);
        }
        fprintf(d, "\n");
        fclose(d);
    }
    for (int c = 0; c < n_cand; ++c) {
        const int n = off[c + 1] - off[c];
        int kept = 0;
        for (int e = 0; e < n; ++e) { inlier[off[c] + e] = (e % 3 != 1); kept += (e % 3 != 1); }
        memcpy(out + 8 * c, S + 8 * c, 64);
        memset(&tr[c], 0, sizeof(tr[c]));
        tr[c].iters[0] = 5;
        if (n < 12) { n_in[c] = 0; continue; }
        out[8 * c] += 0.5; out[8 * c + 7] *= 2;
        tr[c].iters[1] = 4;
        n_in[c] = kept;
    }
    return QSP_OK;
}
