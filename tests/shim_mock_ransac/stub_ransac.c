/* stub_ransac.c -- TEST STUB of qsp_sim3_ransac_batch for the CPU-only check of Sim3SolverHip::FindBatch: it appends everything it
 * receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible.  Candidate c succeeds at
 * iteration min(table[c % 5], n_its[c]) with table = 6 3 9 5 1 (never when n_its[c] == 0); its matches at even positions are
 * inliers; R = c + 0.25 i, t = 10 c + i, s = 1 + c.  $QSP_STUB_FAIL=ransac fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

const char* qsp_last_error(void) { return "injected by the test stub"; }

int qsp_sim3_ransac_batch(int device, int32_t n_cand, const int32_t* off, const int32_t* n_its, const int32_t* toff, const int32_t* tri,
                          const float* K1, const float* K2, const float* X1, const float* X2, const float* s1, const float* s2,
                          int32_t min_inliers, int32_t fix_scale, int32_t* first_it, float* R, float* t, float* s, uint8_t* inlier,
                          int32_t* n_in, int32_t* hyp) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "ransac") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nm = off[n_cand], nt = toff[n_cand];
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d %d", n_cand, nm, nt, min_inliers, fix_scale, hyp ? 1 : 0);
        const int32_t* ia[4] = {off, n_its, toff, tri};
        const char* in_[4] = {"off", "its", "toff", "tri"};
        const int iw[4] = {n_cand + 1, n_cand, n_cand + 1, 3 * nt};
        for (int k = 0; k < 4; ++k) {
            fprintf(d, "\n%s", in_[k]);
            for (int j = 0; j < iw[k]; ++j) fprintf(d, " %d", ia[k][j]);
        }
        const float* a[6] = {K1, K2, X1, X2, s1, s2};
        const char* nm_[6] = {"K1", "K2", "X1", "X2", "s1", "s2"};
        const int w[6] = {4 * n_cand, 4 * n_cand, 3 * nm, 3 * nm, nm, nm};
        for (int k = 0; k < 6; ++k) {
            fprintf(d, "\n%s", nm_[k]);
            for (int j = 0; j < w[k]; ++j) fprintf(d, " %.9g", a[k][j]);
        }
        fprintf(d, "\n");
        fclose(d);
    }
    static const int table[5] = {6, 3, 9, 5, 1};
    for (int c = 0; c < n_cand; ++c) {
        const int n = off[c + 1] - off[c];
        const int hit = n_its[c] == 0 ? 0 : (table[c % 5] < n_its[c] ? table[c % 5] : n_its[c]);
        first_it[c] = hit;
        n_in[c] = 0;
        for (int e = 0; e < n; ++e) {
            inlier[off[c] + e] = hit && e % 2 == 0;
            n_in[c] += hit && e % 2 == 0;
        }
        for (int i = 0; i < 9; ++i) R[9 * c + i] = hit ? c + 0.25f * i : 0.f;
        for (int i = 0; i < 3; ++i) t[3 * c + i] = hit ? 10.f * c + i : 0.f;
        s[c] = hit ? 1.f + c : 0.f;
    }
    return QSP_OK;
}
