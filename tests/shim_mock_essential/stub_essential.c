/* stub_essential.c -- TEST STUB of qsp_essential_graph_optimize for the CPU-only check of OptimizerHip::OptimizeEssentialGraph: it
 * appends everything it receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible: a free
 * vertex comes back with t + (1, 2, 3) and scale 2, a fixed one as it came; point p comes back as p + 0.5 (ref + 1) in x.
 * $QSP_STUB_FAIL=essential fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

int qsp_essential_graph_optimize(int device, int32_t n_kf, const double* S, const uint8_t* fixed, int32_t n_edge, const int32_t* v0,
                                 const int32_t* v1, const double* meas, int32_t fix_scale, int32_t n_iter, double lambda_init,
                                 int32_t n_pt, const double* P, const int32_t* ref, double* out, double* pout, qsp_essential_trace* tr) {
    (void)device; (void)tr;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "essential") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d %.17g\nS", n_kf, n_edge, n_pt, fix_scale, n_iter, lambda_init);
        for (int i = 0; i < 8 * n_kf; ++i) fprintf(d, " %.17g", S[i]);
        fprintf(d, "\nfixed");
        for (int i = 0; i < n_kf; ++i) fprintf(d, " %d", fixed[i]);
        fprintf(d, "\nv0");
        for (int i = 0; i < n_edge; ++i) fprintf(d, " %d", v0[i]);
        fprintf(d, "\nv1");
        for (int i = 0; i < n_edge; ++i) fprintf(d, " %d", v1[i]);
        fprintf(d, "\nmeas");
        for (int i = 0; i < 8 * n_edge; ++i) fprintf(d, " %.17g", meas[i]);
        fprintf(d, "\nP");
        for (int i = 0; i < 3 * n_pt; ++i) fprintf(d, " %.17g", P[i]);
        fprintf(d, "\nref");
        for (int i = 0; i < n_pt; ++i) fprintf(d, " %d", ref[i]);
        fprintf(d, "\n");
        fclose(d);
    }
    for (int v = 0; v < n_kf; ++v) {
        memcpy(out + 8 * v, S + 8 * v, 64);
        if (fixed[v]) continue;
        for (int i = 0; i < 3; ++i) out[8 * v + i] += i + 1;
        out[8 * v + 7] = 2.0;
    }
    for (int p = 0; p < n_pt; ++p) {
        memcpy(pout + 3 * p, P + 3 * p, 24);
        pout[3 * p] += 0.5 * (ref[p] + 1);
    }
    return QSP_OK;
}
