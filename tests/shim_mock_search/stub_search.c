/* stub_search.c -- TEST STUB of qsp_search_by_sim3_batch for the CPU-only check of OrbMatcherHip::SearchBySim3Batch: it appends
 * everything it receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible: slot i1 of candidate
 * c is matched with key point (i1 + c) % n2 when i1 % 3 == c % 3, pre1 is not set and key frame 2 has key points.
 * $QSP_STUB_FAIL=search fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

const char* qsp_last_error(void) { return "injected by the test stub"; }

static void floats(FILE* d, const char* name, const float* a, int n) {
    fprintf(d, "%s", name);
    for (int j = 0; j < n; ++j) fprintf(d, " %.9g", a[j]);
    fprintf(d, "\n");
}
static void bytes(FILE* d, const char* name, const uint8_t* a, int n) {
    fprintf(d, "%s", name);
    for (int j = 0; j < n; ++j) fprintf(d, " %d", a[j]);
    fprintf(d, "\n");
}
static void frame(FILE* d, const qsp_orb_frame* f) {
    fprintf(d, "frame %d %d %d %d\n", f->n, f->grid_cols, f->grid_rows, f->n_levels);
    const float par[7] = {f->min_x, f->max_x, f->min_y, f->max_y, f->grid_w_inv, f->grid_h_inv, f->log_scale};
    floats(d, "par", par, 7);
    floats(d, "sf", f->scale_factors, f->n_levels);
    floats(d, "Rcw", f->Rcw, 9);
    floats(d, "tcw", f->tcw, 3);
    floats(d, "kp", f->kp, 2 * f->n);
    fprintf(d, "octave");
    for (int j = 0; j < f->n; ++j) fprintf(d, " %d", f->octave[j]);
    fprintf(d, "\n");
    bytes(d, "desc", f->desc, 32 * f->n);
    bytes(d, "has", f->has_point, f->n);
    floats(d, "Xw", f->Xw, 3 * f->n);
    floats(d, "dmin", f->dist_min_inv, f->n);
    floats(d, "dmaxi", f->dist_max_inv, f->n);
    floats(d, "dmax", f->dist_max, f->n);
    bytes(d, "mpd", f->mp_desc, 32 * f->n);
}

int qsp_search_by_sim3_batch(int device, const qsp_search_sim3_in* in, qsp_search_sim3_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "search") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nc = in->n_cand, n1 = in->kf1->n;
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d\n", nc, n1, out->best1 || out->dist1 || out->best2 || out->dist2 ? 1 : 0);
        fprintf(d, "off2");
        for (int c = 0; c <= nc; ++c) fprintf(d, " %d", in->off2[c]);
        fprintf(d, "\n");
        floats(d, "K", in->K, 4 * nc);
        floats(d, "s12", in->s12, nc);
        floats(d, "R12", in->R12, 9 * nc);
        floats(d, "t12", in->t12, 3 * nc);
        floats(d, "th", in->th, nc);
        bytes(d, "pre1", in->pre1, nc * n1);
        bytes(d, "pre2", in->pre2, in->off2[nc]);
        frame(d, in->kf1);
        for (int c = 0; c < nc; ++c) frame(d, in->kf2 + c);
        fclose(d);
    }
    for (int c = 0; c < nc; ++c) {
        const int n2 = in->kf2[c].n;
        out->n_found[c] = 0;
        for (int i1 = 0; i1 < n1; ++i1) {
            const int hit = n2 > 0 && i1 % 3 == c % 3 && !in->pre1[c * n1 + i1];
            out->match12[c * n1 + i1] = hit ? (i1 + c) % n2 : -1;
            out->n_found[c] += hit;
        }
    }
    return QSP_OK;
}
