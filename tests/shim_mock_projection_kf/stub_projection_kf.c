/* stub_projection_kf.c -- TEST STUB of qsp_search_by_projection_kf for the CPU-only check of the relocalisation and Sim3 overloads of
 * OrbMatcherHip::SearchByProjection: it writes everything it receives to $QSP_STUB_DUMP and answers with the script in
 * $QSP_STUB_ANSWERS: lines `slot idx src` and `n_matches k` (every other slot: -1).  $QSP_STUB_FAIL=projection_kf fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

const char* qsp_last_error(void) { return "injected by the test stub"; }

static void floats(FILE* d, const char* name, const float* v, long n) {
    fprintf(d, "%s", name);
    for (long j = 0; v && j < n; ++j) fprintf(d, " %.9g", v[j]);
    fprintf(d, "\n");
}
static void bytes(FILE* d, const char* name, const uint8_t* v, long n) {
    fprintf(d, "%s", name);
    for (long j = 0; v && j < n; ++j) fprintf(d, " %d", v[j]);
    fprintf(d, "\n");
}
static void ints(FILE* d, const char* name, const int32_t* v, long n) {
    fprintf(d, "%s", name);
    for (long j = 0; v && j < n; ++j) fprintf(d, " %d", v[j]);
    fprintf(d, "\n");
}

int qsp_search_by_projection_kf(int device, const qsp_search_proj_kf_in* in, qsp_search_proj_kf_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "projection_kf") == 0) return QSP_ERR_DEVICE;
    const qsp_orb_frame* t = in->frame;
    const long n = t->n, ns = in->n_src;
    const char* path = getenv("QSP_STUB_DUMP");
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d\n", in->mode, in->n_src, t->n, in->check_orientation, in->orb_dist);
        fprintf(d, "frame %d %d %d\n", t->grid_cols, t->grid_rows, t->n_levels);
        const float g[8] = {t->min_x, t->max_x, t->min_y, t->max_y, t->grid_w_inv, t->grid_h_inv, t->log_scale, in->th};
        floats(d, "geom", g, 8);
        floats(d, "sf", t->scale_factors, t->n_levels);
        floats(d, "Rcw", t->Rcw, 9);
        floats(d, "tcw", t->tcw, 3);
        floats(d, "kp", t->kp, 2 * n);
        ints(d, "octave", t->octave, n);
        bytes(d, "desc", t->desc, 32 * n);
        floats(d, "K", in->K, 4);
        floats(d, "Ow", in->Ow, 3);
        bytes(d, "slot_blocked", in->slot_blocked, n);
        floats(d, "kp_angle", in->kp_angle, n);
        bytes(d, "src_valid", in->src_valid, ns);
        floats(d, "Xw", in->Xw, 3 * ns);
        bytes(d, "src_desc", in->desc, 32 * ns);
        floats(d, "dist_min_inv", in->dist_min_inv, ns);
        floats(d, "dist_max_inv", in->dist_max_inv, ns);
        floats(d, "dist_max", in->dist_max, ns);
        floats(d, "normal", in->normal, 3 * ns);
        floats(d, "src_angle", in->src_angle, ns);
        fclose(d);
    }
    for (long i = 0; i < ns; ++i) out->choice[i] = out->dist[i] = -1;
    for (long j = 0; j < n; ++j) out->slot_src[j] = -1;
    out->n_matches = 0; out->n_rounds = 1;
    const char* ans = getenv("QSP_STUB_ANSWERS");
    FILE* a = ans ? fopen(ans, "r") : NULL;
    if (a) {
        char key[32];
        while (fscanf(a, "%31s", key) == 1) {
            if (strcmp(key, "slot") == 0) {
                int idx, src;
                if (fscanf(a, "%d %d", &idx, &src) == 2 && idx >= 0 && idx < n) out->slot_src[idx] = src;
            } else if (strcmp(key, "n_matches") == 0) {
                int k;
                if (fscanf(a, "%d", &k) == 1) out->n_matches = k;
            }
        }
        fclose(a);
    }
    return QSP_OK;
}
