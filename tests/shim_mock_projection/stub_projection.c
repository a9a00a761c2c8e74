/* stub_projection.c -- TEST STUB of qsp_search_by_projection for the CPU-only check of OrbMatcherHip::SearchLocalPoints and
 * OrbMatcherHip::SearchByProjection: it writes everything it receives to $QSP_STUB_DUMP and answers with the script in
 * $QSP_STUB_ANSWERS: lines `src i in_view proj_x proj_y proj_xr level view_cos`, `slot idx src` and `n_matches k` (every other
 * source: not in view; every other slot: -1).  $QSP_STUB_FAIL=projection fails. */
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

int qsp_search_by_projection(int device, const qsp_search_proj_in* in, qsp_search_proj_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "projection") == 0) return QSP_ERR_DEVICE;
    const qsp_orb_frame* t = in->frame;
    const long n = t->n, ns = in->n_src;
    const char* path = getenv("QSP_STUB_DUMP");
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d\n", in->mode, in->n_src, t->n, in->check_orientation, in->mono);
        fprintf(d, "frame %d %d %d %d\n", t->grid_cols, t->grid_rows, t->n_levels, t->has_point ? 1 : 0);
        const float g[7] = {t->min_x, t->max_x, t->min_y, t->max_y, t->grid_w_inv, t->grid_h_inv, t->log_scale};
        floats(d, "geom", g, 7);
        floats(d, "sf", t->scale_factors, t->n_levels);
        floats(d, "Rcw", t->Rcw, 9);
        floats(d, "tcw", t->tcw, 3);
        floats(d, "kp", t->kp, 2 * n);
        ints(d, "octave", t->octave, n);
        bytes(d, "desc", t->desc, 32 * n);
        floats(d, "K", in->K, 5);
        floats(d, "Ow", in->Ow, 3);
        const float o[4] = {in->mb, in->th, in->nn_ratio, in->view_cos_limit};
        floats(d, "opt", o, 4);
        floats(d, "last_Rcw", in->last_Rcw, 9);
        floats(d, "last_tcw", in->last_tcw, 3);
        floats(d, "u_right", in->u_right, n);
        bytes(d, "slot_blocked", in->slot_blocked, n);
        floats(d, "kp_angle", in->kp_angle, n);
        bytes(d, "src_valid", in->src_valid, ns);
        bytes(d, "src_blocks", in->src_blocks, ns);
        floats(d, "Xw", in->Xw, 3 * ns);
        bytes(d, "src_desc", in->desc, 32 * ns);
        floats(d, "normal", in->normal, 3 * ns);
        floats(d, "dist_min_inv", in->dist_min_inv, ns);
        floats(d, "dist_max_inv", in->dist_max_inv, ns);
        floats(d, "dist_max", in->dist_max, ns);
        ints(d, "src_octave", in->src_octave, ns);
        floats(d, "src_angle", in->src_angle, ns);
        fclose(d);
    }
    for (long i = 0; i < ns; ++i) {
        out->choice[i] = out->dist[i] = -1;
        if (in->mode == 0) { out->in_view[i] = 0; out->proj_x[i] = out->proj_y[i] = out->proj_xr[i] = out->view_cos[i] = 0.f; out->level[i] = 0; }
    }
    for (long j = 0; j < n; ++j) out->slot_src[j] = -1;
    out->n_matches = 0; out->n_rounds = 1;
    const char* ans = getenv("QSP_STUB_ANSWERS");
    FILE* a = ans ? fopen(ans, "r") : NULL;
    if (a) {
        char key[32];
        while (fscanf(a, "%31s", key) == 1) {
            if (strcmp(key, "src") == 0) {
                int i, v, l; float x, y, xr, c;
                if (fscanf(a, "%d %d %f %f %f %d %f", &i, &v, &x, &y, &xr, &l, &c) != 7) break;
                if (in->mode == 0 && i >= 0 && i < ns) { out->in_view[i] = (uint8_t)v; out->proj_x[i] = x; out->proj_y[i] = y; out->proj_xr[i] = xr; out->level[i] = l; out->view_cos[i] = c; }
            } else if (strcmp(key, "slot") == 0) {
                int j, s;
                if (fscanf(a, "%d %d", &j, &s) != 2) break;
                if (j >= 0 && j < n) out->slot_src[j] = s;
            } else if (strcmp(key, "n_matches") == 0) {
                int k;
                if (fscanf(a, "%d", &k) != 1) break;
                out->n_matches = k;
            }
        }
        fclose(a);
    }
    return QSP_OK;
}
