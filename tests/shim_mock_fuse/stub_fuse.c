/* stub_fuse.c -- TEST STUB of qsp_fuse_batch for the CPU-only check of OrbMatcherHip::FuseBatch: it appends everything it receives
 * to $QSP_STUB_DUMP and answers with the script in $QSP_STUB_ANSWERS: lines `target position best_idx best_dist` for the listed
 * pairs that match (every other pair: -1 -1).  $QSP_STUB_FAIL=fuse fails. */
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

int qsp_fuse_batch(int device, const qsp_fuse_in* in, qsp_fuse_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "fuse") == 0) return QSP_ERR_DEVICE;
    const int nt = in->n_target;
    const char* path = getenv("QSP_STUB_DUMP");
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d\n", nt, in->n_point, out->reason || out->level ? 1 : 0);
        floats(d, "K", in->K, 5L * nt);
        floats(d, "Ow", in->Ow, 3L * nt);
        floats(d, "th", in->th, nt);
        floats(d, "inv_level_sigma2", in->inv_level_sigma2, 16L * nt);
        fprintf(d, "check");
        for (int k = 0; k < nt; ++k) fprintf(d, " %d", in->check_reprojection[k]);
        fprintf(d, "\nu_right_off");
        for (int k = 0; k <= nt; ++k) fprintf(d, " %d", in->u_right_off[k]);
        fprintf(d, "\n");
        floats(d, "u_right", in->u_right, in->u_right_off[nt]);
        fprintf(d, "list_off");
        for (int k = 0; k <= nt; ++k) fprintf(d, " %lld", (long long)in->list_off[k]);
        fprintf(d, "\nlist_idx");
        for (long j = 0; j < in->list_off[nt]; ++j) fprintf(d, " %d", in->list_idx[j]);
        fprintf(d, "\n");
        floats(d, "Xw", in->Xw, 3L * in->n_point);
        floats(d, "normal", in->normal, 3L * in->n_point);
        floats(d, "dist_min_inv", in->dist_min_inv, in->n_point);
        floats(d, "dist_max_inv", in->dist_max_inv, in->n_point);
        floats(d, "dist_max", in->dist_max, in->n_point);
        fprintf(d, "pool_desc");
        for (long j = 0; j < 32L * in->n_point; ++j) fprintf(d, " %d", in->desc[j]);
        fprintf(d, "\n");
        for (int k = 0; k < nt; ++k) {
            const qsp_orb_frame* t = in->target + k;
            fprintf(d, "frame %d %d %d %d %d\n", t->n, t->grid_cols, t->grid_rows, t->n_levels, t->has_point ? 1 : 0);
            const float g[8] = {t->min_x, t->max_x, t->min_y, t->max_y, t->grid_w_inv, t->grid_h_inv, t->log_scale, 0.f};
            floats(d, "geom", g, 7);
            floats(d, "sf", t->scale_factors, t->n_levels);
            floats(d, "Rcw", t->Rcw, 9);
            floats(d, "tcw", t->tcw, 3);
            floats(d, "kp", t->kp, 2L * t->n);
            fprintf(d, "octave");
            for (int j = 0; j < t->n; ++j) fprintf(d, " %d", t->octave[j]);
            fprintf(d, "\ndesc");
            for (int j = 0; j < 32 * t->n; ++j) fprintf(d, " %d", t->desc[j]);
            fprintf(d, "\n");
        }
        fclose(d);
    }
    const long n_pair = (long)in->list_off[nt];
    for (long j = 0; j < n_pair; ++j) out->best_idx[j] = out->best_dist[j] = -1;
    const char* ans = getenv("QSP_STUB_ANSWERS");
    FILE* a = ans ? fopen(ans, "r") : NULL;
    if (a) {
        int k, pos, best, dist;
        while (fscanf(a, "%d %d %d %d", &k, &pos, &best, &dist) == 4)
            if (k >= 0 && k < nt && pos >= 0 && in->list_off[k] + pos < in->list_off[k + 1]) {
                out->best_idx[in->list_off[k] + pos] = best;
                out->best_dist[in->list_off[k] + pos] = dist;
            }
        fclose(a);
    }
    return QSP_OK;
}
