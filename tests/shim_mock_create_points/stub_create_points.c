/* stub_create_points.c -- TEST STUB of qsp_create_new_map_points_batch and qsp_triangulate_batch for the CPU-only check of
 * OrbMatcherHip::CreateNewMapPointsBatch / TriangulateBatch: it appends what it receives to $QSP_STUB_DUMP and answers with a fixed
 * pattern that makes the write-back visible.  The chained call matches source slot i of neighbour c with target (2 * i + c) % n
 * when i % 2 == c % 2, the slot is eligible and the neighbour has key points (the pattern of tests/shim_mock_triangulation), and
 * n_matches[c] = 100 + c.  Both calls mark a matched slot `first` unless i % 3 == 2 and answer x3D = (k + 0.5, i + 0.25,
 * idx2 + 0.125).  $QSP_STUB_FAIL=create / =tri fails the call. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

const char* qsp_last_error(void) { return "injected by the test stub"; }

static void floats(FILE* d, const char* name, const float* v, int n) {
    fprintf(d, "%s", name);
    for (int j = 0; v && j < n; ++j) fprintf(d, " %.9g", v[j]);
    fprintf(d, "\n");
}

static void geometry(FILE* d, const qsp_triangulate_geom* g) {
    fprintf(d, "geom %d %.9g\n", g->n_cand, g->ratio_factor);
    for (int f = 0; f <= g->n_cand; ++f) {
        const qsp_triangulate_frame* F = f ? g->kf2 + (f - 1) : g->kf1;
        const float K[8] = {F->fx, F->fy, F->cx, F->cy, F->invfx, F->invfy, F->mb, F->mbf};
        fprintf(d, "gframe %d\n", F->n);
        floats(d, "Rcw", F->Rcw, 9); floats(d, "tcw", F->tcw, 3); floats(d, "Ow", F->Ow, 3); floats(d, "K", K, 8);
        floats(d, "xy_un", F->xy_un, 2 * F->n); floats(d, "xy", F->xy, 2 * F->n); floats(d, "u_right", F->u_right, F->n);
        floats(d, "depth", F->depth, F->n); floats(d, "sigma2", F->sigma2, F->n); floats(d, "scale", F->scale, F->n);
    }
}

static void answer(const qsp_triangulate_geom* g, const int32_t* match, qsp_triangulate_out* out) {
    const int n1 = g->kf1->n;
    for (int k = 0; k < g->n_cand; ++k) {
        out->n_new[k] = 0;
        for (int i = 0; i < n1; ++i) {
            const int s = k * n1 + i, hit = match[s] >= 0;
            out->accept[s] = hit;
            out->first[s] = hit && i % 3 != 2;
            out->n_new[k] += out->first[s];
            out->x3D[3 * s] = k + 0.5f; out->x3D[3 * s + 1] = i + 0.25f; out->x3D[3 * s + 2] = match[s] + 0.125f;
        }
    }
}

static int taps(const qsp_triangulate_out* o) { return o->reason || o->path || o->cos_rays || o->z || o->err2 || o->ratio_dist; }

int qsp_create_new_map_points_batch(int device, const qsp_search_tri_in* in, const qsp_triangulate_geom* geom, qsp_search_tri_out* sout,
                                    qsp_triangulate_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "create") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nc = in->n_cand;
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call create %d %d %d %d %d\n", nc, in->th, in->only_stereo, in->check_orientation,
                (sout->match_raw || sout->dist || sout->hist || sout->ind || taps(out)) ? 1 : 0);
        floats(d, "F12", in->F12, 9 * nc);
        floats(d, "exy", in->exy, 2 * nc);
        fprintf(d, "search_n %d", in->kf1->bow.n);
        for (int c = 0; c < nc; ++c) fprintf(d, " %d", in->kf2[c].bow.n);
        fprintf(d, "\n");
        geometry(d, geom);
        fclose(d);
    }
    const qsp_bow_frame* S = &in->kf1->bow;
    int at = 0;
    for (int c = 0; c < nc; ++c) {
        const qsp_bow_frame* T = &in->kf2[c].bow;
        for (int i = 0; i < S->n; ++i) {
            const int hit = T->n > 0 && i % 2 == c % 2 && (!S->eligible || S->eligible[i]);
            sout->match[at++] = hit ? (2 * i + c) % T->n : -1;
        }
        sout->n_matches[c] = 100 + c;
    }
    answer(geom, sout->match, out);
    return QSP_OK;
}

int qsp_triangulate_batch(int device, const qsp_triangulate_geom* geom, const int32_t* match, qsp_triangulate_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "tri") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call tri %d 0 0 0 %d\n", geom->n_cand, taps(out));
        fprintf(d, "match");
        for (int j = 0; j < geom->n_cand * geom->kf1->n; ++j) fprintf(d, " %d", match[j]);
        fprintf(d, "\n");
        geometry(d, geom);
        fclose(d);
    }
    answer(geom, match, out);
    return QSP_OK;
}
