/* stub_triangulation.c -- TEST STUB of qsp_search_for_triangulation_batch for the CPU-only check of
 * OrbMatcherHip::SearchForTriangulationBatch: it appends everything it receives to $QSP_STUB_DUMP and answers with a fixed pattern
 * that makes the write-back visible: source slot i of neighbour c is matched with target (2 * i + c) % n_target when
 * i % 2 == c % 2, the slot is eligible and the target frame has key points; n_matches[c] = 100 + c.  $QSP_STUB_FAIL=tri fails. */
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

static void frame(FILE* d, const qsp_tri_frame* t) {
    const qsp_bow_frame* f = &t->bow;
    fprintf(d, "frame %d %d %d\n", f->n, f->n_nodes, f->eligible ? 1 : 0);
    fprintf(d, "desc");
    for (int j = 0; j < 32 * f->n; ++j) fprintf(d, " %d", f->desc[j]);
    fprintf(d, "\n");
    floats(d, "angle", f->angle, f->n);
    fprintf(d, "elig");
    for (int j = 0; f->eligible && j < f->n; ++j) fprintf(d, " %d", f->eligible[j]);
    fprintf(d, "\nnode_id");
    for (int j = 0; j < f->n_nodes; ++j) fprintf(d, " %d", f->node_id[j]);
    fprintf(d, "\nnode_off");
    for (int j = 0; j <= f->n_nodes; ++j) fprintf(d, " %d", f->node_off[j]);
    fprintf(d, "\nfeat");
    for (int j = 0; j < f->node_off[f->n_nodes]; ++j) fprintf(d, " %d", f->feat[j]);
    fprintf(d, "\n");
    floats(d, "xy", t->xy, 2 * f->n);
    fprintf(d, "stereo");
    for (int j = 0; j < f->n; ++j) fprintf(d, " %d", t->stereo[j]);
    fprintf(d, "\n");
    floats(d, "sigma2", t->sigma2, f->n);
    floats(d, "scale", t->scale, f->n);
}

int qsp_search_for_triangulation_batch(int device, const qsp_search_tri_in* in, qsp_search_tri_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "tri") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nc = in->n_cand;
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d\n", nc, in->th, in->only_stereo, in->check_orientation,
                out->match_raw || out->dist || out->hist || out->ind ? 1 : 0);
        floats(d, "F12", in->F12, 9 * nc);
        floats(d, "exy", in->exy, 2 * nc);
        frame(d, in->kf1);
        for (int c = 0; c < nc; ++c) frame(d, in->kf2 + c);
        fclose(d);
    }
    const qsp_bow_frame* S = &in->kf1->bow;
    int at = 0;
    for (int c = 0; c < nc; ++c) {
        const qsp_bow_frame* T = &in->kf2[c].bow;
        for (int i = 0; i < S->n; ++i) {
            const int hit = T->n > 0 && i % 2 == c % 2 && (!S->eligible || S->eligible[i]);
            out->match[at++] = hit ? (2 * i + c) % T->n : -1;
        }
        out->n_matches[c] = 100 + c;
    }
    return QSP_OK;
}
