/* stub_bow.c -- TEST STUB of qsp_search_by_bow_batch for the CPU-only check of OrbMatcherHip::SearchByBoWBatch: it appends
 * everything it receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible: source slot i of
 * candidate c is matched with target (2 * i + c) % n_target when i % 2 == c % 2, the slot is eligible and the target frame has key
 * points; n_matches[c] = 100 + c.  $QSP_STUB_FAIL=bow fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

const char* qsp_last_error(void) { return "injected by the test stub"; }

static void frame(FILE* d, const qsp_bow_frame* f) {
    fprintf(d, "frame %d %d %d\n", f->n, f->n_nodes, f->eligible ? 1 : 0);
    fprintf(d, "desc");
    for (int j = 0; j < 32 * f->n; ++j) fprintf(d, " %d", f->desc[j]);
    fprintf(d, "\nangle");
    for (int j = 0; j < f->n; ++j) fprintf(d, " %.9g", f->angle[j]);
    fprintf(d, "\nelig");
    for (int j = 0; f->eligible && j < f->n; ++j) fprintf(d, " %d", f->eligible[j]);
    fprintf(d, "\nnode_id");
    for (int j = 0; j < f->n_nodes; ++j) fprintf(d, " %d", f->node_id[j]);
    fprintf(d, "\nnode_off");
    for (int j = 0; j <= f->n_nodes; ++j) fprintf(d, " %d", f->node_off[j]);
    fprintf(d, "\nfeat");
    for (int j = 0; j < f->node_off[f->n_nodes]; ++j) fprintf(d, " %d", f->feat[j]);
    fprintf(d, "\n");
}

int qsp_search_by_bow_batch(int device, const qsp_search_bow_in* in, qsp_search_bow_out* out) {
    (void)device;
    const char* f = getenv("QSP_STUB_FAIL");
    if (f && strcmp(f, "bow") == 0) return QSP_ERR_DEVICE;
    const char* path = getenv("QSP_STUB_DUMP");
    const int nc = in->n_cand;
    if (path) {
        FILE* d = fopen(path, "a");
        fprintf(d, "call %d %d %d %d %d %d\n", nc, in->shared_is_source, in->th, in->th_inclusive, in->check_orientation,
                out->match_raw || out->dist || out->hist || out->ind ? 1 : 0);
        fprintf(d, "nn %.9g\n", in->nn_ratio);
        frame(d, in->shared);
        for (int c = 0; c < nc; ++c) frame(d, in->cand + c);
        fclose(d);
    }
    int at = 0;
    for (int c = 0; c < nc; ++c) {
        const qsp_bow_frame* S = in->shared_is_source ? in->shared : in->cand + c;
        const qsp_bow_frame* T = in->shared_is_source ? in->cand + c : in->shared;
        for (int i = 0; i < S->n; ++i) {
            const int hit = T->n > 0 && i % 2 == c % 2 && (!S->eligible || S->eligible[i]);
            out->match[at++] = hit ? (2 * i + c) % T->n : -1;
        }
        out->n_matches[c] = 100 + c;
    }
    return QSP_OK;
}
