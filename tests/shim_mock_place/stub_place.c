/* stub_place.c -- TEST STUB of the qsp_place_db calls for the CPU-only check of KeyFrameDatabaseHip: it appends everything it
 * receives to $QSP_STUB_DUMP and answers with a fixed pattern that makes the write-back visible.  It keeps the listed ids in add()
 * order; a query answers with every listed id that is not excluded, in that order, as lScoreAndMatch; accumulate answers with the
 * entries in REVERSE order as the candidates.  $QSP_STUB_FAIL=query / acc / put fails that call. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qsp_hip.h"

struct qsp_place_db { int64_t known[64], listed[64]; int n_known, n_listed; };
static struct qsp_place_db g_db;

const char* qsp_last_error(void) { return "injected by the test stub"; }

static int failing(const char* what) {
    const char* f = getenv("QSP_STUB_FAIL");
    return f && strcmp(f, what) == 0;
}
static FILE* dump(void) {
    const char* path = getenv("QSP_STUB_DUMP");
    return path ? fopen(path, "a") : NULL;
}
static int find(const int64_t* a, int n, int64_t id) {
    for (int i = 0; i < n; ++i) if (a[i] == id) return i;
    return -1;
}
static void drop(int64_t* a, int* n, int64_t id) {
    const int i = find(a, *n, id);
    if (i < 0) return;
    memmove(a + i, a + i + 1, sizeof(int64_t) * (size_t)(*n - i - 1));
    --*n;
}

int qsp_place_db_create(int device, int64_t words_hint, int32_t slots_hint, qsp_place_db** db) {
    FILE* d = dump();
    if (d) { fprintf(d, "create %d %lld %d\n", device, (long long)words_hint, slots_hint); fclose(d); }
    memset(&g_db, 0, sizeof(g_db));
    *db = &g_db;
    return QSP_OK;
}
void qsp_place_db_destroy(qsp_place_db* db) {
    FILE* d = dump();
    (void)db;
    if (d) { fprintf(d, "destroy\n"); fclose(d); }
}
int qsp_place_db_put(qsp_place_db* db, int64_t kf_id, int32_t n, const int32_t* word, const double* value, int32_t listed) {
    if (failing("put")) return QSP_ERR_DEVICE;
    FILE* d = dump();
    if (d) {
        fprintf(d, "put %lld %d %d\nword", (long long)kf_id, n, listed);
        for (int i = 0; i < n; ++i) fprintf(d, " %d", word[i]);
        fprintf(d, "\nvalue");
        for (int i = 0; i < n; ++i) fprintf(d, " %.17g", value[i]);
        fprintf(d, "\n");
        fclose(d);
    }
    if (find(db->known, db->n_known, kf_id) >= 0) return QSP_ERR_INVALID;
    db->known[db->n_known++] = kf_id;
    if (listed) db->listed[db->n_listed++] = kf_id;
    return QSP_OK;
}
int qsp_place_db_list(qsp_place_db* db, int64_t kf_id) {
    FILE* d = dump();
    if (d) { fprintf(d, "list %lld\n", (long long)kf_id); fclose(d); }
    if (find(db->known, db->n_known, kf_id) < 0 || find(db->listed, db->n_listed, kf_id) >= 0) return QSP_ERR_INVALID;
    db->listed[db->n_listed++] = kf_id;
    return QSP_OK;
}
int qsp_place_db_erase(qsp_place_db* db, int64_t kf_id) {
    FILE* d = dump();
    if (d) { fprintf(d, "erase %lld\n", (long long)kf_id); fclose(d); }
    drop(db->known, &db->n_known, kf_id);
    drop(db->listed, &db->n_listed, kf_id);
    return QSP_OK;
}
int qsp_place_db_clear(qsp_place_db* db) {
    FILE* d = dump();
    if (d) { fprintf(d, "clear\n"); fclose(d); }
    db->n_known = db->n_listed = 0;
    return QSP_OK;
}
int qsp_place_db_size(qsp_place_db* db, int32_t* known, int32_t* listed, int32_t* dead_slots, int64_t* device_bytes) {
    if (known) *known = db->n_known;
    if (listed) *listed = db->n_listed;
    if (dead_slots) *dead_slots = 0;
    if (device_bytes) *device_bytes = 0;
    return QSP_OK;
}
int qsp_place_db_query(qsp_place_db* db, const qsp_place_query_in* in, qsp_place_query_out* out) {
    if (failing("query")) return QSP_ERR_DEVICE;
    FILE* d = dump();
    if (d) {
        fprintf(d, "query %d %d %d %d %.9g %d\nword", in->mode, in->n, in->n_excluded, in->n_ref, in->min_score,
                out->sharing_id || out->sharing_common || out->sharing_first ? 1 : 0);
        for (int i = 0; i < in->n; ++i) fprintf(d, " %d", in->word[i]);
        fprintf(d, "\nvalue");
        for (int i = 0; i < in->n; ++i) fprintf(d, " %.17g", in->value[i]);
        fprintf(d, "\nexcluded");
        for (int i = 0; i < in->n_excluded; ++i) fprintf(d, " %lld", (long long)in->excluded[i]);
        fprintf(d, "\nref");
        for (int i = 0; i < in->n_ref; ++i) fprintf(d, " %lld", (long long)in->ref_id[i]);
        fprintf(d, "\n");
        fclose(d);
    }
    for (int i = 0; i < in->n_ref; ++i) if (find(db->known, db->n_known, in->ref_id[i]) < 0) return QSP_ERR_INVALID;
    int n = 0;
    for (int i = 0; i < db->n_listed; ++i) {
        if (in->mode == QSP_PLACE_LOOP && find(in->excluded, in->n_excluded, db->listed[i]) >= 0) continue;
        out->match_id[n] = db->listed[i];
        out->match_score[n] = 0.5f;
        ++n;
    }
    out->n_match = out->n_sharing = n;
    return QSP_OK;
}
int qsp_place_db_accumulate(qsp_place_db* db, int32_t mode, int32_t n, const int64_t* id, const int32_t* nbr_off, const int64_t* nbr_id,
                            qsp_place_acc_out* out) {
    (void)db;
    if (failing("acc")) return QSP_ERR_DEVICE;
    FILE* d = dump();
    if (d) {
        fprintf(d, "acc %d %d\nid", mode, n);
        for (int i = 0; i < n; ++i) fprintf(d, " %lld", (long long)id[i]);
        fprintf(d, "\noff");
        for (int i = 0; i <= n; ++i) fprintf(d, " %d", nbr_off[i]);
        fprintf(d, "\nnbr");
        for (int i = 0; i < nbr_off[n]; ++i) fprintf(d, " %lld", (long long)nbr_id[i]);
        fprintf(d, "\n");
        fclose(d);
    }
    for (int i = 0; i < n; ++i) out->cand_id[i] = id[n - 1 - i];
    out->n_cand = n;
    return QSP_OK;
}
