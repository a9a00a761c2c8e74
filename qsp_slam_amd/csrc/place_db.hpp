// place_db.hpp -- place recognition against a key-frame database that is resident on the device: KeyFrameDatabase::
// DetectLoopCandidates / DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:76-309), the minimum-score loop of
// LoopClosing::DetectLoop (src/LoopClosing.cc:131-148) and DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:
// 23-68).  Compiled in c_abi.cpp; the rules are spelled out in include/qsp_hip.h.
//
// The reference walks an inverted file (one std::list<KeyFrame*> per word of the query).  Here there is none: a key frame is a
// SLOT with its sorted word list in one arena, and ONE WAVE owns one slot.  Its lanes stride over the slot's words and binary-search
// the query's; a ballot per 64 words gives the size of the intersection and the first common word.  The reference's discovery
// order of lKFsSharingWords -- query words ascending, each word's list in add() order -- is ascending (first common word, list
// sequence number), so one workgroup ranks the sharing slots by that 64-bit key (rank by counting, no size cap).
//
// Score: the terms fabs(vi - wi) - fabs(vi) - fabs(wi) of a 64-word chunk sit in the lanes that found them; every lane then adds
// them IN WORD ORDER, reading lane after lane of the ballot with a shuffle, so the double sum is the serial one of the reference and
// not a tree.  No products anywhere; contraction is OFF all the same.
//
// No path has a size threshold: the query's words are searched in global memory (they stay in L2), whatever their number.
#pragma once
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <unordered_map>
#include <vector>

#include "orb_match.hpp"
#include "staging.hpp"
#include "wave.hpp"

namespace qsp {
namespace place {

constexpr int32_t NO_WORD = 0x7fffffff;

struct Meta {                          // uploaded from the host's mirror
    int64_t off, kf_id;                // its words are [off, off + n) of the arena
    int32_t n, listed;
    uint32_t seq;                      // the order of the add() calls
    int32_t alive;
};
struct State {                         // the device's own: mnLoopQuery mnLoopWords mLoopScore, mnRelocQuery mnRelocWords mRelocScore
    int32_t loop_stamp, loop_words;
    float loop_score;
    int32_t reloc_stamp, reloc_words;
    float reloc_score;
};
struct Head {
    int32_t n_sharing, max_common, min_common, n_match;
    float min_score;
    int32_t n_cand, pad0, pad1;
};

__device__ inline int min_common_of(int max_common) {
#pragma clang fp contract(off)
    return (int)((float)max_common * 0.8f);                  // `int minCommonWords = maxCommonWords*0.8f;`
}

__global__ void k_place_mark(const int32_t* __restrict__ slot, int32_t n, uint8_t* __restrict__ flag) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[slot[i]] = 1;
}

// 4 waves per workgroup, one wave per slot: the size of the intersection and the first common word
__global__ __launch_bounds__(256) void k_place_common(const Meta* __restrict__ meta, State* __restrict__ state, const int32_t* __restrict__ word,
                                                      int32_t n_slots, const int32_t* __restrict__ qword, int32_t nq, int32_t mode, int32_t stamp,
                                                      const uint8_t* __restrict__ excluded, int32_t* __restrict__ common,
                                                      int32_t* __restrict__ first, Head* head) {
    const int lane = threadIdx.x & 63;
    const int32_t s = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (s >= n_slots) return;
    const Meta m = meta[s];
    int cnt = 0;
    int32_t fw = NO_WORD;
    if (m.alive && m.listed && !(excluded && excluded[s])) {          // wave-uniform
        const int32_t* kw = word + m.off;
        for (int32_t base = 0; base < m.n; base += 64) {
            const int32_t j = base + lane;
            bool hit = false;
            int32_t w = NO_WORD;
            if (j < m.n) {
                w = kw[j];
                const int32_t a = orb::lower_bound_id(qword, nq, w);
                hit = a < nq && qword[a] == w;
            }
            const unsigned long long b = __ballot(hit);
            if (b) {
                if (cnt == 0) fw = (int32_t)wave_min(hit ? (unsigned long long)w : (unsigned long long)NO_WORD);
                cnt += __popcll(b);
            }
        }
    }
    if (lane == 0) {
        common[s] = cnt;
        first[s] = fw;
        if (cnt) {
            if (mode == QSP_PLACE_LOOP) { state[s].loop_stamp = stamp; state[s].loop_words = cnt; }
            else { state[s].reloc_stamp = stamp; state[s].reloc_words = cnt; }
            atomicMax(&head->max_common, cnt);
        }
    }
}

// One wave per item.  item_slot == NULL: item = slot, scored when its common words are > minCommonWords, and the score is stored in
// the slot's state.  item_slot != NULL (the refs of DetectLoop's minimum): every item is scored, no state is touched.
__global__ __launch_bounds__(256) void k_place_score(const Meta* __restrict__ meta, State* __restrict__ state, const int32_t* __restrict__ word,
                                                     const double* __restrict__ value, const int32_t* __restrict__ qword,
                                                     const double* __restrict__ qvalue, int32_t nq, const int32_t* __restrict__ item_slot,
                                                     int32_t n_items, const int32_t* __restrict__ common, const Head* __restrict__ head,
                                                     int32_t mode, float* __restrict__ score_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int32_t it = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (it >= n_items) return;
    const int32_t s = item_slot ? item_slot[it] : it;
    if (!item_slot && !(common[it] > min_common_of(head->max_common))) return;
    const Meta m = meta[s];
    const int32_t* kw = word + m.off;
    const double* kv = value + m.off;
    double score = 0;
    for (int32_t base = 0; base < m.n; base += 64) {
        const int32_t j = base + lane;
        bool hit = false;
        double term = 0;
        if (j < m.n) {
            const int32_t w = kw[j];
            const int32_t a = orb::lower_bound_id(qword, nq, w);
            if (a < nq && qword[a] == w) {
                hit = true;
                const double vi = qvalue[a], wi = kv[j];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        for (unsigned long long b = __ballot(hit); b; b &= b - 1)     // ascending lane = ascending word: the reference's serial sum
            score += __shfl(term, __ffsll((long long)b) - 1, 64);
    }
    score = -score / 2.0;
    const float si = (float)score;
    if (lane == 0) {
        score_out[it] = si;
        if (!item_slot) {
            if (mode == QSP_PLACE_LOOP) state[s].loop_score = si; else state[s].reloc_score = si;
        }
    }
}

// One workgroup: DetectLoop's minimum score, then lKFsSharingWords and lScoreAndMatch in the reference's order
__global__ __launch_bounds__(1024) void k_place_order(const Meta* __restrict__ meta, int32_t n_slots, const int32_t* __restrict__ common,
                                                      const int32_t* __restrict__ first, const float* __restrict__ score, Head* head,
                                                      int32_t mode, float given_min, const float* __restrict__ ref_score, int32_t n_ref,
                                                      int32_t* list, unsigned long long* key, uint8_t* kept, int64_t* sharing_id,
                                                      int32_t* sharing_common, int32_t* sharing_first, int64_t* match_id, float* match_score,
                                                      int32_t* last_slot, float* last_score) {
    __shared__ int n_sh, n_kept, s_minc;
    __shared__ float s_min;
    __shared__ unsigned long long t_key[1024];
    __shared__ uint8_t t_kept[1024];
    const int tid = threadIdx.x;
    if (tid == 0) {
        n_sh = 0;
        n_kept = 0;
        float m = given_min;
        if (n_ref > 0) {
            m = 1.0f;                                                  // LoopClosing.cc:136-148
            for (int32_t i = 0; i < n_ref; ++i)
                if (ref_score[i] < m) m = ref_score[i];
        }
        s_min = m;
        s_minc = min_common_of(head->max_common);
    }
    __syncthreads();
    const int minc = s_minc;
    const float min_score = s_min;
    for (int32_t s = tid; s < n_slots; s += 1024) {
        const int32_t c = common[s];
        if (c <= 0) continue;
        const int p = atomicAdd(&n_sh, 1);
        list[p] = s;
        key[p] = ((unsigned long long)(uint32_t)first[s] << 32) | meta[s].seq;
        const bool k = c > minc && (mode == QSP_PLACE_RELOC || score[s] >= min_score);
        kept[p] = k ? 1 : 0;
        if (k) atomicAdd(&n_kept, 1);
    }
    __syncthreads();
    // rank by counting, the keys of 1024 entries at a time staged in LDS; every loop bound depends on n alone, so the barriers are
    // reached by all threads
    const int n = n_sh;
    for (int ib = 0; ib < n; ib += 1024) {
        const int i = ib + tid;
        const unsigned long long ki = i < n ? key[i] : 0ull;
        int r = 0, rk = 0;
        for (int jb = 0; jb < n; jb += 1024) {
            __syncthreads();
            if (jb + tid < n) { t_key[tid] = key[jb + tid]; t_kept[tid] = kept[jb + tid]; }
            __syncthreads();
            const int m = n - jb < 1024 ? n - jb : 1024;
            for (int j = 0; j < m; ++j) {
                const bool lt = t_key[j] < ki;
                r += lt ? 1 : 0;
                rk += (lt && t_kept[j]) ? 1 : 0;
            }
        }
        if (i >= n) continue;
        const int32_t s = list[i];
        sharing_id[r] = meta[s].kf_id;
        sharing_common[r] = common[s];
        sharing_first[r] = first[s];
        if (kept[i]) {
            match_id[rk] = meta[s].kf_id;
            match_score[rk] = score[s];
            last_slot[rk] = s;
            last_score[rk] = score[s];
        }
    }
    if (tid == 0) {
        head->n_sharing = n;
        head->min_common = minc;
        head->n_match = n_kept;
        head->min_score = min_score;
    }
}

// One workgroup, one lane per entry of lScoreAndMatch: the covisibility pass
__global__ __launch_bounds__(1024) void k_place_acc(const Meta* __restrict__ meta, const State* __restrict__ state, int32_t mode, int32_t stamp,
                                                    int32_t minc, float start, int32_t n, const int32_t* __restrict__ entry_slot,
                                                    const float* __restrict__ entry_score, const int32_t* __restrict__ nbr_off,
                                                    const int32_t* __restrict__ nbr_slot, int32_t* best, uint8_t* flag, Head* head,
                                                    int64_t* cand_id, float* acc, int64_t* best_id) {
#pragma clang fp contract(off)
    __shared__ float s_retain;
    __shared__ int n_cand;
    const int tid = threadIdx.x;
    for (int32_t i = tid; i < n; i += 1024) {
        float a = entry_score[i], bs = entry_score[i];
        int32_t b = entry_slot[i];
        for (int32_t k = nbr_off[i]; k < nbr_off[i + 1]; ++k) {
            const int32_t s = nbr_slot[k];
            if (s < 0) continue;
            const State st = state[s];
            float sc;
            if (mode == QSP_PLACE_LOOP) {
                if (!(st.loop_stamp == stamp && st.loop_words > minc)) continue;      // :159
                sc = st.loop_score;
            } else {
                if (st.reloc_stamp != stamp) continue;                                // :273, scored in this query or not
                sc = st.reloc_score;
            }
            a += sc;
            if (sc > bs) { b = s; bs = sc; }
        }
        acc[i] = a;
        best[i] = b;
        best_id[i] = meta[b].kf_id;
    }
    __syncthreads();
    if (tid == 0) {
        float bestAcc = start;
        for (int32_t i = 0; i < n; ++i)
            if (acc[i] > bestAcc) bestAcc = acc[i];
        s_retain = 0.75f * bestAcc;
        n_cand = 0;
    }
    __syncthreads();
    const float retain = s_retain;
    for (int32_t i = tid; i < n; i += 1024) {
        bool f = acc[i] > retain;
        for (int32_t j = 0; f && j < i; ++j)
            if (acc[j] > retain && best[j] == best[i]) f = false;
        flag[i] = f ? 1 : 0;
    }
    __syncthreads();
    for (int32_t i = tid; i < n; i += 1024) {
        if (!flag[i]) continue;
        int pos = 0;
        for (int32_t j = 0; j < i; ++j) pos += flag[j];
        cand_id[pos] = meta[best[i]].kf_id;
        atomicAdd(&n_cand, 1);
    }
    __syncthreads();
    if (tid == 0) head->n_cand = n_cand;
}

}  // namespace place
}  // namespace qsp

struct qsp_place_db {
    int device = 0;
    int32_t* d_word = nullptr;
    double* d_value = nullptr;
    int64_t cap_w = 0, used_w = 0;
    qsp::place::Meta* d_meta = nullptr;
    qsp::place::State* d_state = nullptr;
    int32_t* d_last_slot[2] = {nullptr, nullptr};
    float* d_last_score[2] = {nullptr, nullptr};
    int32_t cap_s = 0;
    std::vector<qsp::place::Meta> meta;                  // the host's mirror: one entry per slot, holes included
    std::unordered_map<int64_t, int32_t> slot_of;        // the key frames that are known
    int32_t n_listed = 0, n_dead = 0, next_stamp = 1;
    uint32_t next_seq = 0;
    struct Last {
        bool valid = false;
        std::vector<int64_t> ids;
        int32_t stamp = 0, min_common = 0;
        float min_score = 0.f;
    } last[2];
};

namespace qsp {
namespace place {

inline int64_t device_bytes(const qsp_place_db* db) {
    return db->cap_w * (int64_t)(sizeof(int32_t) + sizeof(double)) +
           (int64_t)db->cap_s * (int64_t)(sizeof(Meta) + sizeof(State) + 2 * sizeof(int32_t) + 2 * sizeof(float));
}

template <typename T>
int regrow(T*& d, size_t keep, size_t cap) {             // a larger array with the first `keep` entries carried over
    T* q = nullptr;
    QSP_HIP(hipMalloc((void**)&q, cap * sizeof(T)));
    if (keep) {
        const hipError_t e = hipMemcpy(q, d, keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { (void)hipFree(q); QSP_HIP(e); }
    }
    if (d) (void)hipFree(d);
    d = q;
    return QSP_OK;
}

inline int reserve(qsp_place_db* db, int64_t words, int64_t slots) {
    if (words > 0x7fffffff || slots > 0x7fffffff) return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_place_db: more than 2^31 - 1 words or slots");
    if (words > db->cap_w) {
        int64_t cap = db->cap_w * 2 > words ? db->cap_w * 2 : words;
        if (cap > 0x7fffffff) cap = 0x7fffffff;
        QSP_TRY(regrow(db->d_word, (size_t)db->used_w, (size_t)cap));
        QSP_TRY(regrow(db->d_value, (size_t)db->used_w, (size_t)cap));
        db->cap_w = cap;
    }
    if (slots > db->cap_s) {
        int64_t cap = (int64_t)db->cap_s * 2 > slots ? (int64_t)db->cap_s * 2 : slots;
        if (cap > 0x7fffffff) cap = 0x7fffffff;
        const size_t keep = db->meta.size();
        QSP_TRY(regrow(db->d_meta, keep, (size_t)cap));
        QSP_TRY(regrow(db->d_state, keep, (size_t)cap));
        for (int m = 0; m < 2; ++m) {                    // the last queries die with every put: nothing to carry over
            QSP_TRY(regrow(db->d_last_slot[m], 0, (size_t)cap));
            QSP_TRY(regrow(db->d_last_score[m], 0, (size_t)cap));
        }
        db->cap_s = (int32_t)cap;
    }
    return QSP_OK;
}

inline void forget_queries(qsp_place_db* db) { db->last[0].valid = db->last[1].valid = false; }

inline const char* bow_problem(int32_t n, const int32_t* word, const double* value) {
    if (n < 0) return "negative word count";
    if (n && (!word || !value)) return "null words or values";
    for (int32_t i = 0; i < n; ++i) {
        if (word[i] < 0) return "a negative word id";
        if (i && word[i] <= word[i - 1]) return "word ids not strictly ascending";
        if (!std::isfinite(value[i])) return "a value that is not finite";
    }
    return nullptr;
}

inline int fail(const char* who, const char* why) { return qsp_fail(QSP_ERR_INVALID, (std::string(who) + ": " + why).c_str()); }

}  // namespace place
}  // namespace qsp

extern "C" int qsp_place_db_create(int device, int64_t words_hint, int32_t slots_hint, qsp_place_db** out) {
    using namespace qsp;
    if (!out) return qsp_fail(QSP_ERR_INVALID, "qsp_place_db_create: null output");
    if (words_hint < 0 || slots_hint < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_place_db_create: negative capacity hint");
    QSP_TRY(use_device(device, "qsp_place_db_create"));
    qsp_place_db* db = nullptr;
    try { db = new qsp_place_db(); } catch (const std::exception&) { return qsp_fail(QSP_ERR_INVALID, "qsp_place_db_create: out of host memory"); }
    db->device = device;
    const int rc = place::reserve(db, words_hint ? words_hint : (int64_t)1 << 20, slots_hint ? slots_hint : 1024);
    if (rc) { qsp_place_db_destroy(db); return rc; }
    *out = db;
    return QSP_OK;
}

extern "C" void qsp_place_db_destroy(qsp_place_db* db) {
    if (!db) return;
    if (hipSetDevice(db->device) == hipSuccess) {
        (void)hipFree(db->d_word); (void)hipFree(db->d_value); (void)hipFree(db->d_meta); (void)hipFree(db->d_state);
        for (int m = 0; m < 2; ++m) { (void)hipFree(db->d_last_slot[m]); (void)hipFree(db->d_last_score[m]); }
    }
    delete db;
}

extern "C" int qsp_place_db_put(qsp_place_db* db, int64_t kf_id, int32_t n, const int32_t* word, const double* value, int32_t listed) {
    using namespace qsp;
    const char* who = "qsp_place_db_put";
    if (!db) return place::fail(who, "null handle");
    if (const char* why = place::bow_problem(n, word, value)) return place::fail(who, why);
    if (db->slot_of.count(kf_id)) return place::fail(who, "this key frame id is already known");
    if (listed && db->next_seq == 0xffffffffu) return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_place_db_put: list sequence numbers exhausted");
    QSP_HIP(hipSetDevice(db->device));
    const int32_t s = (int32_t)db->meta.size();
    QSP_TRY(place::reserve(db, db->used_w + n, (int64_t)s + 1));
    place::Meta m;
    m.off = db->used_w; m.kf_id = kf_id; m.n = n; m.listed = listed ? 1 : 0; m.seq = listed ? db->next_seq : 0; m.alive = 1;
    try {
        db->meta.push_back(m);
        db->slot_of[kf_id] = s;
    } catch (const std::exception&) {
        if ((int32_t)db->meta.size() > s) db->meta.pop_back();
        return place::fail(who, "out of host memory");
    }
    hipError_t e = hipSuccess;
    if (n) e = hipMemcpy(db->d_word + m.off, word, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (n && e == hipSuccess) e = hipMemcpy(db->d_value + m.off, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db->d_meta + s, &m, sizeof(m), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(db->d_state + s, 0, sizeof(place::State));       // stamps 0 = never, scores 0.0f
    if (e != hipSuccess) {
        db->meta.pop_back();
        db->slot_of.erase(kf_id);
        QSP_HIP(e);
    }
    db->used_w += n;
    if (listed) { ++db->next_seq; ++db->n_listed; }
    place::forget_queries(db);
    return QSP_OK;
}

extern "C" int qsp_place_db_list(qsp_place_db* db, int64_t kf_id) {
    using namespace qsp;
    const char* who = "qsp_place_db_list";
    if (!db) return place::fail(who, "null handle");
    const auto it = db->slot_of.find(kf_id);
    if (it == db->slot_of.end()) return place::fail(who, "unknown key frame id");
    place::Meta m = db->meta[it->second];
    if (m.listed) return place::fail(who, "the key frame is already listed");
    if (db->next_seq == 0xffffffffu) return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_place_db_list: list sequence numbers exhausted");
    m.listed = 1; m.seq = db->next_seq;
    QSP_HIP(hipSetDevice(db->device));
    QSP_HIP(hipMemcpy(db->d_meta + it->second, &m, sizeof(m), hipMemcpyHostToDevice));
    db->meta[it->second] = m;
    ++db->next_seq; ++db->n_listed;
    place::forget_queries(db);
    return QSP_OK;
}

extern "C" int qsp_place_db_erase(qsp_place_db* db, int64_t kf_id) {
    using namespace qsp;
    if (!db) return place::fail("qsp_place_db_erase", "null handle");
    const auto it = db->slot_of.find(kf_id);
    if (it == db->slot_of.end()) return QSP_OK;
    place::Meta m = db->meta[it->second];
    const int32_t was_listed = m.listed;
    m.alive = 0; m.listed = 0;
    QSP_HIP(hipSetDevice(db->device));
    QSP_HIP(hipMemcpy(db->d_meta + it->second, &m, sizeof(m), hipMemcpyHostToDevice));
    db->meta[it->second] = m;
    db->slot_of.erase(it);
    db->n_listed -= was_listed;
    ++db->n_dead;
    place::forget_queries(db);
    return QSP_OK;
}

extern "C" int qsp_place_db_clear(qsp_place_db* db) {
    using namespace qsp;
    if (!db) return place::fail("qsp_place_db_clear", "null handle");
    db->meta.clear();
    db->slot_of.clear();
    db->used_w = 0;
    db->n_listed = db->n_dead = 0;
    db->next_seq = 0;
    db->next_stamp = 1;
    place::forget_queries(db);
    return QSP_OK;
}

extern "C" int qsp_place_db_size(qsp_place_db* db, int32_t* known, int32_t* listed, int32_t* dead_slots, int64_t* device_bytes) {
    using namespace qsp;
    if (!db) return place::fail("qsp_place_db_size", "null handle");
    if (known) *known = (int32_t)db->slot_of.size();
    if (listed) *listed = db->n_listed;
    if (dead_slots) *dead_slots = db->n_dead;
    if (device_bytes) *device_bytes = place::device_bytes(db);
    return QSP_OK;
}

extern "C" int qsp_place_db_query(qsp_place_db* db, const qsp_place_query_in* in, qsp_place_query_out* out) {
    using namespace qsp;
    const char* who = "qsp_place_db_query";
    if (!db || !in || !out) return place::fail(who, "null handle, input or output");
    if (in->mode != QSP_PLACE_LOOP && in->mode != QSP_PLACE_RELOC) return place::fail(who, "unknown mode");
    if (const char* why = place::bow_problem(in->n, in->word, in->value)) return place::fail(who, why);
    const bool loop = in->mode == QSP_PLACE_LOOP;
    const int32_t n_excl = loop ? in->n_excluded : 0, n_ref = loop ? in->n_ref : 0;
    if (n_excl < 0 || n_ref < 0) return place::fail(who, "negative count of excluded ids or refs");
    if ((n_excl && !in->excluded) || (n_ref && !in->ref_id)) return place::fail(who, "null excluded ids or refs");
    if (loop && n_ref == 0 && std::isnan(in->min_score)) return place::fail(who, "min_score is NaN");
    if (!out->match_id || !out->match_score) return place::fail(who, "null match_id or match_score");
    if (db->next_stamp == 0x7fffffff) return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_place_db_query: query stamps exhausted; clear the database");
    const int32_t n_slots = (int32_t)db->meta.size(), nq = in->n;
    std::vector<int32_t> excl, ref;
    try {
        for (int32_t i = 0; i < n_excl; ++i) {
            const auto it = db->slot_of.find(in->excluded[i]);
            if (it != db->slot_of.end()) excl.push_back(it->second);                   // unknown ids are ignored
        }
        for (int32_t i = 0; i < n_ref; ++i) {
            const auto it = db->slot_of.find(in->ref_id[i]);
            if (it == db->slot_of.end()) return place::fail(who, "an unknown ref_id");
            ref.push_back(it->second);
        }
    } catch (const std::exception&) {
        return place::fail(who, "out of host memory");
    }
    QSP_HIP(hipSetDevice(db->device));
    // up      [qword | qvalue | excl | ref]
    // scratch [flag | common | first | score | ref_score | list | key | kept]
    // down    [head | match_id | match_score | sharing_id | sharing_common | sharing_first]
    const size_t ns = (size_t)n_slots, nl = (size_t)db->n_listed;
    StagingLayout L;
    const size_t a_qw = L.take<int32_t>((size_t)nq), a_qv = L.take<double>((size_t)nq), a_ex = L.take<int32_t>(excl.size()),
                 a_rf = L.take<int32_t>(ref.size());
    L.begin_scratch();
    const size_t a_flag = L.take<uint8_t>(ns), a_com = L.take<int32_t>(ns), a_first = L.take<int32_t>(ns), a_score = L.take<float>(ns),
                 a_rs = L.take<float>(ref.size()), a_list = L.take<int32_t>(ns), a_key = L.take<unsigned long long>(ns),
                 a_kept = L.take<uint8_t>(ns);
    L.begin_down();
    const size_t a_head = L.take<place::Head>(1), a_mid = L.take<int64_t>(nl), a_ms = L.take<float>(nl), a_sid = L.take<int64_t>(nl),
                 a_sc = L.take<int32_t>(nl), a_sf = L.take<int32_t>(nl);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return place::fail(who, "out of host memory for the staging buffers");
    put(up, a_qw, in->word, 4 * (size_t)nq);
    put(up, a_qv, in->value, 8 * (size_t)nq);
    put(up, a_ex, excl.data(), 4 * excl.size());
    put(up, a_rf, ref.data(), 4 * ref.size());
    DeviceBlock blk;
    QSP_TRY(blk.take(db->device, L.total()));
    if (L.up_bytes()) QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    const int32_t* d_qw = ptr<int32_t>(d, a_qw);
    const double* d_qv = ptr<double>(d, a_qv);
    uint8_t* d_flag = ptr<uint8_t>(d, a_flag);
    int32_t *d_com = ptr<int32_t>(d, a_com), *d_first = ptr<int32_t>(d, a_first);
    float *d_score = ptr<float>(d, a_score), *d_rs = ptr<float>(d, a_rs);
    place::Head* d_head = ptr<place::Head>(d, a_head);
    const int32_t stamp = db->next_stamp, mode = in->mode;
    // every launch on the null stream, no host round trip in between
    QSP_HIP(hipMemsetAsync(d_head, 0, sizeof(place::Head), 0));
    if (!excl.empty()) {
        QSP_HIP(hipMemsetAsync(d_flag, 0, ns, 0));
        hipLaunchKernelGGL(place::k_place_mark, dim3((unsigned)((excl.size() + 255) / 256)), dim3(256), 0, 0, ptr<int32_t>(d, a_ex),
                           (int32_t)excl.size(), d_flag);
        QSP_HIP(hipGetLastError());
    }
    if (n_slots) {
        const dim3 grid((unsigned)((n_slots + 3) / 4));
        hipLaunchKernelGGL(place::k_place_common, grid, dim3(256), 0, 0, db->d_meta, db->d_state, db->d_word, n_slots, d_qw, nq, mode, stamp,
                           excl.empty() ? (const uint8_t*)nullptr : d_flag, d_com, d_first, d_head);
        QSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(place::k_place_score, grid, dim3(256), 0, 0, db->d_meta, db->d_state, db->d_word, db->d_value, d_qw, d_qv, nq,
                           (const int32_t*)nullptr, n_slots, d_com, d_head, mode, d_score);
        QSP_HIP(hipGetLastError());
    }
    if (!ref.empty()) {
        hipLaunchKernelGGL(place::k_place_score, dim3((unsigned)((ref.size() + 3) / 4)), dim3(256), 0, 0, db->d_meta, db->d_state, db->d_word,
                           db->d_value, d_qw, d_qv, nq, ptr<int32_t>(d, a_rf), (int32_t)ref.size(), (const int32_t*)nullptr, d_head, mode, d_rs);
        QSP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(place::k_place_order, dim3(1), dim3(1024), 0, 0, db->d_meta, n_slots, d_com, d_first, d_score, d_head, mode,
                       loop ? in->min_score : 0.f, d_rs, (int32_t)ref.size(), ptr<int32_t>(d, a_list), ptr<unsigned long long>(d, a_key),
                       ptr<uint8_t>(d, a_kept), ptr<int64_t>(d, a_sid), ptr<int32_t>(d, a_sc), ptr<int32_t>(d, a_sf), ptr<int64_t>(d, a_mid),
                       ptr<float>(d, a_ms), db->d_last_slot[mode], db->d_last_score[mode]);
    QSP_HIP(hipGetLastError());
    // the stamps are on the device from here on: the query counts as made whatever happens next
    ++db->next_stamp;
    db->last[mode].valid = false;
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    const place::Head hd = *ptr<place::Head>(h, L.in_down(a_head));
    qsp_place_db::Last& last = db->last[mode];
    try { last.ids.assign(ptr<int64_t>(h, L.in_down(a_mid)), ptr<int64_t>(h, L.in_down(a_mid)) + hd.n_match); } catch (const std::exception&) {
        return place::fail(who, "out of host memory");
    }
    last.stamp = stamp; last.min_common = hd.min_common; last.min_score = hd.min_score; last.valid = true;
    // outputs are written only once everything has succeeded
    out->n_sharing = hd.n_sharing; out->max_common = hd.max_common; out->min_common = hd.min_common; out->n_match = hd.n_match;
    out->min_score_used = hd.min_score;
    const size_t nm = (size_t)hd.n_match, nsh = (size_t)hd.n_sharing;
    if (nm) {
        memcpy(out->match_id, h + L.in_down(a_mid), 8 * nm);
        memcpy(out->match_score, h + L.in_down(a_ms), 4 * nm);
    }
    if (nsh) {
        if (out->sharing_id) memcpy(out->sharing_id, h + L.in_down(a_sid), 8 * nsh);
        if (out->sharing_common) memcpy(out->sharing_common, h + L.in_down(a_sc), 4 * nsh);
        if (out->sharing_first) memcpy(out->sharing_first, h + L.in_down(a_sf), 4 * nsh);
    }
    return QSP_OK;
}

extern "C" int qsp_place_db_accumulate(qsp_place_db* db, int32_t mode, int32_t n, const int64_t* id, const int32_t* nbr_off,
                                       const int64_t* nbr_id, qsp_place_acc_out* out) {
    using namespace qsp;
    const char* who = "qsp_place_db_accumulate";
    if (!db || !out) return place::fail(who, "null handle or output");
    if (mode != QSP_PLACE_LOOP && mode != QSP_PLACE_RELOC) return place::fail(who, "unknown mode");
    if (n < 0) return place::fail(who, "negative entry count");
    const qsp_place_db::Last& last = db->last[mode];
    if (!last.valid) return place::fail(who, "no live query of this mode (none made, or the database changed since)");
    if ((size_t)n != last.ids.size() || (n && !id) || (n && memcmp(id, last.ids.data(), 8 * (size_t)n) != 0))
        return place::fail(who, "the ids are not the last query's lScoreAndMatch of this mode");
    if (!nbr_off) return place::fail(who, "null nbr_off");
    if (nbr_off[0] != 0) return place::fail(who, "nbr_off does not start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (nbr_off[i + 1] < nbr_off[i]) return place::fail(who, "nbr_off decreases");
    const size_t nn = (size_t)nbr_off[n], ne = (size_t)n;
    if (nn && !nbr_id) return place::fail(who, "null nbr_id");
    if (n && !out->cand_id) return place::fail(who, "null cand_id");
    if (n == 0) { out->n_cand = 0; return QSP_OK; }                                       // :141 / :255
    QSP_HIP(hipSetDevice(db->device));
    // up [nbr_off | nbr_slot]   scratch [best | flag]   down [head | cand_id | acc | best_id]
    StagingLayout L;
    const size_t a_off = L.take<int32_t>(ne + 1), a_nb = L.take<int32_t>(nn);
    L.begin_scratch();
    const size_t a_best = L.take<int32_t>(ne), a_flag = L.take<uint8_t>(ne);
    L.begin_down();
    const size_t a_head = L.take<place::Head>(1), a_cid = L.take<int64_t>(ne), a_acc = L.take<float>(ne), a_bid = L.take<int64_t>(ne);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return place::fail(who, "out of host memory for the staging buffers");
    put(up, a_off, nbr_off, 4 * (ne + 1));
    int32_t* slot = ptr<int32_t>(up.data(), a_nb);
    for (size_t k = 0; k < nn; ++k) {
        const auto it = db->slot_of.find(nbr_id[k]);
        slot[k] = it == db->slot_of.end() ? -1 : it->second;                             // unknown or erased: not of this query
    }
    DeviceBlock blk;
    QSP_TRY(blk.take(db->device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    place::Head* d_head = ptr<place::Head>(d, a_head);
    QSP_HIP(hipMemsetAsync(d_head, 0, sizeof(place::Head), 0));
    hipLaunchKernelGGL(place::k_place_acc, dim3(1), dim3(1024), 0, 0, db->d_meta, db->d_state, mode, last.stamp, last.min_common,
                       mode == QSP_PLACE_LOOP ? last.min_score : 0.f, n, db->d_last_slot[mode], db->d_last_score[mode], ptr<int32_t>(d, a_off),
                       ptr<int32_t>(d, a_nb), ptr<int32_t>(d, a_best), ptr<uint8_t>(d, a_flag), d_head, ptr<int64_t>(d, a_cid),
                       ptr<float>(d, a_acc), ptr<int64_t>(d, a_bid));
    QSP_HIP(hipGetLastError());
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    const place::Head hd = *ptr<place::Head>(h, L.in_down(a_head));
    out->n_cand = hd.n_cand;
    if (hd.n_cand) memcpy(out->cand_id, h + L.in_down(a_cid), 8 * (size_t)hd.n_cand);
    if (out->acc_score) memcpy(out->acc_score, h + L.in_down(a_acc), 4 * ne);
    if (out->best_id) memcpy(out->best_id, h + L.in_down(a_bid), 8 * ne);
    return QSP_OK;
}
