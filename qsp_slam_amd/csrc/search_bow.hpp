// search_bow.hpp -- ORBmatcher::SearchByBoW for ALL candidates in one call: the key-frame overload of LoopClosing::ComputeSim3
// (reference src/ORBmatcher.cc:522-655, shared_is_source = 1) and the frame overload of Tracking::Relocalization (:159-288,
// shared_is_source = 0).  Compiled in c_abi.cpp; the Hamming distance, the two binary searches, rot_bin and three_maxima are
// orb_match.hpp's.
//
// The reference walks the two DBoW2::FeatureVectors in step and, inside a common vocabulary node, matches every source feature
// against the node's target features, greedily: a target that an earlier source took is gone (vbMatched2[idx2] /
// vpMapPointMatches[realIdxF]).  That taken mark is the only loop-carried state, and a feature index belongs to exactly one node
// of a FeatureVector (the host refuses anything else), so nodes are independent: ONE WAVE owns one (candidate, node of the source
// frame), finds the node in the target's ascending id list by binary search, and walks the node's sources serially in list order
// while its lanes stride over the node's target list.  Everything decided on is an integer but for one float32 product.
//
// Taken marks: one byte per target slot in a per-call scratch array.  The mark of list position p is written AND read by lane
// p & 63 alone (the lane that strides over p), so it is that thread's own store followed by its own load: no other lane, wave or
// atomic is involved, any node size takes the same path, and there is no size threshold.
//
// k_bow_rot is the mbCheckOrientation tail: one workgroup per candidate, the 30-bin histogram in LDS, ComputeThreeMaxima
// (:1601-1642) as written, the cull and the count.  Contraction is OFF in both kernels.
#pragma once
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "orb_match.hpp"
#include "staging.hpp"

namespace qsp {
namespace bow {

constexpr unsigned NO_POS = 0xffffffffu;

struct FrameB {                        // one per frame: 0 is the shared one, 1 + c the frame of candidate c
    int32_t off, n;                    // its slots are [off, off + n) of desc / angle / elig
    int32_t node_at, n_nodes;          // its node ids are node_id[node_at ..), its offsets node_off[noff_at .. noff_at + n_nodes]
    int32_t noff_at, feat_at;          // its feature lists start at feat[feat_at]
};

struct In {
    const FrameB* frame;               // [n_cand + 1]
    const int64_t* work_off;           // [n_cand + 1]: candidate c owns the waves [work_off[c], work_off[c + 1]): its source's nodes
    const int32_t *node_id, *node_off, *feat;
    const uint8_t* desc;               // [n_slot][32], 16-byte aligned
    const float* angle;                // [n_slot]
    const uint8_t* elig;               // [n_slot]
    int32_t n_cand, n0, shared_is_source, th, th_inclusive, check_ori;
    float nn_ratio;
};

// where candidate c's outputs (indexed by source slot) and taken marks (indexed by target slot) start
__device__ inline void cand_places(const In& in, int c, int64_t* out_at, int64_t* taken_at) {
    const int64_t flat = (int64_t)in.frame[1 + c].off - in.n0, grid = (int64_t)c * in.n0;
    *out_at = in.shared_is_source ? grid : flat;
    *taken_at = in.shared_is_source ? flat : grid;
}

// 4 waves per workgroup, one wave per (candidate, node of the source frame)
__global__ __launch_bounds__(256) void k_bow_match(In in, int64_t n_work, int32_t* match_raw, int32_t* dist, uint8_t* taken) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_work) return;
    const int c = orb::owner_of(in.work_off, in.n_cand, w);
    const int32_t k = (int32_t)(w - in.work_off[c]);     // the node's place in the source frame's list
    const FrameB S = in.frame[in.shared_is_source ? 0 : 1 + c];
    const FrameB T = in.frame[in.shared_is_source ? 1 + c : 0];
    // the reference's lower_bound walk over the two maps visits exactly the ids both hold
    const int32_t id = in.node_id[S.node_at + k];
    const int32_t* tid = in.node_id + T.node_at;
    const int32_t a = orb::lower_bound_id(tid, T.n_nodes, id);
    if (a >= T.n_nodes || tid[a] != id) return;
    const int32_t s0 = in.node_off[S.noff_at + k], s1 = in.node_off[S.noff_at + k + 1];
    const int32_t t0 = in.node_off[T.noff_at + a], nt = in.node_off[T.noff_at + a + 1] - t0;
    if (s1 == s0 || nt == 0) return;
    const int32_t* sf = in.feat + S.feat_at;
    const int32_t* tf = in.feat + T.feat_at + t0;
    int64_t out_at, taken_at;
    cand_places(in, c, &out_at, &taken_at);
    for (int32_t s = s0; s < s1; ++s) {                  // serial, in the stored order: the greedy of :554 / :187
        const int32_t i = sf[s];
        const int64_t gs = (int64_t)S.off + i;
        if (!in.elig[gs]) continue;                      // wave-uniform
        const uint4* sd = (const uint4*)(in.desc + 32 * gs);
        const uint4 m0 = sd[0], m1 = sd[1];
        int d1 = 256, d2 = 256;
        unsigned p1 = NO_POS;
        for (int32_t j = lane; j < nt; j += 64) {
            const int32_t t = tf[j];
            const int64_t g = (int64_t)T.off + t;
            if (!in.elig[g] || taken[taken_at + t]) continue;
            const int hd = orb::hamming256(in.desc + 32 * g, m0, m1);
            if (hd < d1) { d2 = d1; d1 = hd; p1 = (unsigned)j; }       // :586-595
            else if (hd < d2) d2 = hd;
        }
        // best1 is the minimum of (distance, list position): the first in traversal under the strict `dist < bestDist1`;
        // bestDist2 is the second order statistic of the multiset of distances (with 256, 256 for "none")
        unsigned long long key = ((unsigned long long)(unsigned)d1 << 32) | p1;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long ok = __shfl_xor(key, m, 64);
            const int o2 = __shfl_xor(d2, m, 64);
            const int o1 = (int)(ok >> 32), mine = (int)(key >> 32);
            const int hi1 = o1 > mine ? o1 : mine;
            d2 = d2 < o2 ? d2 : o2;
            d2 = hi1 < d2 ? hi1 : d2;
            key = ok < key ? ok : key;
        }
        const int b1 = (int)(key >> 32);
        const unsigned p = (unsigned)key;
        const bool under = in.th_inclusive ? b1 <= in.th : b1 < in.th;
        if (p != NO_POS && under && (float)b1 < in.nn_ratio * (float)d2) {
            const int32_t t = tf[p];
            if (lane == (int)(p & 63u)) taken[taken_at + t] = 1;       // the lane that strides over p: its own later loads see it
            if (lane == 0) {
                match_raw[out_at + i] = t;
                dist[out_at + i] = b1;
            }
        }
    }
}

// one workgroup per candidate
__global__ __launch_bounds__(256) void k_bow_rot(In in, const int32_t* __restrict__ match_raw, int32_t* __restrict__ match,
                                                 int32_t* __restrict__ n_matches, int32_t* __restrict__ hist_out,
                                                 int32_t* __restrict__ ind_out) {
#pragma clang fp contract(off)
    __shared__ int hist[orb::HISTO_LENGTH];
    __shared__ int ind[3];
    __shared__ int count;
    const int c = blockIdx.x, tid = threadIdx.x;
    const FrameB S = in.frame[in.shared_is_source ? 0 : 1 + c];
    const FrameB T = in.frame[in.shared_is_source ? 1 + c : 0];
    int64_t out_at, taken_at;
    cand_places(in, c, &out_at, &taken_at);
    if (tid < orb::HISTO_LENGTH) hist[tid] = 0;
    if (tid < 3) ind[tid] = -1;
    if (tid == 0) count = 0;
    __syncthreads();
    if (in.check_ori) {
        for (int32_t i = tid; i < S.n; i += 256) {
            const int32_t m = match_raw[out_at + i];
            if (m < 0) continue;
            const int bin = orb::rot_bin(in.angle[(int64_t)S.off + i], in.angle[(int64_t)T.off + m]);
            if (bin >= 0) atomicAdd(&hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) orb::three_maxima(hist, ind);
        __syncthreads();
    }
    for (int32_t i = tid; i < S.n; i += 256) {
        const int32_t m = match_raw[out_at + i];
        bool keep = m >= 0;
        if (keep && in.check_ori) {
            const int bin = orb::rot_bin(in.angle[(int64_t)S.off + i], in.angle[(int64_t)T.off + m]);
            keep = bin >= 0 && (bin == ind[0] || bin == ind[1] || bin == ind[2]);
        }
        match[out_at + i] = keep ? m : -1;
        if (keep) atomicAdd(&count, 1);
    }
    __syncthreads();
    if (tid == 0) n_matches[c] = count;
    if (tid < orb::HISTO_LENGTH) hist_out[(int64_t)c * orb::HISTO_LENGTH + tid] = hist[tid];
    if (tid < 3) ind_out[(int64_t)c * 3 + tid] = ind[tid];
}

}  // namespace bow

// `seen` has f.n zero bytes on entry
static const char* bow_frame_problem(const qsp_bow_frame& f, std::vector<uint8_t>& seen) {
    if (f.n < 0) return "negative key-point count";
    if (f.n_nodes < 0) return "negative node count";
    if (f.n && (!f.desc || !f.angle)) return "null desc or angle";
    if (!f.node_off) return "null node_off";
    if (f.n_nodes && !f.node_id) return "null node_id";
    if (f.node_off[0] != 0) return "node_off does not start at 0";
    for (int32_t k = 0; k < f.n_nodes; ++k) {
        if (f.node_off[k + 1] < f.node_off[k]) return "node_off decreases";
        if (f.node_off[k + 1] > f.n) return "more listed features than key points";
        if (k && f.node_id[k] <= f.node_id[k - 1]) return "node ids not strictly ascending";
    }
    const int32_t nf = f.node_off[f.n_nodes];
    if (nf && !f.feat) return "null feat";
    for (int32_t j = 0; j < nf; ++j) {
        const int32_t i = f.feat[j];
        if (i < 0 || i >= f.n) return "a feature index outside its frame";
        if (seen[i]) return "a feature index listed twice in one frame";
        seen[i] = 1;
    }
    return nullptr;
}

}  // namespace qsp

extern "C" int qsp_search_by_bow_batch(int device, const qsp_search_bow_in* in, qsp_search_bow_out* out) {
    using namespace qsp;
    if (!in) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: null input");
    if (in->n_cand < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: negative candidate count");
    if (in->n_cand == 0) return QSP_OK;
    if (!out || !out->match || !out->n_matches) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: null output");
    if (!in->shared || !in->cand) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: null frames");
    if (in->th < 0 || in->th > 256) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: th outside [0, 256]");
    if (!std::isfinite(in->nn_ratio)) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: nn_ratio is not finite");
    const int32_t nc = in->n_cand;
    const bool sis = in->shared_is_source != 0;
    int64_t n_slot = 0, n_node = 0, n_feat = 0;
    try {
        std::vector<uint8_t> seen;
        for (int32_t f = 0; f <= nc; ++f) {
            const qsp_bow_frame& F = f ? in->cand[f - 1] : *in->shared;
            seen.assign((size_t)(F.n > 0 ? F.n : 0), 0);
            const char* why = bow_frame_problem(F, seen);
            if (why) return qsp_fail(QSP_ERR_INVALID, (std::string("qsp_search_by_bow_batch: ") + (f ? "candidate frame: " : "shared frame: ") + why).c_str());
            n_slot += F.n;
            n_node += F.n_nodes;
            n_feat += F.node_off[F.n_nodes];
        }
    } catch (const std::exception&) {
        return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: out of host memory while checking the feature vectors");
    }
    const int64_t n0 = in->shared->n, n_flat = n_slot - n0, n_grid = (int64_t)nc * n0;
    const int64_t n_out = sis ? n_grid : n_flat, n_taken = sis ? n_flat : n_grid;
    const int64_t n_work = sis ? (int64_t)nc * in->shared->n_nodes : n_node - in->shared->n_nodes;      // one wave per source node
    if (n_slot > 0x7fffffff || n_grid > 0x7fffffff || n_node + nc + 1 > 0x7fffffff || n_work > 0x7fffffff)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_search_by_bow_batch: more than 2^31 - 1 key-point slots or nodes in one call");
    QSP_TRY(use_device(device, "qsp_search_by_bow_batch"));
    // up      [frame | work_off | node_id | node_off | feat | desc | angle | elig]
    // scratch [taken]
    // down    [match | match_raw | dist | n_matches | hist | ind]
    const size_t ns = (size_t)n_slot, no = (size_t)n_out, nf = (size_t)nc + 1;
    StagingLayout L;
    const size_t a_frame = L.take<bow::FrameB>(nf), a_work = L.take<int64_t>(nf), a_nid = L.take<int32_t>((size_t)n_node),
                 a_noff = L.take<int32_t>((size_t)n_node + nf), a_feat = L.take<int32_t>((size_t)n_feat), a_desc = L.take<uint8_t>(ns * 32),
                 a_angle = L.take<float>(ns), a_elig = L.take<uint8_t>(ns);
    L.begin_scratch();
    const size_t a_taken = L.take<uint8_t>((size_t)n_taken);
    L.begin_down();
    const size_t a_match = L.take<int32_t>(no), a_raw = L.take<int32_t>(no), a_dist = L.take<int32_t>(no), a_count = L.take<int32_t>((size_t)nc),
                 a_hist = L.take<int32_t>((size_t)nc * orb::HISTO_LENGTH), a_ind = L.take<int32_t>((size_t)nc * 3);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes()))
        return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_bow_batch: out of host memory for the staging buffers");
    bow::FrameB* fp = ptr<bow::FrameB>(up.data(), a_frame);
    int64_t* work = ptr<int64_t>(up.data(), a_work);
    size_t slot = 0, node = 0, feat = 0;
    int64_t wk = 0;
    for (int32_t f = 0; f <= nc; ++f) {
        const qsp_bow_frame& F = f ? in->cand[f - 1] : *in->shared;
        bow::FrameB& P = fp[f];
        const size_t n = (size_t)F.n, nn = (size_t)F.n_nodes, nl = (size_t)F.node_off[F.n_nodes];
        P.off = (int32_t)slot; P.n = F.n;
        P.node_at = (int32_t)node; P.n_nodes = F.n_nodes;
        P.noff_at = (int32_t)(node + (size_t)f); P.feat_at = (int32_t)feat;
        if (nn) memcpy(up.data() + a_nid + 4 * node, F.node_id, 4 * nn);
        memcpy(up.data() + a_noff + 4 * (node + (size_t)f), F.node_off, 4 * (nn + 1));
        if (nl) memcpy(up.data() + a_feat + 4 * feat, F.feat, 4 * nl);
        if (n) {
            memcpy(up.data() + a_desc + 32 * slot, F.desc, 32 * n);
            memcpy(up.data() + a_angle + 4 * slot, F.angle, 4 * n);
            if (F.eligible) for (size_t i = 0; i < n; ++i) up[a_elig + slot + i] = F.eligible[i] ? 1 : 0;
            else memset(up.data() + a_elig + slot, 1, n);
        }
        if (f) {
            work[f - 1] = wk;
            wk += sis ? in->shared->n_nodes : F.n_nodes;
        }
        slot += n; node += nn; feat += nl;
    }
    work[nc] = wk;
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    bow::In k;
    k.frame = ptr<bow::FrameB>(d, a_frame); k.work_off = ptr<int64_t>(d, a_work);
    k.node_id = ptr<int32_t>(d, a_nid); k.node_off = ptr<int32_t>(d, a_noff); k.feat = ptr<int32_t>(d, a_feat);
    k.desc = ptr<uint8_t>(d, a_desc); k.angle = ptr<float>(d, a_angle); k.elig = ptr<uint8_t>(d, a_elig);
    k.n_cand = nc; k.n0 = (int32_t)n0; k.shared_is_source = sis ? 1 : 0; k.th = in->th; k.th_inclusive = in->th_inclusive ? 1 : 0;
    k.check_ori = in->check_orientation ? 1 : 0; k.nn_ratio = in->nn_ratio;
    uint8_t* d_taken = ptr<uint8_t>(d, a_taken);
    int32_t *d_match = ptr<int32_t>(d, a_match), *d_raw = ptr<int32_t>(d, a_raw), *d_dist = ptr<int32_t>(d, a_dist);
    int32_t *d_count = ptr<int32_t>(d, a_count), *d_hist = ptr<int32_t>(d, a_hist), *d_ind = ptr<int32_t>(d, a_ind);
    // two fills and two launches on one stream, no host round trip in between
    if (n_taken) QSP_HIP(hipMemsetAsync(d_taken, 0, (size_t)n_taken, 0));
    if (no) QSP_HIP(hipMemsetAsync(d_raw, 0xff, (a_count - a_raw), 0));         // match_raw and dist: -1 everywhere
    if (wk) {
        hipLaunchKernelGGL(bow::k_bow_match, dim3((unsigned)((wk + 3) / 4)), dim3(256), 0, 0, k, wk, d_raw, d_dist, d_taken);
        QSP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bow::k_bow_rot, dim3((unsigned)nc), dim3(256), 0, 0, k, d_raw, d_match, d_count, d_hist, d_ind);
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    if (no) {
        memcpy(out->match, h + L.in_down(a_match), 4 * no);
        if (out->match_raw) memcpy(out->match_raw, h + L.in_down(a_raw), 4 * no);
        if (out->dist) memcpy(out->dist, h + L.in_down(a_dist), 4 * no);
    }
    memcpy(out->n_matches, h + L.in_down(a_count), 4 * (size_t)nc);
    if (out->hist) memcpy(out->hist, h + L.in_down(a_hist), 4 * (size_t)nc * orb::HISTO_LENGTH);
    if (out->ind) memcpy(out->ind, h + L.in_down(a_ind), 4 * (size_t)nc * 3);
    return QSP_OK;
}
