// search_triangulation.hpp -- ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:657-823, CheckDistEpipolarLine
// :140-157) for ALL covisible neighbours of LocalMapping::CreateNewMapPoints in one call.  Compiled in c_abi.cpp after
// search_bow.hpp, whose frame layout (bow::FrameB, bow::In), host-side CSR check and rotation tail (k_bow_rot) it uses as they are;
// the Hamming distance and the search over node ids are orb_match.hpp's, the wave reduction is wave.hpp's.
//
// The reference walks the two DBoW2::FeatureVectors in step and, inside a common node, compares every source without a map point
// with every target without one.  It declares vbMatched2 and reads it (:725) but never sets it, so there is NO loop-carried state:
// a source's result does not depend on any other source, and two sources may end up with the same target (kept).
//
// The serial loop and its closed form.  The loop keeps (bestDist, bestIdx2), starts at (th, -1), skips a target when
// `dist > th || dist > bestDist` and replaces the best when the target also passes the two geometric tests.  A target that fails a
// geometric test never changes the state, and bestDist only ever takes distances of passing targets, which never grow.  So the
// loop ends on the passing target (dist <= th) of SMALLEST distance, and among equal distances on the LAST one in list order (`>`
// lets an equal distance through, and it replaces).  That is the minimum of the key (dist << 32) | (0xffffffff - position) over
// the passing targets.  A lane that strides over the list and prunes with its OWN running best drops only targets that cannot be
// that minimum, so a lane-strided walk plus one wave reduction of the key equals the serial loop for any list length: no taken
// marks, no scratch array, no size threshold.
//
// ONE WAVE owns one (candidate, position in the source frame's feature list).  It finds its node by binary search in node_off, the
// target's node by binary search in the ascending ids (as k_bow_match does); every early exit is wave-uniform.  Float32 throughout,
// one IEEE operation at a time (contraction OFF), the last compare in double as the reference's `dsqr < 3.84 * sigma2` is.
#pragma once
#include <cmath>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "orb_match.hpp"
#include "search_bow.hpp"
#include "staging.hpp"
#include "wave.hpp"

namespace qsp {
namespace tri {

struct Geo {                           // beside bow::In: indexed by the same slots
    const float* xy;                   // [n_slot][2]
    const float *sigma2, *scale;       // [n_slot] (read of targets only)
    const uint8_t* stereo;             // [n_slot]
    const float *F12, *exy;            // [n_cand][9], [n_cand][2]
    int32_t n_list, only_stereo;       // n_list: the length of the source frame's feature list
};

// 4 waves per workgroup, one wave per (candidate, position in the source frame's feature list)
__global__ __launch_bounds__(256) void k_tri_match(bow::In in, Geo g, int64_t n_work, int32_t* match_raw, int32_t* dist) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_work) return;
    const int c = (int)((unsigned)w / (unsigned)g.n_list);                  // n_work < 2^31
    const int32_t p = (int32_t)((unsigned)w - (unsigned)c * (unsigned)g.n_list);
    const bow::FrameB S = in.frame[0], T = in.frame[1 + c];
    const int32_t* soff = in.node_off + S.noff_at;       // soff[0] = 0 <= p < n_list = soff[n_nodes]
    int32_t lo = 0, hi = S.n_nodes;                      // the node that holds p: the last k with soff[k] <= p (empty nodes are stepped over)
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (soff[mid] <= p) lo = mid; else hi = mid;
    }
    // the reference's lower_bound walk over the two maps visits exactly the ids both hold
    const int32_t id = in.node_id[S.node_at + lo];
    const int32_t* tid = in.node_id + T.node_at;
    const int32_t a = orb::lower_bound_id(tid, T.n_nodes, id);
    if (a >= T.n_nodes || tid[a] != id) return;
    const int32_t t0 = in.node_off[T.noff_at + a], nt = in.node_off[T.noff_at + a + 1] - t0;
    if (nt == 0) return;
    const int32_t i = in.feat[S.feat_at + p];
    const int64_t gs = (int64_t)S.off + i;
    if (!in.elig[gs]) return;                            // :702
    const bool stereo1 = g.stereo[gs] != 0;
    if (g.only_stereo && !stereo1) return;               // :707
    const int32_t* tf = in.feat + T.feat_at + t0;
    const uint4* sd = (const uint4*)(in.desc + 32 * gs);
    const uint4 m0 = sd[0], m1 = sd[1];
    // the epipolar line of the source in the target image, l = x1' F12 (:143-145): the same for every target
    const float* F = g.F12 + 9 * (int64_t)c;
    const float x1 = g.xy[2 * gs], y1 = g.xy[2 * gs + 1];
    const float la = x1 * F[0] + y1 * F[3] + F[6];
    const float lb = x1 * F[1] + y1 * F[4] + F[7];
    const float lc = x1 * F[2] + y1 * F[5] + F[8];
    const float den = la * la + lb * lb;
    const float ex = g.exy[2 * (int64_t)c], ey = g.exy[2 * (int64_t)c + 1];
    int best = in.th;                                    // :715
    unsigned long long key = orb::NO_KEY;
    for (int32_t j = lane; j < nt; j += 64) {
        const int32_t t = tf[j];
        const int64_t gt = (int64_t)T.off + t;
        if (!in.elig[gt]) continue;                      // :725
        const bool stereo2 = g.stereo[gt] != 0;
        if (g.only_stereo && !stereo2) continue;         // :730
        const int hd = orb::hamming256(in.desc + 32 * gt, m0, m1);
        if (hd > in.th || hd > best) continue;           // :738, `best` being this lane's own
        const float x2 = g.xy[2 * gt], y2 = g.xy[2 * gt + 1];
        if (!stereo1 && !stereo2) {                      // :743-749
            const float distex = ex - x2, distey = ey - y2;
            if (distex * distex + distey * distey < 100.0f * g.scale[gt]) continue;
        }
        const float num = la * x2 + lb * y2 + lc;        // :147-156
        if (den == 0.0f) continue;
        // num * num / den: the double quotient of two float32 values, rounded once more, IS the correctly rounded float32 quotient
        // (53 >= 2 * 24 + 2), whatever the float32 division of the build expands to
        const float dsqr = (float)((double)(num * num) / (double)den);
        if (!((double)dsqr < 3.84 * (double)g.sigma2[gt])) continue;
        best = hd;
        key = ((unsigned long long)(unsigned)hd << 32) | (0xffffffffu - (unsigned)j);
    }
    key = wave_min(key);                                 // the smallest distance, and of equal distances the LAST list position
    if (key == orb::NO_KEY) return;
    if (lane == 0) {
        const int64_t at = (int64_t)c * in.n0 + i;
        match_raw[at] = tf[0xffffffffu - (unsigned)key];
        dist[at] = (int)(key >> 32);
    }
}

// The host side of the call in the steps every one-shot batch call takes -- check, lay out, pack, launch, copy out -- so that
// qsp_create_new_map_points_batch (triangulate.hpp) can run the same two launches inside its own staging block and hand the match
// grid to the triangulation kernels while it is still on the device.
struct SearchPlan {
    const qsp_search_tri_in* in = nullptr;
    int32_t nc = 0;
    int64_t n_slot = 0, n_node = 0, n_feat = 0, n0 = 0, n_list = 0, n_grid = 0, n_work = 0;
    size_t a_frame = 0, a_nid = 0, a_noff = 0, a_feat = 0, a_desc = 0, a_angle = 0, a_elig = 0, a_stereo = 0, a_xy = 0, a_sigma = 0, a_scale = 0,
           a_F = 0, a_e = 0;
    size_t a_match = 0, a_raw = 0, a_dist = 0, a_count = 0, a_hist = 0, a_ind = 0;

    // everything the call refuses, in its order; in->n_cand > 0 has been established by the caller
    int check(const qsp_search_tri_in* in_, const qsp_search_tri_out* out, const char* who) {
        auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
        in = in_;
        if (!out || !out->match || !out->n_matches) return bad(QSP_ERR_INVALID, "null output");
        if (!in->kf1 || !in->kf2) return bad(QSP_ERR_INVALID, "null frames");
        if (!in->F12 || !in->exy) return bad(QSP_ERR_INVALID, "null F12 or epipoles");
        if (in->th < 0 || in->th > 256) return bad(QSP_ERR_INVALID, "th outside [0, 256]");
        nc = in->n_cand;
        try {
            std::vector<uint8_t> seen;
            for (int32_t f = 0; f <= nc; ++f) {
                const qsp_tri_frame& F = f ? in->kf2[f - 1] : *in->kf1;
                const char* side = f ? "neighbour key frame: " : "source key frame: ";
                seen.assign((size_t)(F.bow.n > 0 ? F.bow.n : 0), 0);
                const char* why = bow_frame_problem(F.bow, seen);
                if (why) return bad(QSP_ERR_INVALID, std::string(side) + why);
                if (F.bow.n && (!F.xy || !F.stereo)) return bad(QSP_ERR_INVALID, std::string(side) + "null xy or stereo");
                if (f && F.bow.n && (!F.sigma2 || !F.scale)) return bad(QSP_ERR_INVALID, std::string(side) + "null sigma2 or scale");
                n_slot += F.bow.n;
                n_node += F.bow.n_nodes;
                n_feat += F.bow.node_off[F.bow.n_nodes];
            }
        } catch (const std::exception&) {
            return bad(QSP_ERR_INVALID, "out of host memory while checking the feature vectors");
        }
        const qsp_bow_frame& B1 = in->kf1->bow;
        n0 = B1.n; n_list = B1.node_off[B1.n_nodes]; n_grid = (int64_t)nc * n0; n_work = (int64_t)nc * n_list;
        if (n_slot > 0x7fffffff || n_grid > 0x7fffffff || n_node + nc + 1 > 0x7fffffff || n_work > 0x7fffffff)
            return bad(QSP_ERR_UNSUPPORTED, "more than 2^31 - 1 key-point slots, nodes or work items in one call");
        return QSP_OK;
    }
    // up      [frame | node_id | node_off | feat | desc | angle | elig | stereo | xy | sigma2 | scale | F12 | exy]
    void take_up(StagingLayout& L) {
        const size_t ns = (size_t)n_slot, nf = (size_t)nc + 1;
        a_frame = L.take<bow::FrameB>(nf); a_nid = L.take<int32_t>((size_t)n_node); a_noff = L.take<int32_t>((size_t)n_node + nf);
        a_feat = L.take<int32_t>((size_t)n_feat); a_desc = L.take<uint8_t>(ns * 32); a_angle = L.take<float>(ns);
        a_elig = L.take<uint8_t>(ns); a_stereo = L.take<uint8_t>(ns); a_xy = L.take<float>(2 * ns); a_sigma = L.take<float>(ns);
        a_scale = L.take<float>(ns); a_F = L.take<float>(9 * (size_t)nc); a_e = L.take<float>(2 * (size_t)nc);
    }
    // down    [match | match_raw | dist | n_matches | hist | ind]
    void take_down(StagingLayout& L) {
        const size_t no = (size_t)n_grid;
        a_match = L.take<int32_t>(no); a_raw = L.take<int32_t>(no); a_dist = L.take<int32_t>(no); a_count = L.take<int32_t>((size_t)nc);
        a_hist = L.take<int32_t>((size_t)nc * orb::HISTO_LENGTH); a_ind = L.take<int32_t>((size_t)nc * 3);
    }
    void pack(std::vector<char>& up) const {
        bow::FrameB* fp = ptr<bow::FrameB>(up.data(), a_frame);
        size_t slot = 0, node = 0, feat = 0;
        for (int32_t f = 0; f <= nc; ++f) {
            const qsp_tri_frame& G = f ? in->kf2[f - 1] : *in->kf1;
            const qsp_bow_frame& F = G.bow;
            bow::FrameB& P = fp[f];
            const size_t n = (size_t)F.n, nn = (size_t)F.n_nodes, nl = (size_t)F.node_off[F.n_nodes];
            P.off = (int32_t)slot; P.n = F.n;
            P.node_at = (int32_t)node; P.n_nodes = F.n_nodes;
            P.noff_at = (int32_t)(node + (size_t)f); P.feat_at = (int32_t)feat;
            put(up, a_nid + 4 * node, F.node_id, 4 * nn);
            put(up, a_noff + 4 * (node + (size_t)f), F.node_off, 4 * (nn + 1));
            put(up, a_feat + 4 * feat, F.feat, 4 * nl);
            put(up, a_desc + 32 * slot, F.desc, 32 * n);
            put(up, a_angle + 4 * slot, F.angle, 4 * n);
            put(up, a_xy + 8 * slot, G.xy, 8 * n);
            if (f) {
                put(up, a_sigma + 4 * slot, G.sigma2, 4 * n);
                put(up, a_scale + 4 * slot, G.scale, 4 * n);
            }
            for (size_t i = 0; i < n; ++i) {
                up[a_elig + slot + i] = (!F.eligible || F.eligible[i]) ? 1 : 0;
                up[a_stereo + slot + i] = G.stereo[i] ? 1 : 0;
            }
            slot += n; node += nn; feat += nl;
        }
        put(up, a_F, in->F12, 36 * (size_t)nc);
        put(up, a_e, in->exy, 8 * (size_t)nc);
    }
    int32_t* match_on_device(char* d) const { return ptr<int32_t>(d, a_match); }
    // one fill and two launches on one stream, no host round trip in between
    int launch(char* d) const {
        bow::In k;                                       // what k_tri_match and k_bow_rot read of it; the shared frame is the source
        k.frame = ptr<bow::FrameB>(d, a_frame); k.work_off = nullptr;
        k.node_id = ptr<int32_t>(d, a_nid); k.node_off = ptr<int32_t>(d, a_noff); k.feat = ptr<int32_t>(d, a_feat);
        k.desc = ptr<uint8_t>(d, a_desc); k.angle = ptr<float>(d, a_angle); k.elig = ptr<uint8_t>(d, a_elig);
        k.n_cand = nc; k.n0 = (int32_t)n0; k.shared_is_source = 1; k.th = in->th; k.th_inclusive = 1;
        k.check_ori = in->check_orientation ? 1 : 0; k.nn_ratio = 0.0f;
        Geo g;
        g.xy = ptr<float>(d, a_xy); g.sigma2 = ptr<float>(d, a_sigma); g.scale = ptr<float>(d, a_scale); g.stereo = ptr<uint8_t>(d, a_stereo);
        g.F12 = ptr<float>(d, a_F); g.exy = ptr<float>(d, a_e);
        g.n_list = (int32_t)n_list; g.only_stereo = in->only_stereo ? 1 : 0;
        int32_t *d_match = ptr<int32_t>(d, a_match), *d_raw = ptr<int32_t>(d, a_raw), *d_dist = ptr<int32_t>(d, a_dist);
        int32_t *d_count = ptr<int32_t>(d, a_count), *d_hist = ptr<int32_t>(d, a_hist), *d_ind = ptr<int32_t>(d, a_ind);
        if (n_grid) QSP_HIP(hipMemsetAsync(d_raw, 0xff, (a_count - a_raw), 0));     // match_raw and dist: -1 everywhere
        if (n_work) {
            hipLaunchKernelGGL(k_tri_match, dim3((unsigned)((n_work + 3) / 4)), dim3(256), 0, 0, k, g, n_work, d_raw, d_dist);
            QSP_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(bow::k_bow_rot, dim3((unsigned)nc), dim3(256), 0, 0, k, d_raw, d_match, d_count, d_hist, d_ind);
        QSP_HIP(hipGetLastError());
        return QSP_OK;
    }
    // h: a host copy of the DOWN region
    void copy_out(const char* h, const StagingLayout& L, qsp_search_tri_out* out) const {
        const size_t no = (size_t)n_grid;
        if (no) {
            memcpy(out->match, h + L.in_down(a_match), 4 * no);
            if (out->match_raw) memcpy(out->match_raw, h + L.in_down(a_raw), 4 * no);
            if (out->dist) memcpy(out->dist, h + L.in_down(a_dist), 4 * no);
        }
        memcpy(out->n_matches, h + L.in_down(a_count), 4 * (size_t)nc);
        if (out->hist) memcpy(out->hist, h + L.in_down(a_hist), 4 * (size_t)nc * orb::HISTO_LENGTH);
        if (out->ind) memcpy(out->ind, h + L.in_down(a_ind), 4 * (size_t)nc * 3);
    }
};

}  // namespace tri
}  // namespace qsp

extern "C" int qsp_search_for_triangulation_batch(int device, const qsp_search_tri_in* in, qsp_search_tri_out* out) {
    using namespace qsp;
    const char* who = "qsp_search_for_triangulation_batch";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!in) return bad(QSP_ERR_INVALID, "null input");
    if (in->n_cand < 0) return bad(QSP_ERR_INVALID, "negative candidate count");
    if (in->n_cand == 0) return QSP_OK;
    tri::SearchPlan S;
    QSP_TRY(S.check(in, out, who));
    QSP_TRY(use_device(device, who));
    StagingLayout L;
    S.take_up(L);
    L.begin_down();
    S.take_down(L);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    S.pack(up);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    QSP_TRY(S.launch(blk.data()));
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    S.copy_out(down.data(), L, out);
    return QSP_OK;
}
