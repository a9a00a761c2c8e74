// search_sim3.hpp -- ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1102-1326) for ALL loop candidates of a key frame in one
// call.  Compiled in c_abi.cpp; the steps it shares with the other matchers are orb_match.hpp's, the wave reduction is wave.hpp's.
//
// The reference runs, per candidate, two serial passes (key frame 1 -> 2 and 2 -> 1): project a map point through the candidate
// Sim3, walk the target frame's feature grid inside a level-dependent radius (KeyFrame::GetFeaturesInArea, KeyFrame.cc:570-609),
// keep the Hamming-nearest ORB descriptor, then keep the mutual matches.  Neither pass writes anything the other iterations read,
// so here ONE WAVE owns one (candidate, direction, source slot): all 64 lanes compute the slot's gates redundantly, then stride
// over the target frame's key points, each lane keeping the smallest orb::make_key it met, so one wave min-reduction yields the
// reference's `dist < bestDist` winner.  k_search_sim3_agree gathers the mutual matches and counts them.
//
// Every function below evaluates with contraction OFF: the float32 operations of the reference in its order.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "orb_match.hpp"
#include "staging.hpp"
#include "wave.hpp"

namespace qsp {
namespace search {

struct FrameP {                       // one per frame: 0 is key frame 1, 1 + c key frame 2 of candidate c
    orb::GridP g;
    float R[9], t[3];
};

struct CandP {
    float K[4], s12, R12[9], t12[3], th;
};

struct In {
    const FrameP* frame;              // [n_cand + 1]
    const CandP* cand;                // [n_cand]
    const int64_t* work_off;          // [n_cand + 1]: candidate c owns the waves [work_off[c], work_off[c + 1]): n1 + n2[c] of them
    const int32_t* off2;              // [n_cand + 1]
    const float* kp;                  // [n_slot][2]
    const int32_t* octave;            // [n_slot]
    const uint8_t* desc;              // [n_slot][32], 16-byte aligned
    const uint8_t* has_point;         // [n_slot]
    const float* Xw;                  // [n_slot][3]
    const float *dist_min_inv, *dist_max_inv, *dist_max;   // [n_slot]
    const uint8_t* mp_desc;           // [n_slot][32], 16-byte aligned
    const uint8_t *pre1, *pre2;       // [n_cand][n1], [off2[n_cand]]
    int32_t n_cand, n1;
};

// :1119-1121.  dir 0 (1 -> 2): M = sR21 = (1.0 / s12) * R12.t() (a double factor, rounded to float32 once), t = -sR21 * t12;
// dir 1 (2 -> 1): M = sR12 = s12 * R12, t = t12
__device__ inline void cand_transform(const CandP& C, int dir, float* M, float* t) {
#pragma clang fp contract(off)
    if (dir) {
        for (int i = 0; i < 9; ++i) M[i] = C.s12 * C.R12[i];
        for (int i = 0; i < 3; ++i) t[i] = C.t12[i];
    } else {
        const double is = 1.0 / (double)C.s12;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[3 * i + j] = (float)(is * (double)C.R12[3 * j + i]);
        for (int i = 0; i < 3; ++i) t[i] = -orb::rowdot(M + 3 * i, C.t12);
    }
}

// 4 waves per workgroup, one wave per (candidate, direction, source slot)
__global__ __launch_bounds__(256) void k_search_sim3_best(In in, int64_t n_work, int32_t* __restrict__ best1, int32_t* __restrict__ dist1,
                                                          int32_t* __restrict__ best2, int32_t* __restrict__ dist2) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_work) return;
    const int c = orb::owner_of(in.work_off, in.n_cand, w);
    const int32_t local = (int32_t)(w - in.work_off[c]);
    const int dir = local >= in.n1;
    const int32_t i = dir ? local - in.n1 : local;       // the source slot in its frame
    const FrameP& S = in.frame[dir ? 1 + c : 0];         // source and target frames
    const orb::GridP& T = in.frame[dir ? 0 : 1 + c].g;
    const CandP& C = in.cand[c];
    const int64_t out_at = dir ? (int64_t)in.off2[c] + i : (int64_t)c * in.n1 + i;
    int32_t* const best = dir ? best2 : best1;
    int32_t* const dist = dir ? dist2 : dist1;
    const int64_t s = (int64_t)S.g.off + i;
    int32_t res_best = -1, res_dist = -1;
    bool go = in.has_point[s] && !(dir ? in.pre2[out_at] : in.pre1[out_at]);
    float u = 0.f, v = 0.f, r = 0.f;
    int level = 0;
    orb::CellRange cells = {};
    if (go) {                                            // wave-uniform: every lane evaluates the slot's gates
        float M[9], tt[3], pc[3], p[3];
        cand_transform(C, dir, M, tt);
        for (int k = 0; k < 3; ++k) pc[k] = orb::rowdot(S.R + 3 * k, in.Xw + 3 * s) + S.t[k];     // Rcw * p3Dw + tcw
        for (int k = 0; k < 3; ++k) p[k] = orb::rowdot(M + 3 * k, pc) + tt[k];
        go = !(p[2] < 0.0f);                             // :1163 (a NaN passes here and fails IsInImage)
        const float invz = (float)(1.0 / (double)p[2]);
        const float x = p[0] * invz, y = p[1] * invz;
        u = C.K[0] * x + C.K[2];
        v = C.K[1] * y + C.K[3];
        go = go && u >= T.min_x && u < T.max_x && v >= T.min_y && v < T.max_y;
        const float d3 = (float)sqrt(((double)p[0] * (double)p[0] + (double)p[1] * (double)p[1]) + (double)p[2] * (double)p[2]);
        go = go && !(d3 < in.dist_min_inv[s] || d3 > in.dist_max_inv[s]);
        if (go) {
            level = orb::predict_scale(in.dist_max[s], d3, T.log_scale, T.n_levels);      // in the TARGET key frame
            r = C.th * T.sf[level];
            go = orb::cell_range<false>(T, u, v, r, cells) == orb::CELLS_OK;
        }
    }
    if (go) {
        const uint4* md = (const uint4*)(in.mp_desc + 32 * s);       // the map point's descriptor: once per wave, 8 dwords
        const uint4 m0 = md[0], m1 = md[1];
        unsigned long long key = orb::NO_KEY;
        for (int32_t j = lane; j < T.n; j += 64) {
            const int64_t g = (int64_t)T.off + j;
            const float2 k = ((const float2*)in.kp)[g];
            int cx, cy;
            if (!orb::cell_of(T, k, cx, cy) || !orb::in_range(cells, cx, cy)) continue;
            if (!orb::in_window(k, u, v, r)) continue;
            const int oct = in.octave[g];
            if (oct < level - 1 || oct > level) continue;
            const unsigned long long kk = orb::make_key(orb::hamming256(in.desc + 32 * g, m0, m1), cx, cy, j);
            key = kk < key ? kk : key;
        }
        key = wave_min(key);
        if (key != orb::NO_KEY) {
            res_dist = orb::key_dist(key);
            if (res_dist <= orb::TH_HIGH) res_best = orb::key_index(key);
        }
    }
    if (lane == 0) {
        best[out_at] = res_best;
        dist[out_at] = res_dist;
    }
}

// :1307-1323: one thread per (candidate, slot of key frame 1)
__global__ __launch_bounds__(256) void k_search_sim3_agree(In in, const int32_t* __restrict__ best1, const int32_t* __restrict__ best2,
                                                           int32_t* __restrict__ match12, int32_t* __restrict__ n_found) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)in.n_cand * in.n1) return;
    const int c = (int)(k / in.n1);
    const int32_t i1 = (int32_t)(k - (int64_t)c * in.n1);
    const int32_t b = best1[k];
    const bool ok = b >= 0 && best2[(int64_t)in.off2[c] + b] == i1;
    match12[k] = ok ? b : -1;
    if (ok) atomicAdd(n_found + c, 1);
}

}  // namespace search
}  // namespace qsp

extern "C" int qsp_search_by_sim3_batch(int device, const qsp_search_sim3_in* in, qsp_search_sim3_out* out) {
    using namespace qsp;
    if (!in) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: null input");
    if (in->n_cand < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: negative candidate count");
    if (in->n_cand == 0) return QSP_OK;
    if (!out || !out->match12 || !out->n_found) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: null output");
    if (!!out->best1 != !!out->dist1 || !!out->best1 != !!out->best2 || !!out->best1 != !!out->dist2)
        return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: the tap is four arrays or none");
    if (!in->kf1 || !in->kf2 || !in->K || !in->s12 || !in->R12 || !in->t12 || !in->th || !in->off2)
        return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: null argument");
    const int32_t nc = in->n_cand;
    const char* why = orb::orb_frame_problem(*in->kf1, true);
    if (why) return qsp_fail(QSP_ERR_INVALID, (std::string("qsp_search_by_sim3_batch: key frame 1: ") + why).c_str());
    const int32_t n1 = in->kf1->n;
    if (in->off2[0] != 0) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: offsets start at 0");
    for (int32_t c = 0; c < nc; ++c) {
        if (in->off2[c + 1] < in->off2[c]) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: offsets must not decrease");
        why = orb::orb_frame_problem(in->kf2[c], true);
        if (why) return qsp_fail(QSP_ERR_INVALID, (std::string("qsp_search_by_sim3_batch: key frame 2: ") + why).c_str());
        if (in->off2[c + 1] - in->off2[c] != in->kf2[c].n)
            return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: off2 does not step by the key-point count of key frame 2");
    }
    const int64_t n2_all = in->off2[nc];
    if (n1 && !in->pre1) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: null pre1");
    if (n2_all && !in->pre2) return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: null pre2");
    const int64_t n_slot = (int64_t)n1 + n2_all, n_out1 = (int64_t)nc * n1, n_work = n_out1 + n2_all;
    if (n_slot > 0x7fffffff || n_work > 0x7fffffff)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_search_by_sim3_batch: more than 2^31 - 1 key-point slots in one call");
    QSP_TRY(use_device(device, "qsp_search_by_sim3_batch"));
    // up   [frame | cand | work_off | off2 | kp | octave | desc | has_point | Xw | dist_min_inv | dist_max_inv | dist_max | mp_desc | pre1 | pre2]
    // down [match12 | best1 | dist1 | best2 | dist2 | n_found]
    const size_t ns = (size_t)n_slot, no1 = (size_t)n_out1, no2 = (size_t)n2_all, nf = (size_t)nc + 1;
    StagingLayout L;
    const size_t a_frame = L.take<search::FrameP>(nf), a_cand = L.take<search::CandP>((size_t)nc), a_work = L.take<int64_t>(nf),
                 a_off2 = L.take<int32_t>(nf), a_kp = L.take<float>(ns * 2), a_oct = L.take<int32_t>(ns), a_desc = L.take<uint8_t>(ns * 32),
                 a_has = L.take<uint8_t>(ns), a_Xw = L.take<float>(ns * 3), a_dmin = L.take<float>(ns), a_dmaxi = L.take<float>(ns),
                 a_dmax = L.take<float>(ns), a_mpd = L.take<uint8_t>(ns * 32), a_pre1 = L.take<uint8_t>(no1), a_pre2 = L.take<uint8_t>(no2);
    L.begin_down();
    const size_t a_match = L.take<int32_t>(no1), a_b1 = L.take<int32_t>(no1), a_d1 = L.take<int32_t>(no1), a_b2 = L.take<int32_t>(no2),
                 a_d2 = L.take<int32_t>(no2), a_found = L.take<int32_t>((size_t)nc);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes()))
        return qsp_fail(QSP_ERR_INVALID, "qsp_search_by_sim3_batch: out of host memory for the staging buffers");
    search::FrameP* fp = ptr<search::FrameP>(up.data(), a_frame);
    search::CandP* cp = ptr<search::CandP>(up.data(), a_cand);
    int64_t* work = ptr<int64_t>(up.data(), a_work);
    size_t slot = 0;
    for (int32_t f = 0; f <= nc; ++f) {
        const qsp_orb_frame& F = f ? in->kf2[f - 1] : *in->kf1;
        search::FrameP& P = fp[f];
        orb::fill_grid(P.g, F, slot);
        memcpy(P.R, F.Rcw, sizeof P.R);
        memcpy(P.t, F.tcw, sizeof P.t);
        const size_t n = (size_t)F.n;
        if (n) {
            memcpy(up.data() + a_kp + 8 * slot, F.kp, 8 * n);
            memcpy(up.data() + a_oct + 4 * slot, F.octave, 4 * n);
            memcpy(up.data() + a_desc + 32 * slot, F.desc, 32 * n);
            memcpy(up.data() + a_has + slot, F.has_point, n);
            memcpy(up.data() + a_Xw + 12 * slot, F.Xw, 12 * n);
            memcpy(up.data() + a_dmin + 4 * slot, F.dist_min_inv, 4 * n);
            memcpy(up.data() + a_dmaxi + 4 * slot, F.dist_max_inv, 4 * n);
            memcpy(up.data() + a_dmax + 4 * slot, F.dist_max, 4 * n);
            memcpy(up.data() + a_mpd + 32 * slot, F.mp_desc, 32 * n);
        }
        slot += n;
    }
    for (int32_t c = 0; c < nc; ++c) {
        search::CandP& C = cp[c];
        memcpy(C.K, in->K + 4 * (size_t)c, sizeof C.K);
        C.s12 = in->s12[c];
        memcpy(C.R12, in->R12 + 9 * (size_t)c, sizeof C.R12);
        memcpy(C.t12, in->t12 + 3 * (size_t)c, sizeof C.t12);
        C.th = in->th[c];
        work[c] = (int64_t)c * n1 + in->off2[c];
    }
    work[nc] = n_work;
    put(up, a_off2, in->off2, nf * 4); put(up, a_pre1, in->pre1, no1); put(up, a_pre2, in->pre2, no2);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    search::In k;
    k.frame = ptr<search::FrameP>(d, a_frame); k.cand = ptr<search::CandP>(d, a_cand);
    k.work_off = ptr<int64_t>(d, a_work); k.off2 = ptr<int32_t>(d, a_off2);
    k.kp = ptr<float>(d, a_kp); k.octave = ptr<int32_t>(d, a_oct); k.desc = ptr<uint8_t>(d, a_desc);
    k.has_point = ptr<uint8_t>(d, a_has); k.Xw = ptr<float>(d, a_Xw);
    k.dist_min_inv = ptr<float>(d, a_dmin); k.dist_max_inv = ptr<float>(d, a_dmaxi); k.dist_max = ptr<float>(d, a_dmax);
    k.mp_desc = ptr<uint8_t>(d, a_mpd); k.pre1 = ptr<uint8_t>(d, a_pre1); k.pre2 = ptr<uint8_t>(d, a_pre2);
    k.n_cand = nc; k.n1 = n1;
    int32_t* d_match = ptr<int32_t>(d, a_match);
    int32_t *d_b1 = ptr<int32_t>(d, a_b1), *d_d1 = ptr<int32_t>(d, a_d1), *d_b2 = ptr<int32_t>(d, a_b2), *d_d2 = ptr<int32_t>(d, a_d2);
    int32_t* d_found = ptr<int32_t>(d, a_found);
    // two launches and one fill on one stream, no host round trip in between
    QSP_HIP(hipMemsetAsync(d_found, 0, 4 * (size_t)nc, 0));
    if (n_work) {
        hipLaunchKernelGGL(search::k_search_sim3_best, dim3((unsigned)((n_work + 3) / 4)), dim3(256), 0, 0, k, n_work, d_b1, d_d1, d_b2, d_d2);
        QSP_HIP(hipGetLastError());
    }
    if (n_out1) {
        hipLaunchKernelGGL(search::k_search_sim3_agree, dim3((unsigned)((n_out1 + 255) / 256)), dim3(256), 0, 0, k, d_b1, d_b2, d_match, d_found);
        QSP_HIP(hipGetLastError());
    }
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    if (no1) memcpy(out->match12, h + L.in_down(a_match), 4 * no1);
    memcpy(out->n_found, h + L.in_down(a_found), 4 * (size_t)nc);
    if (out->best1) {
        if (no1) { memcpy(out->best1, h + L.in_down(a_b1), 4 * no1); memcpy(out->dist1, h + L.in_down(a_d1), 4 * no1); }
        if (no2) { memcpy(out->best2, h + L.in_down(a_b2), 4 * no2); memcpy(out->dist2, h + L.in_down(a_d2), 4 * no2); }
    }
    return QSP_OK;
}
