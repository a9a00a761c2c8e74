// fuse.hpp -- the match phase of both ORBmatcher::Fuse overloads (reference src/ORBmatcher.cc:825-975, the pose overload of
// LocalMapping::SearchInNeighbors, and :977-1100, the Sim3 overload of LoopClosing::SearchAndFuse) for ALL target key frames in one
// call.  Compiled in c_abi.cpp; the steps it shares with the other matchers are orb_match.hpp's, the wave reduction is wave.hpp's.
//
// Everything the reference computes up to (bestIdx, bestDist) reads only the map point (position, normal, distance limits,
// descriptor) and the target key frame (pose, intrinsics, key points, octaves, mvuRight, descriptors, grid); the map enters
// afterwards, in the action (GetMapPoint(bestIdx), Replace, AddObservation / AddMapPoint, vpReplacePoint[iMP] = ...), which stays
// on the host.  So ONE WAVE owns one (target, listed point): all 64 lanes evaluate the point's gates redundantly, then stride
// over the target's key points, each lane keeping the smallest orb::make_key it met, so one wave min-reduction yields the
// reference's `dist < bestDist` winner.  The points are a pool shared by all targets; a target lists the pool indices it searches.
//
// The two overloads differ in three places: the pose overload tests the reprojection error of each key point (:914-938,
// check = 1), the Sim3 overload does not; the pose overload writes 1 / z in float32 and the Sim3 overload 1.0 / z in double
// rounded to float32, which are the same float32 (the double quotient of two float32 values rounded once more is the correctly
// rounded float32 quotient); and bestDist starts at 256 in one and at INT_MAX in the other, which cannot differ either: both are
// above every Hamming distance of 256 bits (at most 256, and a distance of 256 is above TH_LOW = 50 and refused like INT_MAX).
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
namespace fuse {

enum Reason : int32_t { MATCHED = 0, Z_NEG, OUTSIDE, DISTANCE, ANGLE, EMPTY, NONE_ELIGIBLE, ABOVE_TH };

struct TargetP {
    orb::GridP g;
    float inv_sigma2[orb::MAX_LEVELS];
    float R[9], t[3], Ow[3];
    float K[5];                       // fx fy cx cy bf
    float th;
    int32_t check;                    // the reprojection test of the pose overload
};

struct In {
    const TargetP* target;            // [n_target]
    const int64_t* list_off;          // [n_target + 1]: target k owns the pairs [list_off[k], list_off[k + 1])
    const int32_t* list_idx;          // [n_pair] pool indices
    const float* kp;                  // [n_slot][2]
    const int32_t* octave;            // [n_slot]
    const uint8_t* desc;              // [n_slot][32], 16-byte aligned
    const float* u_right;             // [n_slot]
    const float *Xw, *normal;         // [n_point][3]
    const float *dist_min_inv, *dist_max_inv, *dist_max;   // [n_point]
    const uint8_t* mp_desc;           // [n_point][32], 16-byte aligned
    int32_t n_target;
};

// 4 waves per workgroup, one wave per (target, listed point)
__global__ __launch_bounds__(256) void k_fuse_best(In in, int64_t n_pair, int32_t* __restrict__ best, int32_t* __restrict__ dist,
                                                   int32_t* __restrict__ reason, int32_t* __restrict__ level_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_pair) return;
    const TargetP& T = in.target[orb::owner_of(in.list_off, in.n_target, w)];
    const orb::GridP& G = T.g;
    const int64_t s = in.list_idx[w];                    // the point in the pool
    int32_t res_best = -1, res_dist = -1, why = fuse::MATCHED, level = -1;
    float u = 0.f, v = 0.f, ur = 0.f, r = 0.f;
    orb::CellRange cells = {};
    {                                                    // wave-uniform: every lane evaluates the point's gates
        const float* X = in.Xw + 3 * s;
        float p[3], d3;
        double dot;
        for (int k = 0; k < 3; ++k) p[k] = orb::rowdot(T.R + 3 * k, X) + T.t[k];             // Rcw * p3Dw + tcw
        const float invz = (float)(1.0 / (double)p[2]);
        const float x = p[0] * invz, y = p[1] * invz;
        u = T.K[0] * x + T.K[2];
        v = T.K[1] * y + T.K[3];
        ur = u - T.K[4] * invz;
        orb::view_geometry(X, T.Ow, in.normal + 3 * s, &d3, &dot);
        if (p[2] < 0.0f) why = fuse::Z_NEG;              // :856 (a NaN passes here and fails IsInImage)
        else if (!(u >= G.min_x && u < G.max_x && v >= G.min_y && v < G.max_y)) why = fuse::OUTSIDE;
        else if (d3 < in.dist_min_inv[s] || d3 > in.dist_max_inv[s]) why = fuse::DISTANCE;
        else if (dot < 0.5 * (double)d3) why = fuse::ANGLE;
        else {
            level = orb::predict_scale(in.dist_max[s], d3, G.log_scale, G.n_levels);
            r = T.th * G.sf[level];
            if (orb::cell_range<false>(G, u, v, r, cells) != orb::CELLS_OK) why = fuse::EMPTY;
        }
    }
    if (why == fuse::MATCHED) {
        const uint4* md = (const uint4*)(in.mp_desc + 32 * s);       // the map point's descriptor: once per wave, 8 dwords
        const uint4 m0 = md[0], m1 = md[1];
        unsigned long long key = orb::NO_KEY;
        bool in_area = false;
        for (int32_t j = lane; j < G.n; j += 64) {
            const int64_t g = (int64_t)G.off + j;
            const float2 k = ((const float2*)in.kp)[g];
            int cx, cy;
            if (!orb::cell_of(G, k, cx, cy) || !orb::in_range(cells, cx, cy)) continue;
            if (!orb::in_window(k, u, v, r)) continue;
            in_area = true;                                          // vIndices holds it (:892)
            const int oct = in.octave[g];
            if (oct < level - 1 || oct > level) continue;
            if (T.check) {                                           // :914-938
                const float ex = u - k.x, ey = v - k.y, kr = in.u_right[g];
                float e2 = ex * ex + ey * ey;
                if (kr >= 0) {
                    const float er = ur - kr;
                    e2 = e2 + er * er;
                    if ((double)(e2 * T.inv_sigma2[oct]) > 7.8) continue;
                } else if ((double)(e2 * T.inv_sigma2[oct]) > 5.99) continue;
            }
            const unsigned long long kk = orb::make_key(orb::hamming256(in.desc + 32 * g, m0, m1), cx, cy, j);
            key = kk < key ? kk : key;
        }
        key = wave_min(key);
        if (key != orb::NO_KEY) {
            res_dist = orb::key_dist(key);
            if (res_dist <= orb::TH_LOW) res_best = orb::key_index(key);                         // :952 / :1082
            else why = fuse::ABOVE_TH;
        } else {
            why = __ballot(in_area) ? fuse::NONE_ELIGIBLE : fuse::EMPTY;
        }
    }
    if (lane == 0) {
        best[w] = res_best;
        dist[w] = res_dist;
        reason[w] = why;
        level_out[w] = level;
    }
}

}  // namespace fuse
}  // namespace qsp

extern "C" int qsp_fuse_batch(int device, const qsp_fuse_in* in, qsp_fuse_out* out) {
    using namespace qsp;
    const char* who = "qsp_fuse_batch";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!in) return bad(QSP_ERR_INVALID, "null input");
    if (in->n_target < 0) return bad(QSP_ERR_INVALID, "negative target count");
    if (in->n_target == 0) return QSP_OK;
    if (in->n_point < 0) return bad(QSP_ERR_INVALID, "negative point count");
    if (!in->target || !in->K || !in->Ow || !in->th || !in->u_right_off || !in->inv_level_sigma2 || !in->check_reprojection || !in->list_off)
        return bad(QSP_ERR_INVALID, "null argument");
    const int32_t nt = in->n_target;
    if (in->list_off[0] != 0) return bad(QSP_ERR_INVALID, "list_off starts at 0");
    if (in->u_right_off[0] != 0) return bad(QSP_ERR_INVALID, "u_right_off starts at 0");
    int64_t n_slot = 0;
    for (int32_t k = 0; k < nt; ++k) {
        if (in->list_off[k + 1] < in->list_off[k]) return bad(QSP_ERR_INVALID, "list_off must not decrease");
        const char* why = orb::orb_frame_problem(in->target[k], false);
        if (why) return bad(QSP_ERR_INVALID, std::string("target: ") + why);
        if ((int64_t)in->u_right_off[k + 1] - (int64_t)in->u_right_off[k] != in->target[k].n)
            return bad(QSP_ERR_INVALID, "u_right_off does not step by the key-point count of the target");
        n_slot += in->target[k].n;
    }
    const int64_t n_pair = in->list_off[nt];
    if (n_pair > 0x7fffffff || n_slot > 0x7fffffff) return bad(QSP_ERR_UNSUPPORTED, "more than 2^31 - 1 pairs or key-point slots in one call");
    if (n_slot && !in->u_right) return bad(QSP_ERR_INVALID, "null u_right");
    if (n_pair == 0) return QSP_OK;
    if (!in->list_idx) return bad(QSP_ERR_INVALID, "null list_idx");
    if (!in->Xw || !in->normal || !in->dist_min_inv || !in->dist_max_inv || !in->dist_max || !in->desc) return bad(QSP_ERR_INVALID, "null point array");
    for (int64_t i = 0; i < n_pair; ++i)
        if (in->list_idx[i] < 0 || in->list_idx[i] >= in->n_point) return bad(QSP_ERR_INVALID, "list_idx outside [0, n_point)");
    if (!out || !out->best_idx || !out->best_dist) return bad(QSP_ERR_INVALID, "null output");
    if (!!out->reason != !!out->level) return bad(QSP_ERR_INVALID, "the tap is two arrays or none");
    QSP_TRY(use_device(device, who));
    // up   [target | list_off | list_idx | kp | octave | desc | u_right | Xw | normal | dist_min_inv | dist_max_inv | dist_max | mp_desc]
    // down [best | dist | reason | level]
    const size_t ns = (size_t)n_slot, np = (size_t)in->n_point, nq = (size_t)n_pair;
    StagingLayout L;
    const size_t a_tgt = L.take<fuse::TargetP>((size_t)nt), a_loff = L.take<int64_t>((size_t)nt + 1), a_lidx = L.take<int32_t>(nq),
                 a_kp = L.take<float>(ns * 2), a_oct = L.take<int32_t>(ns), a_desc = L.take<uint8_t>(ns * 32), a_ur = L.take<float>(ns),
                 a_Xw = L.take<float>(np * 3), a_nrm = L.take<float>(np * 3), a_dmin = L.take<float>(np), a_dmaxi = L.take<float>(np),
                 a_dmax = L.take<float>(np), a_mpd = L.take<uint8_t>(np * 32);
    L.begin_down();
    const size_t a_best = L.take<int32_t>(nq), a_dist = L.take<int32_t>(nq), a_why = L.take<int32_t>(nq), a_lvl = L.take<int32_t>(nq);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    fuse::TargetP* tp = ptr<fuse::TargetP>(up.data(), a_tgt);
    size_t slot = 0;
    for (int32_t k = 0; k < nt; ++k) {
        const qsp_orb_frame& F = in->target[k];
        fuse::TargetP& P = tp[k];
        orb::fill_grid(P.g, F, slot);
        for (int l = 0; l < F.n_levels; ++l) P.inv_sigma2[l] = in->inv_level_sigma2[16 * (size_t)k + l];
        memcpy(P.R, F.Rcw, sizeof P.R);
        memcpy(P.t, F.tcw, sizeof P.t);
        memcpy(P.Ow, in->Ow + 3 * (size_t)k, sizeof P.Ow);
        memcpy(P.K, in->K + 5 * (size_t)k, sizeof P.K);
        P.th = in->th[k];
        P.check = in->check_reprojection[k] ? 1 : 0;
        const size_t n = (size_t)F.n;
        put(up, a_kp + 8 * slot, F.kp, 8 * n);
        put(up, a_oct + 4 * slot, F.octave, 4 * n);
        put(up, a_desc + 32 * slot, F.desc, 32 * n);
        put(up, a_ur + 4 * slot, in->u_right + in->u_right_off[k], 4 * n);
        slot += n;
    }
    put(up, a_loff, in->list_off, 8 * ((size_t)nt + 1)); put(up, a_lidx, in->list_idx, 4 * nq);
    put(up, a_Xw, in->Xw, 12 * np); put(up, a_nrm, in->normal, 12 * np); put(up, a_dmin, in->dist_min_inv, 4 * np);
    put(up, a_dmaxi, in->dist_max_inv, 4 * np); put(up, a_dmax, in->dist_max, 4 * np); put(up, a_mpd, in->desc, 32 * np);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    fuse::In k;
    k.target = ptr<fuse::TargetP>(d, a_tgt); k.list_off = ptr<int64_t>(d, a_loff); k.list_idx = ptr<int32_t>(d, a_lidx);
    k.kp = ptr<float>(d, a_kp); k.octave = ptr<int32_t>(d, a_oct); k.desc = ptr<uint8_t>(d, a_desc); k.u_right = ptr<float>(d, a_ur);
    k.Xw = ptr<float>(d, a_Xw); k.normal = ptr<float>(d, a_nrm);
    k.dist_min_inv = ptr<float>(d, a_dmin); k.dist_max_inv = ptr<float>(d, a_dmaxi); k.dist_max = ptr<float>(d, a_dmax);
    k.mp_desc = ptr<uint8_t>(d, a_mpd); k.n_target = nt;
    hipLaunchKernelGGL(fuse::k_fuse_best, dim3((unsigned)((n_pair + 3) / 4)), dim3(256), 0, 0, k, n_pair, ptr<int32_t>(d, a_best),
                       ptr<int32_t>(d, a_dist), ptr<int32_t>(d, a_why), ptr<int32_t>(d, a_lvl));
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    memcpy(out->best_idx, h + L.in_down(a_best), 4 * nq);
    memcpy(out->best_dist, h + L.in_down(a_dist), 4 * nq);
    if (out->reason) {
        memcpy(out->reason, h + L.in_down(a_why), 4 * nq);
        memcpy(out->level, h + L.in_down(a_lvl), 4 * nq);
    }
    return QSP_OK;
}
