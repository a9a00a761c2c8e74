// search_projection_kf.hpp -- the two projection searches against a key frame's map points, with the result of the reference's
// SERIAL loop: RELOC = ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th,
// ORBdist) (reference src/ORBmatcher.cc:1472-1599, Tracking::Relocalization), SIM3 = SearchByProjection(KeyFrame* pKF, cv::Mat Scw,
// const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, th) (:290-403, LoopClosing::ComputeSim3).  Compiled in c_abi.cpp
// after search_projection.hpp, whose Rec, In, Out, k_proj_round, run_rounds and Action it uses as they are.
//
// Both loops skip a slot that holds ANY point (RELOC: CurrentFrame.mvpMapPoints[i2], SIM3: vpMatched[idx]) and every matched source
// writes its point there, so every source blocks: the fixed point of search_projection.hpp with src_blocks all ones.  Two sources
// can therefore never end on one slot -- the later one would have seen it taken -- and no slot is ever over-written.
//
// What differs from LOCAL / LAST is k_proj_gate_kf (one lane per source): RELOC has no depth test and the closed image test, SIM3
// refuses z < 0, has the half-open image test of KeyFrame::IsInImage and the viewing-angle test, and the two write 1 / z and u
// differently.  The rounds differ through three settings of k_proj_round: the accept threshold, no right-image test, and (SIM3) the
// octave window applied after the area instead of inside it.
//
// Every function below evaluates with contraction OFF: the float32 operations of the reference in its order.
#pragma once
#include "search_projection.hpp"

namespace qsp {
namespace proj {

// one lane per source.  o.proj_x, o.proj_y and o.level are the taps: of a source that passed every gate, else 0
__global__ __launch_bounds__(256) void k_proj_gate_kf(In in, Rec* __restrict__ rec, Out o) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= in.n_src) return;
    Rec rc = {};
    int32_t why = MATCHED, level = 0;
    bool gated = false;                                              // passed every gate: u, v and the level are outputs
    if (!in.src_valid[i]) why = INVALID_SRC;
    else {
        const float* X = in.Xw + 3 * i;
        float p[3];
        for (int k = 0; k < 3; ++k) p[k] = orb::rowdot(in.R + 3 * k, X) + in.t[k];        // Rcw * P + tcw
        float u, v;
        if (in.mode == RELOC) {
            const float invz = (float)(1.0 / (double)p[2]);          // :1502, and no test of its sign
            u = in.K[0] * p[0] * invz + in.K[2]; v = in.K[1] * p[1] * invz + in.K[3];
            if (u < in.g.min_x || u > in.g.max_x || v < in.g.min_y || v > in.g.max_y) why = OUTSIDE;  // :1507-1510, closed at both ends
            else if (u != u || v != v) why = NONFINITE;              // passes every compare above; the reference goes on to floor(NaN)
        } else {
            if (p[2] < 0.0f) why = Z_NEG;                            // :327 (-0.0 passes)
            const float invz = 1.0f / p[2];
            const float x = p[0] * invz, y = p[1] * invz;
            u = in.K[0] * x + in.K[2]; v = in.K[1] * y + in.K[3];
            // KeyFrame::IsInImage, half-open; a NaN fails it, as in the reference
            if (why == MATCHED && !(u >= in.g.min_x && u < in.g.max_x && v >= in.g.min_y && v < in.g.max_y)) why = OUTSIDE;
        }
        rc.u = u; rc.v = v; rc.ur = 0.f;
        if (why == MATCHED) {
            float PO[3];
            const float d3 = orb::view_geometry(X, in.Ow, PO);
            if (d3 < in.dist_min_inv[i] || d3 > in.dist_max_inv[i]) why = DISTANCE;
            if (why == MATCHED && in.mode == SIM3) {
                const float* Pn = in.normal + 3 * i;
                const double dot = ((double)PO[0] * (double)Pn[0] + (double)PO[1] * (double)Pn[1]) + (double)PO[2] * (double)Pn[2];
                if (dot < 0.5 * (double)d3) why = ANGLE;             // :354
            }
            if (why == MATCHED) {
                float fl;
                level = orb::predict_scale(in.dist_max[i], d3, in.g.log_scale, in.g.n_levels, &fl);
                if (d3 != d3 || fl != fl) why = NONFINITE;
                else {
                    const float r = in.th * in.g.sf[level];
                    rc.radius = r;
                    rc.lvl_min = level - 1;
                    rc.lvl_max = in.mode == RELOC ? level + 1 : level;                       // :1528 / :380
                    const orb::Cells cr = orb::cell_range<true>(in.g, u, v, r, rc.cells);
                    gated = cr != orb::CELLS_NONFINITE;                                     // NONFINITE: a NaN radius
                    if (cr != orb::CELLS_OK) why = gated ? EMPTY : NONFINITE;
                }
            }
        }
    }
    rc.reason = why;
    rec[i] = rc;
    o.choice[i] = -1; o.dist[i] = -1; o.reason[i] = why; o.dist2[i] = -1; o.level_best[i] = -1; o.level2[i] = -1;
    o.proj_x[i] = gated ? rc.u : 0.f;
    o.proj_y[i] = gated ? rc.v : 0.f;
    o.level[i] = gated ? level : 0;
}

}  // namespace proj
}  // namespace qsp

extern "C" int qsp_search_by_projection_kf(int device, const qsp_search_proj_kf_in* in, qsp_search_proj_kf_out* out) {
    using namespace qsp;
    const char* who = "qsp_search_by_projection_kf";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!in) return bad(QSP_ERR_INVALID, "null input");
    if (in->n_src < 0) return bad(QSP_ERR_INVALID, "negative source count");
    if (in->n_src == 0) return QSP_OK;
    if (in->n_src > orb::MAX_KEYPOINTS) return bad(QSP_ERR_INVALID, "more than 2^26 sources");
    if (in->mode != 0 && in->mode != 1) return bad(QSP_ERR_INVALID, "unknown mode");
    const bool reloc = in->mode == 0, ori = reloc && in->check_orientation;
    if (!reloc && in->orb_dist != orb::TH_LOW) return bad(QSP_ERR_INVALID, "SIM3 accepts at TH_LOW = 50 only");
    if (!reloc && in->check_orientation) return bad(QSP_ERR_INVALID, "SIM3 has no orientation check");
    if (!in->frame) return bad(QSP_ERR_INVALID, "null frame");
    const qsp_orb_frame& F = *in->frame;
    const char* why = orb::orb_frame_problem(F, false);
    if (why) return bad(QSP_ERR_INVALID, std::string("frame: ") + why);
    if (F.n && (!in->slot_blocked || (ori && !in->kp_angle))) return bad(QSP_ERR_INVALID, "null key-point array");
    if (!in->src_valid || !in->Xw || !in->desc || !in->dist_min_inv || !in->dist_max_inv || !in->dist_max) return bad(QSP_ERR_INVALID, "null source array");
    if (!reloc && !in->normal) return bad(QSP_ERR_INVALID, "null source array (SIM3)");
    if (ori && !in->src_angle) return bad(QSP_ERR_INVALID, "null source array (RELOC with the orientation check)");
    const int32_t ns = in->n_src, n = F.n;
    if (!out || !out->choice || !out->dist || (n && !out->slot_src)) return bad(QSP_ERR_INVALID, "null output");
    QSP_TRY(use_device(device, who));
    // up      [kp | octave | desc | slot_blocked | src_valid | Xw | src_desc | dist_min_inv | dist_max_inv | dist_max | normal]
    // scratch [rec | claim 0 | claim 1 | changed | dist2 | level_best | level2]  (the last three: k_proj_round writes them, nobody reads)
    // down    [choice | dist | reason | level | proj_x | proj_y]
    const size_t zn = (size_t)n, zs = (size_t)ns, zq = reloc ? 0 : zs;
    StagingLayout L;
    const size_t a_kp = L.take<float>(zn * 2), a_oct = L.take<int32_t>(zn), a_desc = L.take<uint8_t>(zn * 32), a_blk = L.take<uint8_t>(zn),
                 a_val = L.take<uint8_t>(zs), a_Xw = L.take<float>(zs * 3), a_sd = L.take<uint8_t>(zs * 32), a_dmin = L.take<float>(zs),
                 a_dmaxi = L.take<float>(zs), a_dmax = L.take<float>(zs), a_nrm = L.take<float>(zq * 3);
    L.begin_scratch();
    const size_t a_rec = L.take<proj::Rec>(zs), a_c0 = L.take<int32_t>(zn), a_c1 = L.take<int32_t>(zn), a_chg = L.take<int32_t>(1),
                 a_d2 = L.take<int32_t>(zs), a_l1 = L.take<int32_t>(zs), a_l2 = L.take<int32_t>(zs);
    L.begin_down();
    const size_t a_choice = L.take<int32_t>(zs), a_dist = L.take<int32_t>(zs), a_why = L.take<int32_t>(zs), a_lvl = L.take<int32_t>(zs),
                 a_px = L.take<float>(zs), a_py = L.take<float>(zs);
    std::vector<char> up, down;
    proj::Action act;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    if (!act.init(zn, zs)) return bad(QSP_ERR_INVALID, "out of host memory");
    put(up, a_kp, F.kp, 8 * zn); put(up, a_oct, F.octave, 4 * zn); put(up, a_desc, F.desc, 32 * zn); put(up, a_blk, in->slot_blocked, zn);
    put(up, a_val, in->src_valid, zs); put(up, a_Xw, in->Xw, 12 * zs); put(up, a_sd, in->desc, 32 * zs);
    put(up, a_dmin, in->dist_min_inv, 4 * zs); put(up, a_dmaxi, in->dist_max_inv, 4 * zs); put(up, a_dmax, in->dist_max, 4 * zs);
    if (!reloc) put(up, a_nrm, in->normal, 12 * zs);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    proj::In k = {};
    orb::fill_grid(k.g, F, 0);
    k.mode = reloc ? proj::RELOC : proj::SIM3; k.n_src = ns;
    memcpy(k.R, F.Rcw, sizeof k.R); memcpy(k.t, F.tcw, sizeof k.t); memcpy(k.Ow, in->Ow, sizeof k.Ow); memcpy(k.K, in->K, 4 * sizeof(float));
    k.th = in->th;
    k.accept_th = in->orb_dist; k.no_right = 1;
    k.kp = ptr<float>(d, a_kp); k.octave = ptr<int32_t>(d, a_oct); k.desc = ptr<uint8_t>(d, a_desc);
    k.slot_blocked = ptr<uint8_t>(d, a_blk); k.src_valid = ptr<uint8_t>(d, a_val);
    k.Xw = ptr<float>(d, a_Xw); k.src_desc = ptr<uint8_t>(d, a_sd); k.normal = ptr<float>(d, a_nrm);
    k.dist_min_inv = ptr<float>(d, a_dmin); k.dist_max_inv = ptr<float>(d, a_dmaxi); k.dist_max = ptr<float>(d, a_dmax);
    proj::Out o = {};
    o.choice = ptr<int32_t>(d, a_choice); o.dist = ptr<int32_t>(d, a_dist); o.reason = ptr<int32_t>(d, a_why); o.dist2 = ptr<int32_t>(d, a_d2);
    o.level_best = ptr<int32_t>(d, a_l1); o.level2 = ptr<int32_t>(d, a_l2);
    o.proj_x = ptr<float>(d, a_px); o.proj_y = ptr<float>(d, a_py); o.level = ptr<int32_t>(d, a_lvl);
    proj::Rec* d_rec = ptr<proj::Rec>(d, a_rec);
    hipLaunchKernelGGL(proj::k_proj_gate_kf, dim3((unsigned)((zs + 255) / 256)), dim3(256), 0, 0, k, d_rec, o);
    QSP_HIP(hipGetLastError());
    int32_t n_rounds = 0;
    QSP_TRY(proj::run_rounds(who, k, d_rec, ptr<int32_t>(d, a_c0), ptr<int32_t>(d, a_c1), ptr<int32_t>(d, a_chg), o, &n_rounds));
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    const int32_t* choice = ptr<int32_t>(h, L.in_down(a_choice));
    why = act.run(choice, ori, in->src_angle, in->kp_angle, in->slot_blocked, true);     // every source blocks: no two hold one slot
    if (why) return bad(QSP_ERR_DEVICE, why);
    // outputs are written only once everything has succeeded
    memcpy(out->choice, choice, 4 * zs);
    memcpy(out->dist, h + L.in_down(a_dist), 4 * zs);
    if (out->reason) memcpy(out->reason, h + L.in_down(a_why), 4 * zs);
    if (out->level) memcpy(out->level, h + L.in_down(a_lvl), 4 * zs);
    if (out->proj_x) memcpy(out->proj_x, h + L.in_down(a_px), 4 * zs);
    if (out->proj_y) memcpy(out->proj_y, h + L.in_down(a_py), 4 * zs);
    if (out->bin) memcpy(out->bin, act.bin.data(), 4 * zs);
    act.give(out);
    out->n_rounds = n_rounds;
    return QSP_OK;
}
