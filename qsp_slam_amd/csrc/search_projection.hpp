// search_projection.hpp -- the tracking thread's two projection searches with the result of the reference's SERIAL loop:
// LOCAL = Frame::isInFrustum (reference src/Frame.cc:306-362) + ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
// (src/ORBmatcher.cc:45-129), LAST = ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (:1328-1470).
// Compiled in c_abi.cpp; the steps it shares with the other matchers are orb_match.hpp's.
//
// The inner loop of both skips a key-point slot whose map point has observations, and earlier iterations of the same loop write
// those slots: source i sees slot idx as taken when it was taken at entry (slot_blocked) or when a source j < i whose own point has
// observations (src_blocks[j]) chose it.  Nothing else crosses between sources, so the serial loop is the unique fixed point of
//     choice[i] = match(i; blocked = initial U { choice[j] : j < i, src_blocks[j] })
// (unique by induction on i: choice[0] reads no other choice, choice[i] only those below it).  k_proj_round evaluates the right-hand
// side for all sources at once from the choices of the round before, handed over as claim[idx] = min { j : src_blocks[j], j chose
// idx } (an integer atomicMin: no arrival order in it); source i takes idx as blocked when claim[idx] < i.  After round r the
// sources 0 .. r - 1 hold their serial values, and a round that repeats the choices of the one before has reproduced its own claims:
// the fixed point.  The host reads one 4-byte `changed` word per round.
//
// k_proj_gate (one lane per source) computes what no round changes: projection, gates, level or octave window, radius, cell range.
// k_proj_round (one wave per source, four per workgroup; a wave whose source the gates refused leaves at once) strides over the
// frame's key points as k_fuse_best does and reduces to the two smallest keys.  The action phase (slot table, histogram,
// ComputeThreeMaxima, nulling) is index work and runs on the host after the download: Action::run, for both entry points.
//
// Every function below evaluates with contraction OFF: the float32 operations of the reference in its order.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "orb_match.hpp"
#include "staging.hpp"

namespace qsp {
namespace proj {

constexpr int32_t NO_CLAIM = 0x7fffffff;
enum Mode : int32_t { LOCAL = 0, LAST = 1, RELOC = 2, SIM3 = 3 };     // RELOC, SIM3: search_projection_kf.hpp, whose public 0 / 1 map onto them
enum Reason : int32_t { MATCHED = 0, INVALID_SRC, Z_NEG, OUTSIDE, DISTANCE, ANGLE, NONFINITE, EMPTY, NONE_ELIGIBLE, ABOVE_TH, RATIO };

struct Rec {                          // what k_proj_gate leaves per source for every round
    float u, v, ur, radius;
    orb::CellRange cells;
    int32_t lvl_min, lvl_max;         // the octave window, both ends included
    int32_t reason;                   // MATCHED: the rounds search for it
};

struct In {
    orb::GridP g;                     // the frame: its n key points are the arrays below from their start (off = 0)
    int32_t mode, n_src;
    float R[9], t[3], Ow[3];
    float K[5];                       // fx fy cx cy bf
    float th, nn_ratio, view_cos_limit;
    int32_t forward, backward;        // LAST: decided once on the host from tlc and mb
    const float* kp;                  // [n][2]
    const int32_t* octave;            // [n]
    const uint8_t* desc;              // [n][32], 16-byte aligned
    const float* u_right;             // [n]
    const uint8_t* slot_blocked;      // [n]
    const uint8_t *src_valid, *src_blocks;                 // [n_src]
    const float *Xw, *normal;         // [n_src][3]
    const float *dist_min_inv, *dist_max_inv, *dist_max;   // [n_src]
    const uint8_t* src_desc;          // [n_src][32], 16-byte aligned
    const int32_t* src_octave;        // [n_src]
    int32_t accept_th;                // the best is kept when its distance is <= accept_th (LOCAL, LAST: TH_HIGH)
    int32_t no_right;                 // 1: no right-image test, u_right is not read (RELOC, SIM3)
};

struct Out {                          // per source
    int32_t *choice, *dist, *reason, *dist2, *level_best, *level2;
    uint8_t* in_view;
    float *proj_x, *proj_y, *proj_xr, *view_cos;
    int32_t* level;
};

// one lane per source
__global__ __launch_bounds__(256) void k_proj_gate(In in, Rec* __restrict__ rec, Out o) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= in.n_src) return;
    Rec rc = {};
    int32_t why = MATCHED, level = 0;
    uint8_t in_view = 0;
    float view_cos = 0.f;
    if (!in.src_valid[i]) why = INVALID_SRC;
    else {
        const float* X = in.Xw + 3 * i;
        float p[3];
        for (int k = 0; k < 3; ++k) p[k] = orb::rowdot(in.R + 3 * k, X) + in.t[k];        // Rcw * P + tcw
        float invz;
        if (in.mode == LOCAL) {
            if (p[2] < 0.0f) why = Z_NEG;                            // Frame.cc:320 (-0.0 passes)
            invz = 1.0f / p[2];
        } else {
            invz = (float)(1.0 / (double)p[2]);                      // :1365
            if (invz < 0) why = Z_NEG;                               // :1367 (z == -0.0 is refused here, +0.0 is not)
        }
        const float u = in.K[0] * p[0] * invz + in.K[2], v = in.K[1] * p[1] * invz + in.K[3];
        rc.u = u; rc.v = v; rc.ur = u - in.K[4] * invz;
        if (why == MATCHED) {
            if (u < in.g.min_x || u > in.g.max_x || v < in.g.min_y || v > in.g.max_y) why = OUTSIDE;   // closed at both ends
            else if (u != u || v != v) why = NONFINITE;              // passes every compare above; the reference goes on to floor(NaN)
        }
        float r = 0.f;
        if (why == MATCHED && in.mode == LOCAL) {
            float d3;
            double dot;
            orb::view_geometry(X, in.Ow, in.normal + 3 * i, &d3, &dot);
            view_cos = (float)(dot / (double)d3);
            if (d3 < in.dist_min_inv[i] || d3 > in.dist_max_inv[i]) why = DISTANCE;
            else if (view_cos < in.view_cos_limit) why = ANGLE;
            else {
                float fl;
                level = orb::predict_scale(in.dist_max[i], d3, in.g.log_scale, in.g.n_levels, &fl);
                if (d3 != d3 || view_cos != view_cos || fl != fl) why = NONFINITE;
                else {
                    in_view = 1;
                    r = (double)view_cos > 0.998 ? 2.5f : 4.0f;      // RadiusByViewingCos
                    if ((double)in.th != 1.0) r = r * in.th;         // bFactor
                    r = r * in.g.sf[level];
                    rc.lvl_min = level - 1; rc.lvl_max = level;
                }
            }
        } else if (why == MATCHED) {
            const int oc = in.src_octave[i];                         // checked on the host: inside [0, n_levels)
            r = in.th * in.g.sf[oc];
            if (in.forward) { rc.lvl_min = oc; rc.lvl_max = orb::MAX_LEVELS; }
            else if (in.backward) { rc.lvl_min = 0; rc.lvl_max = oc; }
            else { rc.lvl_min = oc - 1; rc.lvl_max = oc + 1; }
        }
        if (why == MATCHED) {
            rc.radius = r;
            const orb::Cells cr = orb::cell_range<true>(in.g, u, v, r, rc.cells);
            if (cr != orb::CELLS_OK) why = cr == orb::CELLS_EMPTY ? EMPTY : NONFINITE;       // NONFINITE: a NaN radius
        }
    }
    rc.reason = why;
    rec[i] = rc;
    o.choice[i] = -1; o.dist[i] = -1; o.reason[i] = why; o.dist2[i] = -1; o.level_best[i] = -1; o.level2[i] = -1;
    o.in_view[i] = in_view;
    o.proj_x[i] = in_view ? rc.u : 0.f;
    o.proj_y[i] = in_view ? rc.v : 0.f;
    o.proj_xr[i] = in_view ? rc.ur : 0.f;
    o.view_cos[i] = in_view ? view_cos : 0.f;
    o.level[i] = in_view ? level : 0;
}

// the two smallest keys of two sorted pairs over disjoint sets
__device__ inline void merge2(unsigned long long& a1, unsigned long long& a2, unsigned long long b1, unsigned long long b2) {
    const unsigned long long lo = a1 < b1 ? a1 : b1, hi = a1 < b1 ? b1 : a1, m = a2 < b2 ? a2 : b2;
    a1 = lo;
    a2 = hi < m ? hi : m;
}

// 4 waves per workgroup, one wave per source; one launch per round
__global__ __launch_bounds__(256) void k_proj_round(In in, const Rec* __restrict__ rec, const int32_t* __restrict__ claim_prev,
                                                    int32_t* __restrict__ claim_next, int32_t* __restrict__ changed, Out o) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= in.n_src) return;
    const Rec rc = rec[i];
    if (rc.reason != MATCHED) return;                                // what k_proj_gate wrote for it stands
    const uint4* md = (const uint4*)(in.src_desc + 32 * i);
    const uint4 m0 = md[0], m1 = md[1];
    unsigned long long k1 = orb::NO_KEY, k2 = orb::NO_KEY;
    bool in_area = false;
    for (int32_t j = lane; j < in.g.n; j += 64) {
        const float2 k = ((const float2*)in.kp)[j];
        int cx, cy;
        if (!orb::cell_of(in.g, k, cx, cy) || !orb::in_range(rc.cells, cx, cy)) continue;
        const int oct = in.octave[j];
        const bool lvl_out = oct < rc.lvl_min || oct > rc.lvl_max;
        if (lvl_out && in.mode != SIM3) continue;                    // Frame::GetFeaturesInArea filters the levels itself
        if (!orb::in_window(k, rc.u, rc.v, rc.radius)) continue;
        in_area = true;                                              // vIndices holds it
        if (in.slot_blocked[j] || claim_prev[j] < i) continue;       // :87-89 / :1403-1405 / :1541 / :375
        if (lvl_out) continue;                                       // SIM3: KeyFrame::GetFeaturesInArea has no level filter, :380 has
        if (!in.no_right) {
            const float kr = in.u_right[j];
            if (kr > 0 && fabsf(rc.ur - kr) > rc.radius) continue;   // :91-96 / :1407-1413
        }
        const int hd = orb::hamming256(in.desc + 32 * (int64_t)j, m0, m1);
        if (hd >= 256) continue;                                     // never below the initial bestDist
        const unsigned long long kk = orb::make_key(hd, cx, cy, j);
        if (kk < k1) { k2 = k1; k1 = kk; }
        else if (kk < k2) k2 = kk;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) merge2(k1, k2, __shfl_xor(k1, m, 64), __shfl_xor(k2, m, 64));
    const bool any_area = __ballot(in_area) != 0;
    if (lane != 0) return;
    int32_t pick = -1, d1 = -1, d2 = -1, l1 = -1, l2 = -1, why = MATCHED;
    if (k1 == orb::NO_KEY) why = any_area ? NONE_ELIGIBLE : EMPTY;
    else {
        const int32_t b = orb::key_index(k1);
        d1 = orb::key_dist(k1);
        l1 = in.octave[b];
        if (k2 != orb::NO_KEY) {
            d2 = orb::key_dist(k2);
            l2 = in.octave[orb::key_index(k2)];
        }
        if (d1 > in.accept_th) why = ABOVE_TH;
        else if (in.mode == LOCAL && l1 == l2 && (float)d1 > in.nn_ratio * (float)d2) why = RATIO;   // :120 (no second: levels differ)
        else pick = b;
    }
    if (in.mode != LOCAL) { d2 = -1; l1 = -1; l2 = -1; }             // best only
    // `changed` follows the choice alone: a round with the choices of the one before was computed from the very claims those choices
    // make, so its dist, dist2, levels and reason are already the fixed point's
    if (o.choice[i] != pick) atomicOr(changed, 1);
    o.choice[i] = pick; o.dist[i] = d1; o.reason[i] = why; o.dist2[i] = d2; o.level_best[i] = l1; o.level2[i] = l2;
    if (pick >= 0 && (in.mode >= RELOC || in.src_blocks[i])) atomicMin(claim_next + pick, (int32_t)i);   // RELOC, SIM3: every source blocks
}

// The rounds on the host, for both entry points: round 1 sees the initial blocks only, every round reads the 4-byte `changed` word,
// and the claim tables swap.  claim0 and claim1 hold n int32 each; *n_rounds counts the launches.
inline int run_rounds(const char* who, const In& k, const Rec* d_rec, int32_t* claim0, int32_t* claim1, int32_t* d_chg, const Out& o,
                      int32_t* n_rounds_out) {
    const size_t zn = (size_t)k.g.n, zs = (size_t)k.n_src;
    int32_t* claim[2] = {claim0, claim1};
    if (zn) QSP_HIP(hipMemsetD32Async((hipDeviceptr_t)claim[0], NO_CLAIM, zn, 0));          // round 1: the initial blocks only
    int32_t n_rounds = 0;
    for (int32_t changed = 1; changed;) {
        // a round that still changes a choice after n_src + 1 of them contradicts the induction: a bug, never an input
        if (n_rounds > k.n_src)
            return qsp_fail(QSP_ERR_DEVICE, (std::string(who) + ": internal error: the rounds did not reach their fixed point").c_str());
        if (zn) QSP_HIP(hipMemsetD32Async((hipDeviceptr_t)claim[1], NO_CLAIM, zn, 0));
        QSP_HIP(hipMemsetAsync(d_chg, 0, 4, 0));
        hipLaunchKernelGGL(k_proj_round, dim3((unsigned)((zs + 3) / 4)), dim3(256), 0, 0, k, d_rec, claim[0], claim[1], d_chg, o);
        QSP_HIP(hipGetLastError());
        QSP_HIP(hipMemcpy(&changed, d_chg, 4, hipMemcpyDeviceToHost));
        std::swap(claim[0], claim[1]);
        ++n_rounds;
    }
    *n_rounds_out = n_rounds;
    return QSP_OK;
}

// The action phase on the host, for both entry points: the sources in order take their slots, the last writer of a slot stays
// (:123 / :1428); then the orientation check (:1433-1467 / :1562-1596): bins, histogram, three maxima, nulling.
struct Action {
    std::vector<int32_t> slot_src, bin;                              // [n], [n_src]
    int32_t n_matches = 0, hist[orb::HISTO_LENGTH] = {}, ind[3] = {-1, -1, -1};

    bool init(size_t n, size_t n_src) {
        try { slot_src.assign(n, -1); bin.assign(n_src, -1); } catch (const std::exception&) { return false; }
        return true;
    }
    // ori: the orientation check, over src_angle and kp_angle.  exclusive: every source blocks (RELOC, SIM3), so no two sources hold
    // one slot and none holds a slot taken at entry.  Returns what went wrong, or null
    const char* run(const int32_t* choice, bool ori, const float* src_angle, const float* kp_angle, const uint8_t* slot_blocked, bool exclusive) {
        const int32_t ns = (int32_t)bin.size(), n = (int32_t)slot_src.size();
        for (int32_t i = 0; i < ns; ++i) {
            const int32_t c = choice[i];
            if (c < 0) continue;
            if (c >= n) return "internal error: a choice outside the frame";
            if (exclusive && (slot_src[c] != -1 || slot_blocked[c])) return "internal error: a taken slot chosen";
            slot_src[c] = i;
            ++n_matches;
            if (ori) {
                bin[i] = orb::rot_bin(src_angle[i], kp_angle[c]);
                if (bin[i] >= 0) ++hist[bin[i]];
            }
        }
        if (ori) {
            orb::three_maxima(hist, ind);
            for (int32_t i = 0; i < ns; ++i)
                if (bin[i] >= 0 && bin[i] != ind[0] && bin[i] != ind[1] && bin[i] != ind[2]) {
                    slot_src[choice[i]] = -2;                        // also where a later source over-wrote it, as the reference does
                    --n_matches;
                }
        }
        return nullptr;
    }
    template <class O>
    void give(O* out) const {
        if (!slot_src.empty()) memcpy(out->slot_src, slot_src.data(), 4 * slot_src.size());
        out->n_matches = n_matches;
        memcpy(out->hist, hist, sizeof hist);
        memcpy(out->ind, ind, sizeof ind);
    }
};

}  // namespace proj
}  // namespace qsp

extern "C" int qsp_search_by_projection(int device, const qsp_search_proj_in* in, qsp_search_proj_out* out) {
    using namespace qsp;
    const char* who = "qsp_search_by_projection";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!in) return bad(QSP_ERR_INVALID, "null input");
    if (in->n_src < 0) return bad(QSP_ERR_INVALID, "negative source count");
    if (in->n_src == 0) return QSP_OK;
    if (in->n_src > orb::MAX_KEYPOINTS) return bad(QSP_ERR_INVALID, "more than 2^26 sources");
    if (in->mode != proj::LOCAL && in->mode != proj::LAST) return bad(QSP_ERR_INVALID, "unknown mode");
    const bool local = in->mode == proj::LOCAL, ori = !local && in->check_orientation;
    if (!in->frame) return bad(QSP_ERR_INVALID, "null frame");
    const qsp_orb_frame& F = *in->frame;
    const char* why = orb::orb_frame_problem(F, false);
    if (why) return bad(QSP_ERR_INVALID, std::string("frame: ") + why);
    if (F.n && (!in->u_right || !in->slot_blocked || (ori && !in->kp_angle))) return bad(QSP_ERR_INVALID, "null key-point array");
    if (!in->src_valid || !in->src_blocks || !in->Xw || !in->desc) return bad(QSP_ERR_INVALID, "null source array");
    if (local && (!in->normal || !in->dist_min_inv || !in->dist_max_inv || !in->dist_max)) return bad(QSP_ERR_INVALID, "null source array (LOCAL)");
    if (!local && (!in->src_octave || (ori && !in->src_angle))) return bad(QSP_ERR_INVALID, "null source array (LAST)");
    const int32_t ns = in->n_src, n = F.n;
    if (!out || !out->choice || !out->dist || (n && !out->slot_src)) return bad(QSP_ERR_INVALID, "null output");
    if (local && (!out->in_view || !out->proj_x || !out->proj_y || !out->proj_xr || !out->level || !out->view_cos))
        return bad(QSP_ERR_INVALID, "null output (LOCAL)");
    if (!local)
        for (int32_t i = 0; i < ns; ++i)
            if (in->src_valid[i] && (in->src_octave[i] < 0 || in->src_octave[i] >= F.n_levels))
                return bad(QSP_ERR_INVALID, "a source's octave outside [0, n_levels)");
    QSP_TRY(use_device(device, who));
    // up      [kp | octave | desc | u_right | slot_blocked | src_valid | src_blocks | Xw | src_desc | normal | dist_min_inv | dist_max_inv |
    //          dist_max | src_octave]
    // scratch [rec | claim 0 | claim 1 | changed]
    // down    [choice | dist | reason | dist2 | level_best | level2 | in_view | proj_x | proj_y | proj_xr | view_cos | level]
    const size_t zn = (size_t)n, zs = (size_t)ns, zl = local ? zs : 0, zo = local ? 0 : zs;
    StagingLayout L;
    const size_t a_kp = L.take<float>(zn * 2), a_oct = L.take<int32_t>(zn), a_desc = L.take<uint8_t>(zn * 32), a_ur = L.take<float>(zn),
                 a_blk = L.take<uint8_t>(zn), a_val = L.take<uint8_t>(zs), a_sblk = L.take<uint8_t>(zs), a_Xw = L.take<float>(zs * 3),
                 a_sd = L.take<uint8_t>(zs * 32), a_nrm = L.take<float>(zl * 3), a_dmin = L.take<float>(zl), a_dmaxi = L.take<float>(zl),
                 a_dmax = L.take<float>(zl), a_soct = L.take<int32_t>(zo);
    L.begin_scratch();
    const size_t a_rec = L.take<proj::Rec>(zs), a_c0 = L.take<int32_t>(zn), a_c1 = L.take<int32_t>(zn), a_chg = L.take<int32_t>(1);
    L.begin_down();
    const size_t a_choice = L.take<int32_t>(zs), a_dist = L.take<int32_t>(zs), a_why = L.take<int32_t>(zs), a_d2 = L.take<int32_t>(zs),
                 a_l1 = L.take<int32_t>(zs), a_l2 = L.take<int32_t>(zs), a_view = L.take<uint8_t>(zs), a_px = L.take<float>(zs),
                 a_py = L.take<float>(zs), a_pxr = L.take<float>(zs), a_cos = L.take<float>(zs), a_lvl = L.take<int32_t>(zs);
    std::vector<char> up, down;
    proj::Action act;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    if (!act.init(zn, zs)) return bad(QSP_ERR_INVALID, "out of host memory");
    put(up, a_kp, F.kp, 8 * zn); put(up, a_oct, F.octave, 4 * zn); put(up, a_desc, F.desc, 32 * zn); put(up, a_ur, in->u_right, 4 * zn);
    put(up, a_blk, in->slot_blocked, zn); put(up, a_val, in->src_valid, zs); put(up, a_sblk, in->src_blocks, zs);
    put(up, a_Xw, in->Xw, 12 * zs); put(up, a_sd, in->desc, 32 * zs);
    if (local) {
        put(up, a_nrm, in->normal, 12 * zs); put(up, a_dmin, in->dist_min_inv, 4 * zs); put(up, a_dmaxi, in->dist_max_inv, 4 * zs);
        put(up, a_dmax, in->dist_max, 4 * zs);
    } else put(up, a_soct, in->src_octave, 4 * zs);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    proj::In k = {};
    orb::fill_grid(k.g, F, 0);
    k.mode = in->mode; k.n_src = ns;
    memcpy(k.R, F.Rcw, sizeof k.R); memcpy(k.t, F.tcw, sizeof k.t); memcpy(k.Ow, in->Ow, sizeof k.Ow); memcpy(k.K, in->K, sizeof k.K);
    k.th = in->th; k.nn_ratio = in->nn_ratio; k.view_cos_limit = in->view_cos_limit;
    k.accept_th = orb::TH_HIGH; k.no_right = 0;
    if (!local) {
        // :1341-1349: twc = -Rcw^T tcw (a product scaled by -1: the double row sum rounded once, then negated), tlc = Rlw twc + tlw
        float twc[3];
        for (int c = 0; c < 3; ++c)
            twc[c] = -(float)(((double)F.Rcw[c] * (double)F.tcw[0] + (double)F.Rcw[3 + c] * (double)F.tcw[1]) + (double)F.Rcw[6 + c] * (double)F.tcw[2]);
        const float* r2 = in->last_Rcw + 6;
        const volatile float rz = (float)(((double)r2[0] * (double)twc[0] + (double)r2[1] * (double)twc[1]) + (double)r2[2] * (double)twc[2]);
        const float tlc_z = rz + in->last_tcw[2];
        k.forward = tlc_z > in->mb && !in->mono;
        k.backward = -tlc_z > in->mb && !in->mono;
    }
    k.kp = ptr<float>(d, a_kp); k.octave = ptr<int32_t>(d, a_oct); k.desc = ptr<uint8_t>(d, a_desc); k.u_right = ptr<float>(d, a_ur);
    k.slot_blocked = ptr<uint8_t>(d, a_blk); k.src_valid = ptr<uint8_t>(d, a_val); k.src_blocks = ptr<uint8_t>(d, a_sblk);
    k.Xw = ptr<float>(d, a_Xw); k.src_desc = ptr<uint8_t>(d, a_sd); k.normal = ptr<float>(d, a_nrm);
    k.dist_min_inv = ptr<float>(d, a_dmin); k.dist_max_inv = ptr<float>(d, a_dmaxi); k.dist_max = ptr<float>(d, a_dmax);
    k.src_octave = ptr<int32_t>(d, a_soct);
    proj::Out o;
    o.choice = ptr<int32_t>(d, a_choice); o.dist = ptr<int32_t>(d, a_dist); o.reason = ptr<int32_t>(d, a_why); o.dist2 = ptr<int32_t>(d, a_d2);
    o.level_best = ptr<int32_t>(d, a_l1); o.level2 = ptr<int32_t>(d, a_l2); o.in_view = ptr<uint8_t>(d, a_view);
    o.proj_x = ptr<float>(d, a_px); o.proj_y = ptr<float>(d, a_py); o.proj_xr = ptr<float>(d, a_pxr); o.view_cos = ptr<float>(d, a_cos);
    o.level = ptr<int32_t>(d, a_lvl);
    proj::Rec* d_rec = ptr<proj::Rec>(d, a_rec);
    hipLaunchKernelGGL(proj::k_proj_gate, dim3((unsigned)((zs + 255) / 256)), dim3(256), 0, 0, k, d_rec, o);
    QSP_HIP(hipGetLastError());
    int32_t n_rounds = 0;
    QSP_TRY(proj::run_rounds(who, k, d_rec, ptr<int32_t>(d, a_c0), ptr<int32_t>(d, a_c1), ptr<int32_t>(d, a_chg), o, &n_rounds));
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    const int32_t* choice = ptr<int32_t>(h, L.in_down(a_choice));
    why = act.run(choice, ori, in->src_angle, in->kp_angle, in->slot_blocked, false);
    if (why) return bad(QSP_ERR_DEVICE, why);
    // outputs are written only once everything has succeeded
    memcpy(out->choice, choice, 4 * zs);
    memcpy(out->dist, h + L.in_down(a_dist), 4 * zs);
    if (local) {
        memcpy(out->in_view, h + L.in_down(a_view), zs);
        memcpy(out->proj_x, h + L.in_down(a_px), 4 * zs); memcpy(out->proj_y, h + L.in_down(a_py), 4 * zs);
        memcpy(out->proj_xr, h + L.in_down(a_pxr), 4 * zs); memcpy(out->view_cos, h + L.in_down(a_cos), 4 * zs);
        memcpy(out->level, h + L.in_down(a_lvl), 4 * zs);
    }
    if (out->reason) memcpy(out->reason, h + L.in_down(a_why), 4 * zs);
    if (local && out->dist2) memcpy(out->dist2, h + L.in_down(a_d2), 4 * zs);
    if (local && out->level_best) memcpy(out->level_best, h + L.in_down(a_l1), 4 * zs);
    if (local && out->level2) memcpy(out->level2, h + L.in_down(a_l2), 4 * zs);
    if (ori && out->bin) memcpy(out->bin, act.bin.data(), 4 * zs);
    act.give(out);
    out->n_rounds = n_rounds;
    return QSP_OK;
}
