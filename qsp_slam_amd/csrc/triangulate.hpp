// triangulate.hpp -- the numeric part of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:467-607, UnprojectStereo
// src/KeyFrame.cc:616-632) for ALL covisible neighbours in one call, on the match grid qsp_search_for_triangulation_batch
// returns.  Compiled in c_abi.cpp after search_triangulation.hpp, whose SearchPlan the chained call runs as it is.
//
// Every (neighbour k, source slot idx1) with idx2 = match[k][idx1] >= 0 is independent of every other up to one rule: the
// reference triangulates the neighbours in order, and a slot of key frame 1 that an earlier neighbour's pair filled no longer
// matches.  Of the neighbours that matched idx1, the FIRST whose pair passes every gate creates the point.  So k_tri_points
// evaluates every pair, ONE LANE per slot, and k_tri_first, one lane per idx1, walks the neighbours in order and marks that first
// one.  No atomics, no LDS, no wave operations: the lanes of a wave may diverge freely (SVD, UnprojectStereo of either side, or an
// early end), which costs a few hundred FP64 operations per lane in a call that is bound by its launches and copies.
//
// Arithmetic.  Float32 one IEEE operation at a time (contraction OFF) in the reference's order.  A CV_32F matrix product row is
// summed in double and rounded once (as orb_match.hpp's rowdot does; a vector added to the product is added in float32, as fuse.hpp
// does for Rcw * p + tcw -- NOT verified against OpenCV, where UnprojectStereo's `R * x3Dc + t` may fold into one gemm and round
// once: a known possible deviation of at most one ulp of a coordinate, listed in INTEGRATION.md).  Mat::dot and cv::norm return
// double: `Rcw.row(2).dot(x3Dt) + tcw.at<float>(2)` is a double sum rounded to float32 on assignment, and
// `ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2))` is formed in double throughout.  A float32
// quotient is the double quotient rounded once more (the correctly rounded float32 quotient, see search_triangulation.hpp).
// A compare against a double literal promotes the float32 side.  cos(2 * atan2(mb / 2, depth)) takes the float overloads in the
// reference; here each of the two functions is evaluated in double and rounded to float32, which is the correctly rounded float32
// value up to double rounding and within one ulp of any libm whose own error is below one ulp.
//
// The linear triangulation.  A (4x4) is formed in float32 as written (one multiply, one subtract per entry).  The right singular
// vector of its smallest singular value is computed in FP64 by a one-sided (Hestenes) Jacobi iteration on the columns: at most
// JACOBI_SWEEPS sweeps over the six column pairs, ended by the first sweep that rotates nothing.  OpenCV's float32 JacobiSVD is not
// restated: an FP64 null vector of the same float32 A lies inside the noise the float32 formulation itself has (a one-ulp change of
// A moves the point further), which tests/triangulate_oracle.py measures per pair.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "search_triangulation.hpp"

namespace qsp {
namespace tri {

constexpr int JACOBI_SWEEPS = 30;
enum PointReason : int32_t { ACCEPTED = 0, NO_MATCH, LOW_PARALLAX, W_ZERO, Z1_NEG, Z2_NEG, REPROJ1, REPROJ2, DIST_ZERO, SCALE_RATIO, NO_DEPTH };
enum PointPath : int32_t { PATH_NONE = 0, PATH_SVD, PATH_UNPROJECT1, PATH_UNPROJECT2 };

struct FrameG {
    int32_t off, n;                    // its slots are [off, off + n) of the flat arrays
    float R[9], t[3], Ow[3];           // Rcw, tcw, the camera centre
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
};

struct PointsIn {
    const FrameG* frame;               // [1 + n_cand]: key frame 1, then the neighbours
    const float *xy_un, *xy;           // [n_slot][2] mvKeysUn[i].pt, mvKeys[i].pt
    const float *u_right, *depth, *sigma2, *scale;   // [n_slot]
    int32_t n1;
    float ratio_factor;
};

struct PointsOut {
    uint8_t* accept;                   // [n_grid]
    float* x3D;                        // [n_grid][3]
    int32_t *reason, *path;            // the taps: all of them or none
    float *cos_rays, *z, *err2, *ratio_dist;
};

__device__ inline double dot3(const float* a, const float* b) {
#pragma clang fp contract(off)
    return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}
__device__ inline float quot(float a, float b) { return (float)((double)a / (double)b); }
// cos(2 * atan2(mb / 2, depth)), :488 / :490
__device__ inline float stereo_cos(float mb, float depth) {
#pragma clang fp contract(off)
    const float a = (float)atan2((double)(mb / 2.0f), (double)depth);
    return (float)cos((double)(2.0f * a));
}
// Rwc * x with Rwc = Rcw^T: row i of Rwc is column i of Rcw
__device__ inline void rot_t(const float* R, const float* x, float* y) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) y[i] = (float)(((double)R[i] * (double)x[0] + (double)R[3 + i] * (double)x[1]) + (double)R[6 + i] * (double)x[2]);
}

// The right singular vector of the smallest singular value of the 4x4 A (row-major), in FP64.  One-sided Jacobi: V accumulates the
// rotations that make the columns of U = A V orthogonal; their norms are the singular values.  Every index is a compile-time
// constant once the loops are unrolled, so U and V live in registers.
__device__ inline void null_vector(const float* A, double* v) {
#pragma clang fp contract(off)
    double U[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            U[i][j] = (double)A[4 * i + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    alpha += U[i][p] * U[i][p];
                    beta += U[i][q] * U[i][q];
                    gamma += U[i][p] * U[i][q];
                }
                // orthogonal to working precision (a zero column, or a NaN, never rotates)
                if (!(fabs(gamma) > 0x1p-52 * sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double up = U[i][p], uq = U[i][q], vp = V[i][p], vq = V[i][q];
                    U[i][p] = c * up - s * uq;
                    U[i][q] = s * up + c * uq;
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double best = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double n2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) n2 += U[i][j] * U[i][j];
        if (j == 0 || n2 < best) {
            best = n2;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = V[i][j];
        }
    }
}

// one lane per (neighbour, source slot); the buffers behind `o` were zeroed, so a lane that ends early leaves zeros
__global__ __launch_bounds__(256) void k_tri_points(PointsIn g, const int32_t* __restrict__ match, int64_t n_grid, PointsOut o) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_grid) return;
    const int k = (int)((unsigned)s / (unsigned)g.n1);                      // n_grid < 2^31
    const int32_t idx1 = (int32_t)((unsigned)s - (unsigned)k * (unsigned)g.n1);
    const int32_t idx2 = match[s];
    const FrameG& F1 = g.frame[0];
    const FrameG& F2 = g.frame[1 + k];
    if (idx2 < 0 || idx2 >= F2.n) {                                         // (the host refused an index >= n; the search never writes one)
        if (o.reason) o.reason[s] = NO_MATCH;
        return;
    }
    const int64_t g1 = (int64_t)F1.off + idx1, g2 = (int64_t)F2.off + idx2;
    const float ur1 = g.u_right[g1], ur2 = g.u_right[g2];
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;                              // :469, :473
    const float k1x = g.xy_un[2 * g1], k1y = g.xy_un[2 * g1 + 1], k2x = g.xy_un[2 * g2], k2y = g.xy_un[2 * g2 + 1];
    const float xn1[3] = {(k1x - F1.cx) * F1.invfx, (k1y - F1.cy) * F1.invfy, 1.0f};       // :476-477
    const float xn2[3] = {(k2x - F2.cx) * F2.invfx, (k2y - F2.cy) * F2.invfy, 1.0f};
    float ray1[3], ray2[3];
    rot_t(F1.R, xn1, ray1);                                                 // :479-480
    rot_t(F2.R, xn2, ray2);
    const float cos_rays = (float)(dot3(ray1, ray2) / (sqrt(dot3(ray1, ray1)) * sqrt(dot3(ray2, ray2))));   // :481
    float cs = cos_rays + 1.0f, cs1 = cs, cs2 = cs;
    if (st1) cs1 = stereo_cos(F1.mb, g.depth[g1]);                          // :487-490: the second only when the first is not stereo
    else if (st2) cs2 = stereo_cos(F2.mb, g.depth[g2]);
    cs = cs2 < cs1 ? cs2 : cs1;                                             // std::min
    int32_t why = ACCEPTED, path = PATH_NONE;
    float X[3] = {0.f, 0.f, 0.f}, z1 = 0.f, z2 = 0.f, e1 = 0.f, e2 = 0.f, ratio = 0.f;
    if (cos_rays < cs && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998)) {
        path = PATH_SVD;                                                    // :498-513
        float A[16];
        for (int j = 0; j < 4; ++j) {
            const float a1 = j < 3 ? F1.R[j] : F1.t[0], b1 = j < 3 ? F1.R[3 + j] : F1.t[1], c1 = j < 3 ? F1.R[6 + j] : F1.t[2];
            const float a2 = j < 3 ? F2.R[j] : F2.t[0], b2 = j < 3 ? F2.R[3 + j] : F2.t[1], c2 = j < 3 ? F2.R[6 + j] : F2.t[2];
            A[j] = xn1[0] * c1 - a1;
            A[4 + j] = xn1[1] * c1 - b1;
            A[8 + j] = xn2[0] * c2 - a2;
            A[12 + j] = xn2[1] * c2 - b2;
        }
        double v[4];
        null_vector(A, v);
        if ((float)v[3] == 0) why = W_ZERO;
        else for (int i = 0; i < 3; ++i) X[i] = (float)(v[i] / v[3]);
    } else if ((st1 && cs1 < cs2) || (st2 && cs2 < cs1)) {                  // :516-523, KeyFrame::UnprojectStereo
        const bool one = st1 && cs1 < cs2;
        path = one ? PATH_UNPROJECT1 : PATH_UNPROJECT2;
        const FrameG& F = one ? F1 : F2;
        const int64_t gi = one ? g1 : g2;
        const float z = g.depth[gi];
        if (!(z > 0)) why = NO_DEPTH;                                       // the reference returns an empty Mat and then dots it
        else {
            const float xc[3] = {(g.xy[2 * gi] - F.cx) * z * F.invfx, (g.xy[2 * gi + 1] - F.cy) * z * F.invfy, z};   // the DISTORTED mvKeys
            float y[3];
            rot_t(F.R, xc, y);
            for (int i = 0; i < 3; ++i) X[i] = y[i] + F.Ow[i];
        }
    } else {
        why = LOW_PARALLAX;                                                 // :524
    }
    if (why == ACCEPTED) {
        z1 = (float)(dot3(F1.R + 6, X) + (double)F1.t[2]);                  // :530
        if (z1 <= 0) why = Z1_NEG;
    }
    if (why == ACCEPTED) {
        z2 = (float)(dot3(F2.R + 6, X) + (double)F2.t[2]);                  // :534
        if (z2 <= 0) why = Z2_NEG;
    }
    if (why == ACCEPTED) {                                                  // :539-563
        const float x1 = (float)(dot3(F1.R, X) + (double)F1.t[0]), y1 = (float)(dot3(F1.R + 3, X) + (double)F1.t[1]);
        const float invz = (float)(1.0 / (double)z1);
        const float u = F1.fx * x1 * invz + F1.cx, v = F1.fy * y1 * invz + F1.cy;
        const float ex = u - k1x, ey = v - k1y;
        e1 = ex * ex + ey * ey;
        if (!st1) {
            if ((double)e1 > 5.991 * (double)g.sigma2[g1]) why = REPROJ1;
        } else {
            const float er = (u - F1.mbf * invz) - ur1;
            e1 = e1 + er * er;
            if ((double)e1 > 7.8 * (double)g.sigma2[g1]) why = REPROJ1;
        }
    }
    if (why == ACCEPTED) {                                                  // :566-589
        const float x2 = (float)(dot3(F2.R, X) + (double)F2.t[0]), y2 = (float)(dot3(F2.R + 3, X) + (double)F2.t[1]);
        const float invz = (float)(1.0 / (double)z2);
        const float u = F2.fx * x2 * invz + F2.cx, v = F2.fy * y2 * invz + F2.cy;
        const float ex = u - k2x, ey = v - k2y;
        e2 = ex * ex + ey * ey;
        if (!st2) {
            if ((double)e2 > 5.991 * (double)g.sigma2[g2]) why = REPROJ2;
        } else {
            const float er = (u - F1.mbf * invz) - ur2;                     // :582: key frame 1's mbf
            e2 = e2 + er * er;
            if ((double)e2 > 7.8 * (double)g.sigma2[g2]) why = REPROJ2;
        }
    }
    if (why == ACCEPTED) {                                                  // :592-607
        const float n1[3] = {X[0] - F1.Ow[0], X[1] - F1.Ow[1], X[2] - F1.Ow[2]};
        const float n2[3] = {X[0] - F2.Ow[0], X[1] - F2.Ow[1], X[2] - F2.Ow[2]};
        const float d1 = (float)sqrt(dot3(n1, n1)), d2 = (float)sqrt(dot3(n2, n2));
        if (d1 == 0 || d2 == 0) why = DIST_ZERO;
        else {
            ratio = quot(d2, d1);
            const float ro = quot(g.scale[g1], g.scale[g2]);
            if (ratio * g.ratio_factor < ro || ratio > ro * g.ratio_factor) why = SCALE_RATIO;
        }
    }
    o.accept[s] = why == ACCEPTED ? 1 : 0;
    for (int i = 0; i < 3; ++i) o.x3D[3 * s + i] = X[i];
    if (o.reason) {
        o.reason[s] = why;
        o.path[s] = path;
        o.cos_rays[s] = cos_rays;
        o.z[2 * s] = z1; o.z[2 * s + 1] = z2;
        o.err2[2 * s] = e1; o.err2[2 * s + 1] = e2;
        o.ratio_dist[s] = ratio;
    }
}

// one lane per source slot: of the neighbours whose pair was accepted, in order, the first creates the point
__global__ __launch_bounds__(256) void k_tri_first(const uint8_t* __restrict__ accept, int32_t n_cand, int32_t n1, uint8_t* __restrict__ first) {
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n1) return;
    bool taken = false;
    for (int32_t k = 0; k < n_cand; ++k) {
        const int64_t s = (int64_t)k * n1 + i;
        const bool a = accept[s] != 0;
        first[s] = (a && !taken) ? 1 : 0;
        taken = taken || a;
    }
}

static const char* geom_frame_problem(const qsp_triangulate_frame& f) {
    if (f.n < 0) return "negative key-point count";
    if (f.n && (!f.xy_un || !f.xy || !f.u_right || !f.depth || !f.sigma2 || !f.scale)) return "null key-point array";
    return nullptr;
}

// The host side in the steps of SearchPlan.  The match grid is either the caller's (qsp_triangulate_batch: checked and uploaded)
// or the search's, still on the device (qsp_create_new_map_points_batch).
struct PointsPlan {
    const qsp_triangulate_geom* geom = nullptr;
    int32_t nc = 0;
    int64_t n1 = 0, n_slot = 0, n_grid = 0;
    bool tap = false, own_match = false;
    size_t a_frame = 0, a_xyun = 0, a_xy = 0, a_ur = 0, a_depth = 0, a_sigma = 0, a_scale = 0, a_match = 0;
    size_t a_accept = 0, a_first = 0, a_x3D = 0, a_why = 0, a_path = 0, a_cos = 0, a_z = 0, a_err = 0, a_ratio = 0, a_end = 0;

    // geom->n_cand > 0 has been established by the caller
    int check(const qsp_triangulate_geom* geom_, const qsp_triangulate_out* out, const char* who) {
        auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
        geom = geom_;
        nc = geom->n_cand;
        if (!out || !out->accept || !out->first || !out->x3D || !out->n_new) return bad(QSP_ERR_INVALID, "null output");
        if (!geom->kf1 || !geom->kf2) return bad(QSP_ERR_INVALID, "null frames");
        for (int32_t f = 0; f <= nc; ++f) {
            const qsp_triangulate_frame& F = f ? geom->kf2[f - 1] : *geom->kf1;
            const char* why = geom_frame_problem(F);
            if (why) return bad(QSP_ERR_INVALID, std::string(f ? "neighbour key frame: " : "source key frame: ") + why);
            n_slot += F.n;
        }
        n1 = geom->kf1->n;
        n_grid = (int64_t)nc * n1;
        if (n_slot > 0x7fffffff || n_grid > 0x7fffffff) return bad(QSP_ERR_UNSUPPORTED, "more than 2^31 - 1 slots in one call");
        tap = out->reason || out->path || out->cos_rays || out->z || out->err2 || out->ratio_dist;
        return QSP_OK;
    }
    int check_match(const int32_t* match, const char* who) const {
        auto bad = [&](int code, const char* why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
        if (n_grid && !match) return bad(QSP_ERR_INVALID, "null match");
        for (int32_t k = 0; k < nc; ++k)
            for (int64_t i = 0; i < n1; ++i) {
                const int32_t m = match[(int64_t)k * n1 + i];
                if (m < -1 || m >= geom->kf2[k].n) return bad(QSP_ERR_INVALID, "a match index outside [-1, n) of its neighbour");
            }
        return QSP_OK;
    }
    // up      [frame | xy_un | xy | u_right | depth | sigma2 | scale | (match)]
    void take_up(StagingLayout& L, bool with_match) {
        const size_t ns = (size_t)n_slot;
        own_match = with_match;
        a_frame = L.take<FrameG>((size_t)nc + 1); a_xyun = L.take<float>(2 * ns); a_xy = L.take<float>(2 * ns); a_ur = L.take<float>(ns);
        a_depth = L.take<float>(ns); a_sigma = L.take<float>(ns); a_scale = L.take<float>(ns);
        if (with_match) a_match = L.take<int32_t>((size_t)n_grid);
    }
    // down    [accept | first | x3D | reason | path | cos_rays | z | err2 | ratio_dist], the taps only when one was asked for
    void take_down(StagingLayout& L) {
        const size_t no = (size_t)n_grid, nt = tap ? no : 0;
        a_accept = L.take<uint8_t>(no); a_first = L.take<uint8_t>(no); a_x3D = L.take<float>(3 * no);
        a_why = L.take<int32_t>(nt); a_path = L.take<int32_t>(nt); a_cos = L.take<float>(nt); a_z = L.take<float>(2 * nt);
        a_err = L.take<float>(2 * nt); a_ratio = L.take<float>(nt);
        a_end = L.take<char>(0);
    }
    void pack(std::vector<char>& up, const int32_t* match) const {
        FrameG* fp = ptr<FrameG>(up.data(), a_frame);
        size_t slot = 0;
        for (int32_t f = 0; f <= nc; ++f) {
            const qsp_triangulate_frame& F = f ? geom->kf2[f - 1] : *geom->kf1;
            FrameG& P = fp[f];
            const size_t n = (size_t)F.n;
            P.off = (int32_t)slot; P.n = F.n;
            memcpy(P.R, F.Rcw, sizeof P.R); memcpy(P.t, F.tcw, sizeof P.t); memcpy(P.Ow, F.Ow, sizeof P.Ow);
            P.fx = F.fx; P.fy = F.fy; P.cx = F.cx; P.cy = F.cy; P.invfx = F.invfx; P.invfy = F.invfy; P.mb = F.mb; P.mbf = F.mbf;
            put(up, a_xyun + 8 * slot, F.xy_un, 8 * n); put(up, a_xy + 8 * slot, F.xy, 8 * n);
            put(up, a_ur + 4 * slot, F.u_right, 4 * n); put(up, a_depth + 4 * slot, F.depth, 4 * n);
            put(up, a_sigma + 4 * slot, F.sigma2, 4 * n); put(up, a_scale + 4 * slot, F.scale, 4 * n);
            slot += n;
        }
        if (own_match) put(up, a_match, match, 4 * (size_t)n_grid);
    }
    // one fill and two launches on the stream the search's launches are on
    int launch(char* d, const int32_t* d_match) const {
        if (!n_grid) return QSP_OK;
        QSP_HIP(hipMemsetAsync(d + a_accept, 0, a_end - a_accept, 0));
        PointsIn g;
        g.frame = ptr<FrameG>(d, a_frame); g.xy_un = ptr<float>(d, a_xyun); g.xy = ptr<float>(d, a_xy); g.u_right = ptr<float>(d, a_ur);
        g.depth = ptr<float>(d, a_depth); g.sigma2 = ptr<float>(d, a_sigma); g.scale = ptr<float>(d, a_scale);
        g.n1 = (int32_t)n1; g.ratio_factor = geom->ratio_factor;
        PointsOut o;
        o.accept = ptr<uint8_t>(d, a_accept); o.x3D = ptr<float>(d, a_x3D);
        o.reason = tap ? ptr<int32_t>(d, a_why) : nullptr; o.path = ptr<int32_t>(d, a_path); o.cos_rays = ptr<float>(d, a_cos);
        o.z = ptr<float>(d, a_z); o.err2 = ptr<float>(d, a_err); o.ratio_dist = ptr<float>(d, a_ratio);
        hipLaunchKernelGGL(k_tri_points, dim3((unsigned)((n_grid + 255) / 256)), dim3(256), 0, 0, g, own_match ? ptr<int32_t>(d, a_match) : d_match,
                           n_grid, o);
        QSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tri_first, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, 0, o.accept, nc, (int32_t)n1, ptr<uint8_t>(d, a_first));
        QSP_HIP(hipGetLastError());
        return QSP_OK;
    }
    // h: a host copy of the DOWN region
    void copy_out(const char* h, const StagingLayout& L, qsp_triangulate_out* out) const {
        const size_t no = (size_t)n_grid;
        if (no) {
            memcpy(out->accept, h + L.in_down(a_accept), no);
            memcpy(out->first, h + L.in_down(a_first), no);
            memcpy(out->x3D, h + L.in_down(a_x3D), 12 * no);
            if (out->reason) memcpy(out->reason, h + L.in_down(a_why), 4 * no);
            if (out->path) memcpy(out->path, h + L.in_down(a_path), 4 * no);
            if (out->cos_rays) memcpy(out->cos_rays, h + L.in_down(a_cos), 4 * no);
            if (out->z) memcpy(out->z, h + L.in_down(a_z), 8 * no);
            if (out->err2) memcpy(out->err2, h + L.in_down(a_err), 8 * no);
            if (out->ratio_dist) memcpy(out->ratio_dist, h + L.in_down(a_ratio), 4 * no);
        }
        const uint8_t* first = ptr<uint8_t>(h, L.in_down(a_first));
        for (int32_t k = 0; k < nc; ++k) {
            int32_t n = 0;
            for (int64_t i = 0; i < n1; ++i) n += first[(int64_t)k * n1 + i];
            out->n_new[k] = n;
        }
    }
};

}  // namespace tri
}  // namespace qsp

extern "C" int qsp_triangulate_batch(int device, const qsp_triangulate_geom* geom, const int32_t* match, qsp_triangulate_out* out) {
    using namespace qsp;
    const char* who = "qsp_triangulate_batch";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!geom) return bad(QSP_ERR_INVALID, "null input");
    if (geom->n_cand < 0) return bad(QSP_ERR_INVALID, "negative candidate count");
    if (geom->n_cand == 0) return QSP_OK;
    tri::PointsPlan P;
    QSP_TRY(P.check(geom, out, who));
    QSP_TRY(P.check_match(match, who));
    QSP_TRY(use_device(device, who));
    StagingLayout L;
    P.take_up(L, true);
    L.begin_down();
    P.take_down(L);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    P.pack(up, match);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    QSP_TRY(P.launch(blk.data(), nullptr));
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    P.copy_out(down.data(), L, out);
    return QSP_OK;
}

extern "C" int qsp_create_new_map_points_batch(int device, const qsp_search_tri_in* in, const qsp_triangulate_geom* geom, qsp_search_tri_out* sout,
                                               qsp_triangulate_out* out) {
    using namespace qsp;
    const char* who = "qsp_create_new_map_points_batch";
    auto bad = [&](int code, const std::string& why) { return qsp_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!in || !geom) return bad(QSP_ERR_INVALID, "null input");
    if (in->n_cand < 0 || geom->n_cand < 0) return bad(QSP_ERR_INVALID, "negative candidate count");
    if (in->n_cand != geom->n_cand) return bad(QSP_ERR_INVALID, "the search input and the geometry hold different neighbour counts");
    if (in->n_cand == 0) return QSP_OK;
    tri::SearchPlan S;
    tri::PointsPlan P;
    QSP_TRY(S.check(in, sout, who));
    QSP_TRY(P.check(geom, out, who));
    // the search writes indices of ITS frames into the grid: the geometry must describe the same frames
    for (int32_t f = 0; f <= in->n_cand; ++f)
        if ((f ? in->kf2[f - 1] : *in->kf1).bow.n != (f ? geom->kf2[f - 1] : *geom->kf1).n)
            return bad(QSP_ERR_INVALID, "a key frame has different key-point counts in the search input and in the geometry");
    QSP_TRY(use_device(device, who));
    // one block: both calls' UP regions, then both calls' DOWN regions; the match grid never leaves the device in between
    StagingLayout L;
    S.take_up(L);
    P.take_up(L, false);
    L.begin_down();
    S.take_down(L);
    P.take_down(L);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes())) return bad(QSP_ERR_INVALID, "out of host memory for the staging buffers");
    S.pack(up);
    P.pack(up, nullptr);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    QSP_TRY(S.launch(blk.data()));
    QSP_TRY(P.launch(blk.data(), S.match_on_device(blk.data())));
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    S.copy_out(down.data(), L, sout);
    P.copy_out(down.data(), L, out);
    return QSP_OK;
}
