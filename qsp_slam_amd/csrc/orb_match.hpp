// orb_match.hpp -- what the ORB matcher entry points share: the limits, a frame's grid parameters, and the steps every one of them
// takes as the reference writes them -- OpenCV's row product, the 256-bit Hamming distance, MapPoint::PredictScale, the cell range of
// GetFeaturesInArea, Frame::PosInGrid, the 64-bit key that carries the reference's traversal order, the viewing geometry, the two
// binary searches, and the rotation histogram's bin and ComputeThreeMaxima.  search_sim3.hpp, fuse.hpp, search_bow.hpp,
// search_triangulation.hpp and search_projection.hpp include it; what differs per entry point stays in its kernel.
//
// No grid is built anywhere: a key point is eligible when its own cell (cell_of) lies inside the grid and inside the visited range
// (in_range), and the reference's traversal order -- ascending (cell x, cell y, index) -- sits in the key under the distance
// (make_key), so one wave minimum yields the reference's `dist < bestDist` winner.
//
// Every function below evaluates with contraction OFF: the float32 operations of the reference in its order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace qsp {
namespace orb {

constexpr int MAX_LEVELS = 16;
constexpr int MAX_GRID = 64;
constexpr int MAX_KEYPOINTS = 1 << 26;   // the key keeps the key-point index in 26 bits
constexpr int TH_HIGH = 100;
constexpr int TH_LOW = 50;
constexpr int HISTO_LENGTH = 30;
constexpr unsigned long long NO_KEY = ~0ull;

struct GridP {                        // a frame's key-point slots and feature grid
    int32_t off, n;                   // its key-point slots are [off, off + n) of the flat arrays
    float min_x, max_x, min_y, max_y;
    int32_t cols, rows;
    float w_inv, h_inv;
    int32_t n_levels;
    float log_scale;
    float sf[MAX_LEVELS];
};

struct CellRange {
    int32_t min_cx, max_cx, min_cy, max_cy;
};
enum Cells { CELLS_OK, CELLS_EMPTY, CELLS_NONFINITE };

// cv::Mat R * X as OpenCV's small-matrix product leaves it: the row product summed in double and rounded to float once
__device__ inline float rowdot(const float* r, const float* X) {
#pragma clang fp contract(off)
    return (float)(((double)r[0] * (double)X[0] + (double)r[1] * (double)X[1]) + (double)r[2] * (double)X[2]);
}

__device__ inline int popc128(const uint4& a, const uint4& b) {
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

// ORBmatcher::DescriptorDistance of the 32 bytes at desc (16-byte aligned) and the descriptor a wave holds as m0, m1
__device__ inline int hamming256(const uint8_t* desc, const uint4& m0, const uint4& m1) {
    const uint4* d = (const uint4*)desc;
    return popc128(d[0], m0) + popc128(d[1], m1);
}

// MapPoint::PredictScale(dist3D, frame), MapPoint.cc:374-406, with the frame's mfLogScaleFactor and mnScaleLevels.  *fl is the level
// before the clamp, for a caller that refuses a NaN
__device__ inline int predict_scale(float dist_max, float d3, float log_scale, int n_levels, float* fl_out = nullptr) {
#pragma clang fp contract(off)
    const float ratio = dist_max / d3;
    const float fl = ceilf(logf(ratio) / log_scale);
    if (fl_out) *fl_out = fl;
    return fl < 0.f ? 0 : (fl >= (float)n_levels ? n_levels - 1 : (int)fl);
}

// GetFeaturesInArea's cell range and early returns, Frame.cc:369-383 and KeyFrame.cc:575-589.  GATE_NAN: a NaN among the four
// bounds (a NaN radius) is reported and c is left alone; without it the bounds go through the conversions as they are
template <bool GATE_NAN>
__device__ inline Cells cell_range(const GridP& G, float u, float v, float r, CellRange& c) {
#pragma clang fp contract(off)
    const float ax = ((u - G.min_x) - r) * G.w_inv, bx = ((u - G.min_x) + r) * G.w_inv;
    const float ay = ((v - G.min_y) - r) * G.h_inv, by = ((v - G.min_y) + r) * G.h_inv;
    if (GATE_NAN && (ax != ax || bx != bx || ay != ay || by != by)) return CELLS_NONFINITE;
    c.min_cx = max(0, (int)floorf(ax));
    c.max_cx = min(G.cols - 1, (int)ceilf(bx));
    c.min_cy = max(0, (int)floorf(ay));
    c.max_cy = min(G.rows - 1, (int)ceilf(by));
    return c.min_cx >= G.cols || c.max_cx < 0 || c.min_cy >= G.rows || c.max_cy < 0 ? CELLS_EMPTY : CELLS_OK;
}

// Frame::PosInGrid, Frame.cc:419-429: the cell the key point was filed under.  false: never filed, so never found
__device__ inline bool cell_of(const GridP& G, float2 kp, int& cx, int& cy) {
#pragma clang fp contract(off)
    cx = (int)roundf((kp.x - G.min_x) * G.w_inv);
    cy = (int)roundf((kp.y - G.min_y) * G.h_inv);
    return !(cx < 0 || cx >= G.cols || cy < 0 || cy >= G.rows);
}

__device__ inline bool in_range(const CellRange& c, int cx, int cy) {
    return !(cx < c.min_cx || cx > c.max_cx || cy < c.min_cy || cy > c.max_cy);
}

// GetFeaturesInArea's window around the projection (u, v), open at both ends
__device__ inline bool in_window(float2 kp, float u, float v, float r) {
#pragma clang fp contract(off)
    return fabsf(kp.x - u) < r && fabsf(kp.y - v) < r;
}

// distance, then the reference's traversal order: ascending (cell x, cell y, index)
__device__ inline unsigned long long make_key(int hd, int cx, int cy, int32_t j) {
    return ((unsigned long long)(unsigned)hd << 40) | ((unsigned long long)cx << 33) | ((unsigned long long)cy << 26) | (unsigned long long)j;
}
__device__ inline int32_t key_dist(unsigned long long key) { return (int32_t)(key >> 40); }
__device__ inline int32_t key_index(unsigned long long key) { return (int32_t)(key & (unsigned long long)(MAX_KEYPOINTS - 1)); }

// PO = X - Ow and its length, summed in double and rounded once
__device__ inline float view_geometry(const float* X, const float* Ow, float* PO) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) PO[k] = X[k] - Ow[k];
    return (float)sqrt(((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1]) + (double)PO[2] * (double)PO[2]);
}
// with the point's mean viewing direction: PO . normal as well, in double
__device__ inline void view_geometry(const float* X, const float* Ow, const float* Pn, float* d3, double* dot) {
#pragma clang fp contract(off)
    float PO[3];
    *d3 = view_geometry(X, Ow, PO);
    *dot = ((double)PO[0] * (double)Pn[0] + (double)PO[1] * (double)Pn[1]) + (double)PO[2] * (double)Pn[2];
}

// the last index whose offset is <= w, off[0] <= w being given: the owner of work item w (empty ranges are stepped over)
__device__ inline int owner_of(const int64_t* off, int n, int64_t w) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// std::lower_bound over ascending node ids: the first place whose id is not below `id`, n if there is none
__device__ inline int32_t lower_bound_id(const int32_t* ids, int32_t n, int32_t id) {
    int32_t a = 0, b = n;
    while (a < b) {
        const int32_t mid = a + ((b - a) >> 1);
        if (ids[mid] < id) a = mid + 1; else b = mid;
    }
    return a;
}

// ORBmatcher.cc:607-614 / :238-245 / :1433-1439.  factor = 1.0f / 30, so rot * factor lies in [0, 12]: only bins 0..12 ever fill
// and the `bin == 30` wrap never fires (a reference quirk, kept).  -1: an angle pair outside the reference's domain (its assert),
// counted in no bin
__host__ __device__ inline int rot_bin(float a_src, float a_tgt) {
#pragma clang fp contract(off)
    float rot = a_src - a_tgt;
    if (rot < 0.0f) rot += 360.0f;
    const float r = roundf(rot * (1.0f / HISTO_LENGTH));                // half away from zero
    if (!(r >= 0.0f && r <= (float)HISTO_LENGTH)) return -1;
    const int bin = (int)r;
    return bin == HISTO_LENGTH ? 0 : bin;
}

// ComputeThreeMaxima, ORBmatcher.cc:1601-1642, on bin counts
__host__ __device__ inline void three_maxima(const int* hist, int* ind) {
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < HISTO_LENGTH; ++i) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
    ind[0] = i1; ind[1] = i2; ind[2] = i3;
}

inline void fill_grid(GridP& P, const qsp_orb_frame& F, size_t off) {
    P.off = (int32_t)off; P.n = F.n;
    P.min_x = F.min_x; P.max_x = F.max_x; P.min_y = F.min_y; P.max_y = F.max_y;
    P.cols = F.grid_cols; P.rows = F.grid_rows; P.w_inv = F.grid_w_inv; P.h_inv = F.grid_h_inv;
    P.n_levels = F.n_levels; P.log_scale = F.log_scale;
    for (int l = 0; l < F.n_levels; ++l) P.sf[l] = F.scale_factors[l];
}

// what a call refuses in a frame; with_points: its map-point arrays are read as well
inline const char* orb_frame_problem(const qsp_orb_frame& f, bool with_points) {
    if (f.n < 0) return "negative key-point count";
    if (f.n > MAX_KEYPOINTS) return "more than 2^26 key points in a frame";
    if (f.grid_cols < 1 || f.grid_cols > MAX_GRID || f.grid_rows < 1 || f.grid_rows > MAX_GRID) return "grid outside 1..64 x 1..64";
    if (f.n_levels < 1 || f.n_levels > MAX_LEVELS) return "n_levels outside 1..16";
    if (!f.scale_factors) return "null scale_factors";
    if (f.n && (!f.kp || !f.octave || !f.desc)) return with_points ? "null frame array" : "null key-point array";
    if (with_points && f.n && (!f.has_point || !f.Xw || !f.dist_min_inv || !f.dist_max_inv || !f.dist_max || !f.mp_desc)) return "null frame array";
    for (int32_t i = 0; i < f.n; ++i)
        if (f.octave[i] < 0 || f.octave[i] >= f.n_levels) return "a key point's level outside [0, n_levels)";
    return nullptr;
}

}  // namespace orb
}  // namespace qsp
