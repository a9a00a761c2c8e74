// sim3_ransac.hpp -- Sim3Solver (reference src/Sim3Solver.cc) for ALL loop candidates of a key frame in one call.  Compiled in
// c_abi.cpp.
//
// The reference's caller (LoopClosing::ComputeSim3, src/LoopClosing.cc:292-352) drives one Sim3Solver per candidate five RANSAC
// iterations at a time, round-robin.  Per candidate that is up to 300 hypotheses, each Horn's closed form on three point pairs
// (ComputeSim3, :226-337), two projections of every match and a threshold test (CheckInliers, :340-364); no hypothesis depends on
// an earlier one except through "stop at the first with more than minInliers inliers".  Here ONE WAVE evaluates one (candidate,
// hypothesis): all 64 lanes run Horn's step redundantly in registers (FP64 from the float32 inputs, T12 / T21 rounded to float32
// once), then stride over the candidate's matches in the reference's float32 arithmetic and count by ballot.  The random triples
// are the caller's (the reference draws them from one global rand() stream that interleaves across candidates).
//
// Every function below evaluates with contraction OFF: plain IEEE operations in the order written, NaN and inf included -- a
// degenerate triple (norm(vec) == 0 -> 0 / 0) makes every comparison of CheckInliers false and counts 0, as in the reference.
// k_sim3_ransac_select re-evaluates the winning hypothesis through the same device functions, so its flags are the bits the
// count came from.
#pragma once
#include <float.h>

#include <cstring>
#include <vector>

#include "staging.hpp"

namespace qsp {
namespace ransac {

constexpr int LDS_MATCHES = 256;      // a candidate of up to this many matches is staged on chip (12 floats per match)
constexpr int MAX_ITS = 1024;
constexpr int SWEEPS = 8;             // cyclic Jacobi sweeps over the 4x4 N: fixed, so that every wave runs the same instructions
constexpr unsigned NONE = 0xffffffffu;

struct In {
    const int32_t *off, *n_its, *trip_off, *triples;   // [n_cand + 1], [n_cand], [n_cand + 1], [n_trip][3]
    const float *K1, *K2;                               // [n_cand][4] fx fy cx cy
    const float *X1, *X2, *sig1, *sig2;                 // [n_match][3], [n_match][3], [n_match], [n_match]
    int32_t min_inliers, fix_scale;
};

struct Hyp {
    float T12[12], T21[12];           // rows of [sR | t], float32: what CheckInliers projects with
    float R[9], t[3], s;              // mR12i, mt12i, ms12i
};

struct Match {                        // what the constructor keeps per match, :81-109
    float X1[3], X2[3], p1[2], p2[2], max1, max2;
};

// FromCameraToImage, :405-423
__device__ inline void to_image(const float* X, const float* K, float* p) {
#pragma clang fp contract(off)
    const float invz = 1 / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    p[0] = K[0] * x + K[2];
    p[1] = K[1] * y + K[3];
}

__device__ inline Match derive(const In& in, const float* K1, const float* K2, int64_t k) {
#pragma clang fp contract(off)
    Match m;
    for (int i = 0; i < 3; ++i) { m.X1[i] = in.X1[3 * k + i]; m.X2[i] = in.X2[3 * k + i]; }
    to_image(m.X1, K1, m.p1);
    to_image(m.X2, K2, m.p2);
    m.max1 = (float)(9.210 * (double)in.sig1[k]);       // mvnMaxError1.push_back(9.210*sigmaSquare1): a double product, :87-88
    m.max2 = (float)(9.210 * (double)in.sig2[k]);
    return m;
}

// One Jacobi rotation that annihilates A[P][Q]; V collects the eigenvectors in its columns.  An exact zero is left alone (a
// diagonal N -- three points on a line parallel to an axis -- stays as it is); NaN != 0, so a NaN matrix rotates into NaNs.
template <int P, int Q>
__device__ inline void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
#pragma clang fp contract(off)
    const double apq = A[P][Q];
    if (apq != 0.0) {
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k == P || k == Q) continue;
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = A[P][k] = c * akp - s * akq;
            A[k][Q] = A[Q][k] = s * akp + c * akq;
        }
        A[P][P] = A[P][P] - t * apq;
        A[Q][Q] = A[Q][Q] + t * apq;
        A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][P], vkq = V[k][Q];
            V[k][P] = c * vkp - s * vkq;
            V[k][Q] = s * vkp + c * vkq;
        }
    }
}

// ComputeSim3, :226-337, on the pairs tri[0..2] of the candidate whose matches start at X1 / X2.  Wave-uniform: every lane computes
// the same hypothesis.
__device__ inline void horn(const float* X1, const float* X2, const int32_t* tri, int fix_scale, Hyp& H) {
#pragma clang fp contract(off)
    double P1[3][3], P2[3][3], O1[3], O2[3];             // [point][coordinate]
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) { P1[k][i] = (double)X1[3 * (int64_t)tri[k] + i]; P2[k][i] = (double)X2[3 * (int64_t)tri[k] + i]; }
    // step 1: centroids and relative coordinates
    for (int i = 0; i < 3; ++i) {
        O1[i] = ((P1[0][i] + P1[1][i]) + P1[2][i]) / 3.0;
        O2[i] = ((P2[0][i] + P2[1][i]) + P2[2][i]) / 3.0;
    }
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) { P1[k][i] -= O1[i]; P2[k][i] -= O2[i]; }
    // step 2: M = Pr2 * Pr1^T
    double M[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = (P2[0][i] * P1[0][j] + P2[1][i] * P1[1][j]) + P2[2][i] * P1[2][j];
    // step 3: N
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    // step 4: the eigenvector of the largest eigenvalue (cv::eigen's row 0), by cyclic Jacobi
#pragma unroll 1
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(A, V); jacobi_rotate<0, 2>(A, V); jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V); jacobi_rotate<1, 3>(A, V); jacobi_rotate<2, 3>(A, V);
    }
    double best = A[0][0], e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (A[j][j] > best) {                            // the first of equal eigenvalues stays
            best = A[j][j];
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = V[i][j];
        }
    // The eigenvector's sign is the solver's accident and does not matter: for -e the angle becomes atan2(n, -w) = pi - ang and
    // the axis -vec / n, and a turn of 2 pi - 2 ang about -u is the turn of 2 ang about u.  Rodrigues gives the same matrix.
    const double nv = sqrt((e[1] * e[1] + e[2] * e[2]) + e[3] * e[3]);
    const double ang = atan2(nv, e[0]);
    double rv[3];
    for (int i = 0; i < 3; ++i) rv[i] = ((2.0 * ang) * e[1 + i]) / nv;          // nv == 0: 0 / 0, NaN from here on
    // cv::Rodrigues
    double R[3][3];
    const double theta = sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2]);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
        const double r[3] = {rv[0] * it, rv[1] * it, rv[2] * it};
        const double rx[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = ((i == j ? c : 0.0) + c1 * (r[i] * r[j])) + s * rx[i][j];
    }
    // steps 5, 6: rotate set 2, scale
    double s12 = 1.0;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) {                // Mat::dot and the den loop walk the 3x3 [coordinate][point] row by row
                const double p3 = (R[i][0] * P2[k][0] + R[i][1] * P2[k][1]) + R[i][2] * P2[k][2];
                nom += P1[k][i] * p3;
                den += p3 * p3;
            }
        s12 = nom / den;
    }
    // steps 7, 8: t = O1 - s R O2, T12 = [sR | t], T21 = [sR^-1 | -sR^-1 t]
    double sR[3][3], t[3], sRi[3][3], ti[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) sR[i][j] = s12 * R[i][j];
    for (int i = 0; i < 3; ++i) t[i] = O1[i] - ((sR[i][0] * O2[0] + sR[i][1] * O2[1]) + sR[i][2] * O2[2]);
    const double is = 1.0 / s12;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) sRi[i][j] = is * R[j][i];
    for (int i = 0; i < 3; ++i) ti[i] = -((sRi[i][0] * t[0] + sRi[i][1] * t[1]) + sRi[i][2] * t[2]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            H.T12[4 * i + j] = (float)sR[i][j];
            H.T21[4 * i + j] = (float)sRi[i][j];
            H.R[3 * i + j] = (float)R[i][j];
        }
        H.T12[4 * i + 3] = H.t[i] = (float)t[i];
        H.T21[4 * i + 3] = (float)ti[i];
    }
    H.s = (float)s12;
}

// Project, :382-403, for one point: Rcw * X + tcw as OpenCV's small-matrix product leaves it (the row product summed in double and
// rounded to float, tcw added in float), then the pinhole in float32
__device__ inline void project(const float* T, const float* X, const float* K, float* p) {
#pragma clang fp contract(off)
    float c[3];
    for (int r = 0; r < 3; ++r) {
        const float rx = (float)(((double)T[4 * r] * (double)X[0] + (double)T[4 * r + 1] * (double)X[1]) + (double)T[4 * r + 2] * (double)X[2]);
        c[r] = rx + T[4 * r + 3];
    }
    to_image(c, K, p);
}

// CheckInliers' test for one match, :350-356 (Mat::dot sums float products in double); strict, false on NaN
__device__ inline bool is_inlier(const Hyp& H, const float* K1, const float* K2, const Match& m) {
#pragma clang fp contract(off)
    float q[2];
    project(H.T12, m.X2, K1, q);
    const float a0 = m.p1[0] - q[0], a1 = m.p1[1] - q[1];
    const float err1 = (float)((double)a0 * (double)a0 + (double)a1 * (double)a1);
    project(H.T21, m.X1, K2, q);
    const float b0 = q[0] - m.p2[0], b1 = q[1] - m.p2[1];
    const float err2 = (float)((double)b0 * (double)b0 + (double)b1 * (double)b1);
    return err1 < m.max1 && err2 < m.max2;
}

// grid (n_cand, ceil(max n_its / 4)), 4 waves: wave w of block (c, g) owns hypothesis 4 g + w of candidate c
__global__ __launch_bounds__(256) void k_sim3_ransac_count(In in, int32_t* __restrict__ hyp_count, unsigned* __restrict__ first) {
#pragma clang fp contract(off)
    __shared__ float lds[12][LDS_MATCHES];
    const int c = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_its = in.n_its[c];
    if ((int)blockIdx.y * 4 >= n_its) return;            // the whole workgroup: nothing left for this candidate
    const int64_t m0 = in.off[c];
    const int n = in.off[c + 1] - in.off[c];
    const float* K1 = in.K1 + 4 * (int64_t)c;
    const float* K2 = in.K2 + 4 * (int64_t)c;
    const bool staged = n <= LDS_MATCHES;
    if (staged) {
        if ((int)threadIdx.x < n) {
            const Match m = derive(in, K1, K2, m0 + threadIdx.x);
            const float v[12] = {m.X1[0], m.X1[1], m.X1[2], m.X2[0], m.X2[1], m.X2[2], m.p1[0], m.p1[1], m.p2[0], m.p2[1], m.max1, m.max2};
#pragma unroll
            for (int i = 0; i < 12; ++i) lds[i][threadIdx.x] = v[i];
        }
        __syncthreads();
    }
    const int h = blockIdx.y * 4 + wave;
    if (h >= n_its) return;
    const int64_t slot = (int64_t)in.trip_off[c] + h;
    Hyp H;
    horn(in.X1 + 3 * m0, in.X2 + 3 * m0, in.triples + 3 * slot, in.fix_scale, H);
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        bool ok = false;
        if (k < n) {
            Match m;
            if (staged) {
                m.X1[0] = lds[0][k]; m.X1[1] = lds[1][k]; m.X1[2] = lds[2][k];
                m.X2[0] = lds[3][k]; m.X2[1] = lds[4][k]; m.X2[2] = lds[5][k];
                m.p1[0] = lds[6][k]; m.p1[1] = lds[7][k]; m.p2[0] = lds[8][k]; m.p2[1] = lds[9][k];
                m.max1 = lds[10][k]; m.max2 = lds[11][k];
            } else {
                m = derive(in, K1, K2, m0 + k);
            }
            ok = is_inlier(H, K1, K2, m);
        }
        count += __popcll(__ballot(ok));
    }
    if (lane == 0) {
        hyp_count[slot] = count;
        // iterate() returns at the FIRST hypothesis with more than minInliers inliers (:192-199).  Every hypothesis before it had at
        // most minInliers, so mnBestInliers <= minInliers when it arrives and the `>= mnBestInliers` gate of :183 cannot hold it
        // back: the result is the smallest index whose count exceeds minInliers -- a min-reduction over the hypothesis index.
        if (count > in.min_inliers) atomicMin(first + c, (unsigned)h);
    }
}

// one wave per candidate: the winning hypothesis again, through the same device functions
__global__ __launch_bounds__(64) void k_sim3_ransac_select(In in, const unsigned* __restrict__ first, int32_t* __restrict__ first_it,
                                                           int32_t* __restrict__ n_inliers, float* __restrict__ R12, float* __restrict__ t12,
                                                           float* __restrict__ s12, uint8_t* __restrict__ inlier) {
#pragma clang fp contract(off)
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t m0 = in.off[c];
    const int n = in.off[c + 1] - in.off[c];
    const unsigned f = first[c];
    if (f == NONE) {                                     // "none": iteration 0, no inlier, a zero transform
        for (int k = lane; k < n; k += 64) inlier[m0 + k] = 0;
        if (lane < 9) R12[9 * (int64_t)c + lane] = 0.f;
        if (lane < 3) t12[3 * (int64_t)c + lane] = 0.f;
        if (lane == 0) { s12[c] = 0.f; first_it[c] = 0; n_inliers[c] = 0; }
        return;
    }
    const float* K1 = in.K1 + 4 * (int64_t)c;
    const float* K2 = in.K2 + 4 * (int64_t)c;
    Hyp H;
    horn(in.X1 + 3 * m0, in.X2 + 3 * m0, in.triples + 3 * ((int64_t)in.trip_off[c] + f), in.fix_scale, H);
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        bool ok = false;
        if (k < n) {
            ok = is_inlier(H, K1, K2, derive(in, K1, K2, m0 + k));
            inlier[m0 + k] = ok ? 1 : 0;
        }
        count += __popcll(__ballot(ok));
    }
    if (lane == 0) {
        for (int i = 0; i < 9; ++i) R12[9 * (int64_t)c + i] = H.R[i];
        for (int i = 0; i < 3; ++i) t12[3 * (int64_t)c + i] = H.t[i];
        s12[c] = H.s;
        first_it[c] = (int32_t)f + 1;
        n_inliers[c] = count;
    }
}

}  // namespace ransac

}  // namespace qsp

extern "C" int qsp_sim3_ransac_batch(int device, int32_t n_cand, const int32_t* match_off, const int32_t* n_its, const int32_t* trip_off,
                                     const int32_t* triples, const float* K1, const float* K2, const float* X1c, const float* X2c,
                                     const float* sigma2_1, const float* sigma2_2, int32_t min_inliers, int32_t fix_scale,
                                     int32_t* first_it, float* R12, float* t12, float* s12, uint8_t* inlier, int32_t* n_inliers,
                                     int32_t* hyp_inliers) {
    using namespace qsp;
    if (n_cand < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: negative candidate count");
    if (n_cand == 0) return QSP_OK;
    if (!match_off || !n_its || !trip_off || !K1 || !K2 || !first_it || !R12 || !t12 || !s12 || !n_inliers)
        return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: null argument");
    if (match_off[0] != 0 || trip_off[0] != 0) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: offsets start at 0");
    int max_its = 0;
    for (int c = 0; c < n_cand; ++c) {
        if (match_off[c + 1] < match_off[c] || trip_off[c + 1] < trip_off[c])
            return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: offsets must not decrease");
        if (n_its[c] < 0 || n_its[c] > trip_off[c + 1] - trip_off[c] || n_its[c] > ransac::MAX_ITS)
            return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: n_its outside [0, min(triples given, 1024)]");
        max_its = n_its[c] > max_its ? n_its[c] : max_its;
    }
    const size_t nc = (size_t)n_cand, nm = (size_t)match_off[n_cand], nt = (size_t)trip_off[n_cand];
    if (nm && (!X1c || !X2c || !sigma2_1 || !sigma2_2 || !inlier)) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: null match array");
    if (nt && !triples) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: null triples");
    for (int c = 0; c < n_cand; ++c) {
        const int32_t n = match_off[c + 1] - match_off[c];
        for (int32_t k = trip_off[c]; k < trip_off[c + 1]; ++k) {
            const int32_t a = triples[3 * (size_t)k], b = triples[3 * (size_t)k + 1], d = triples[3 * (size_t)k + 2];
            if (a < 0 || a >= n || b < 0 || b >= n || d < 0 || d >= n)
                return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: triple index out of range");
            if (a == b || a == d || b == d) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: a triple repeats an index");
        }
    }
    QSP_TRY(use_device(device, "qsp_sim3_ransac_batch"));
    // up      [off | n_its | trip_off | triples | K1 | K2 | X1 | X2 | sig1 | sig2]
    // scratch [first]
    // down    [first_it | n_inliers | R | t | s | hyp_count | inlier]
    StagingLayout L;
    const size_t a_off = L.take<int32_t>(nc + 1), a_its = L.take<int32_t>(nc), a_toff = L.take<int32_t>(nc + 1), a_tri = L.take<int32_t>(3 * nt),
                 a_K1 = L.take<float>(4 * nc), a_K2 = L.take<float>(4 * nc), a_X1 = L.take<float>(3 * nm), a_X2 = L.take<float>(3 * nm),
                 a_s1 = L.take<float>(nm), a_s2 = L.take<float>(nm);
    L.begin_scratch();
    const size_t a_first = L.take<unsigned>(nc);
    L.begin_down();
    const size_t a_first_it = L.take<int32_t>(nc), a_ninl = L.take<int32_t>(nc), a_R = L.take<float>(9 * nc), a_t = L.take<float>(3 * nc),
                 a_s = L.take<float>(nc), a_hyp = L.take<int32_t>(nt), a_inl = L.take<uint8_t>(nm);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes()))
        return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_ransac_batch: out of host memory for the staging buffers");
    put(up, a_off, match_off, 4 * (nc + 1)); put(up, a_its, n_its, 4 * nc); put(up, a_toff, trip_off, 4 * (nc + 1)); put(up, a_tri, triples, 12 * nt);
    put(up, a_K1, K1, 16 * nc); put(up, a_K2, K2, 16 * nc); put(up, a_X1, X1c, 12 * nm); put(up, a_X2, X2c, 12 * nm);
    put(up, a_s1, sigma2_1, 4 * nm); put(up, a_s2, sigma2_2, 4 * nm);
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    ransac::In in;
    in.off = ptr<int32_t>(d, a_off); in.n_its = ptr<int32_t>(d, a_its); in.trip_off = ptr<int32_t>(d, a_toff);
    in.triples = ptr<int32_t>(d, a_tri); in.K1 = ptr<float>(d, a_K1); in.K2 = ptr<float>(d, a_K2); in.X1 = ptr<float>(d, a_X1);
    in.X2 = ptr<float>(d, a_X2); in.sig1 = ptr<float>(d, a_s1); in.sig2 = ptr<float>(d, a_s2);
    in.min_inliers = min_inliers; in.fix_scale = fix_scale ? 1 : 0;
    int32_t *d_first_it = ptr<int32_t>(d, a_first_it), *d_ninl = ptr<int32_t>(d, a_ninl), *d_hyp = ptr<int32_t>(d, a_hyp);
    float *d_R = ptr<float>(d, a_R), *d_t = ptr<float>(d, a_t), *d_s = ptr<float>(d, a_s);
    uint8_t* d_inl = ptr<uint8_t>(d, a_inl);
    unsigned* d_first = ptr<unsigned>(d, a_first);
    // both kernels and the two fills on one stream, no host round trip in between
    if (nt) QSP_HIP(hipMemsetAsync(d_hyp, 0, 4 * nt, 0));                 // the triples beyond n_its count 0
    QSP_HIP(hipMemsetAsync(d_first, 0xff, 4 * nc, 0));                     // ransac::NONE
    if (max_its > 0) {
        hipLaunchKernelGGL(ransac::k_sim3_ransac_count, dim3(n_cand, (max_its + 3) / 4), dim3(256), 0, 0, in, d_hyp, d_first);
        QSP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ransac::k_sim3_ransac_select, dim3(n_cand), dim3(64), 0, 0, in, d_first, d_first_it, d_ninl, d_R, d_t, d_s, d_inl);
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    memcpy(first_it, h + L.in_down(a_first_it), 4 * nc);
    memcpy(n_inliers, h + L.in_down(a_ninl), 4 * nc);
    memcpy(R12, h + L.in_down(a_R), 36 * nc);
    memcpy(t12, h + L.in_down(a_t), 12 * nc);
    memcpy(s12, h + L.in_down(a_s), 4 * nc);
    if (hyp_inliers && nt) memcpy(hyp_inliers, h + L.in_down(a_hyp), 4 * nt);
    if (nm) memcpy(inlier, h + L.in_down(a_inl), nm);
    return QSP_OK;
}
