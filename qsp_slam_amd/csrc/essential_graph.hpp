// essential_graph.hpp -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:785-1048) from
// optimizer.initializeOptimization() to the corrected map points.  Compiled in c_abi.cpp; the dense factorisation is dense_chol.hpp's.
//
// The problem: n_kf VertexSim3Expmap in hessian order (ascending key-frame id; state tx ty tz qx qy qz qw s), a fixed flag per
// vertex, n_edge EdgeSim3 in insertion order with error log(Z S_v0 S_v1^-1) (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h
// :106-114, Sim3::log in sim3.h:148-231), identity information, no robust kernel, g2o's NUMERIC Jacobians (base_binary_edge.hpp:
// central differences through the vertex's oplus, delta 1e-9) and g2o's Levenberg-Marquardt
// (optimization_algorithm_levenberg.cpp:61-189) with the caller's lambda_init.
//
// Work split
//   k_eg_err     one lane per edge: the edge's error (7) and chi2.
//   k_eg_lin     32 lanes per edge, two edges per wave: lane l < 28 evaluates the error with vertex l / 14 moved by
//                (l & 1 ? -1 : +1) * 1e-9 along direction (l % 14) / 2; the even lane takes its odd neighbour's error by one
//                shuffle and writes column d of that vertex's Jacobian.  A fixed vertex gets no Jacobian (g2o skips it too).
//   k_eg_asm     one wave per FREE vertex i (= block row of H): lane (a, b) owns entry (a, b) of every 7x7 block of the row and
//                walks the vertex's incident edges in insertion order (CSR): H_ii += J_i^T J_i, H_ij += J_i^T J_j, b_i -= J_i^T e.
//                Every entry has one writer and one order; there are no floating-point atomics anywhere on this path, so two
//                calls on the same input return the same bits.  Rows and columns of fixed vertices do not exist.
//   solve        dense, ba::k_chol_first / ba::k_chol_step (one launch per 64-wide block step) on H + lambda I padded to the
//                block with an identity tail, then k_eg_back, this file's own block back-substitution (one workgroup).
//   k_eg_update  one lane per vertex: S <- exp(dx) S.     k_eg_reduce  one wave: chi2 and computeScale() in a fixed lane order.
//   k_eg_points  one lane per map point: S_out[r]^-1.map(S_in[r].map(p)).
// The host reads back four doubles per trial (chi2, rho's denominator, the factorisation's failure flag), as qsp_ba_optimize does.
//
// fix_scale: oplusImpl zeroes update[6], so the numeric scale column is exactly 0, the scale rows of H are lambda on the diagonal
// and 0 elsewhere, and x[6] = 0.  Those rows are DROPPED here: the system has 6 unknowns per free vertex.  x[6] = 0 adds exactly
// 0 to computeScale() -- whose lane order is that of the 7-wide numbering in both modes -- and the trial decisions see the same
// chi2, so what comes out is the 7-wide system's result up to the rounding of a factorisation blocked at other columns.
//
// The difference quotient multiplies the rounding of an error evaluation by 5e8: everything from the states to the error runs
// with contraction OFF in the order written (sim3:: helpers; log7 below in the same style), which tests/essential_oracle.py
// restates operation for operation.  Sim3::log's W.lu().solve(t) is restated as Eigen's 3x3 partial-pivot LU with its unrolled
// triangular solves (lu3_solve).
#pragma once
#include <algorithm>
#include <mutex>

#include "dense_chol.hpp"
#include "se3.hpp"
#include "sim3_opt.hpp"
#include "staging.hpp"
#include "wave.hpp"

namespace qsp {
namespace eg {

constexpr int DIM_MAX = 10208;      // unknowns of the dense factorisation (1 458 free key frames at 7)
constexpr int TRACE_MAX = 32;       // iterations qsp_essential_trace records

// Quaterniond::toRotationMatrix (Eigen), row-major
__device__ inline void rotmat(const double* q, double* R) {
#pragma clang fp contract(off)
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

__device__ inline void swap_row(double* a, double* b) {
    for (int i = 0; i < 4; ++i) { const double t = a[i]; a[i] = b[i]; b[i] = t; }
}
// W x = t by partial-pivot LU, rows (w0 w1 w2 | t) swapped whole; L kept in place below the diagonal; then
// y1 = t1 - l10 y0, y2 = t2 - (l20 y0 + l21 y1), x2 = y2 / u22, x1 = (y1 - u12 x2) / u11, x0 = (y0 - (u01 x1 + u02 x2)) / u00
__device__ inline void lu3_solve(const double* W, const double* t, double* x) {
#pragma clang fp contract(off)
    double r0[4] = {W[0], W[1], W[2], t[0]}, r1[4] = {W[3], W[4], W[5], t[1]}, r2[4] = {W[6], W[7], W[8], t[2]};
    if (fabs(r1[0]) > fabs(r0[0])) swap_row(r0, r1);
    if (fabs(r2[0]) > fabs(r0[0])) swap_row(r0, r2);
    r1[0] = r1[0] / r0[0];
    r2[0] = r2[0] / r0[0];
    r1[1] = r1[1] - r1[0] * r0[1]; r1[2] = r1[2] - r1[0] * r0[2];
    r2[1] = r2[1] - r2[0] * r0[1]; r2[2] = r2[2] - r2[0] * r0[2];
    if (fabs(r2[1]) > fabs(r1[1])) swap_row(r1, r2);
    r2[1] = r2[1] / r1[1];
    r2[2] = r2[2] - r2[1] * r1[2];
    const double y0 = r0[3];
    const double y1 = r1[3] - r1[0] * y0;
    const double y2 = r2[3] - (r2[0] * y0 + r2[1] * y1);
    x[2] = y2 / r2[2];
    x[1] = (y1 - r1[2] * x[2]) / r1[1];
    x[0] = (y0 - (r0[1] * x[1] + r0[2] * x[2])) / r0[0];
}

// Sim3::log: omega (3), upsilon (3), sigma
__device__ inline void log7(const double* S, double* u) {
#pragma clang fp contract(off)
    const double s = S[7], sigma = log(s), eps = 0.00001;
    double R[9], om[3], Om[9], Om2[9], W[9];
    rotmat(S + 3, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta, f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d), f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
            const double theta2 = theta * theta, a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    ba::skew3(om, Om);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    for (int i = 0; i < 9; ++i) W[i] = (A * Om[i] + B * Om2[i]) + ((i % 4 == 0) ? C : 0.0);
    lu3_solve(W, S, u + 3);
    for (int i = 0; i < 3; ++i) u[i] = om[i];
    u[6] = sigma;
}

// EdgeSim3::computeError: log((Z * S0) * S1^-1)
__device__ inline void edge_err(const double* Z, const double* S0, const double* S1, double* e) {
#pragma clang fp contract(off)
    double A[8], Bi[8], Er[8];
    sim3::mul(Z, S0, A);
    sim3::inv(S1, Bi);
    sim3::mul(A, Bi, Er);
    log7(Er, e);
}

struct Graph {
    int n_kf, n_edge, n_free, D, fix_scale, ld;
    const int32_t *v0, *v1;          // [n_edge]
    const int32_t *slot;             // [n_kf]: index among the free vertices, -1 = fixed
    const int32_t *free_v;           // [n_free]
    const int32_t *inc_off, *inc;    // CSR over vertices: (edge << 1) | side, in insertion order
    const double* Z;                 // [n_edge][8]
    double *E, *chi, *J;             // [n_edge][7], [n_edge], [n_edge][2][7 directions][7 error rows]
};

__global__ __launch_bounds__(64) void k_eg_err(Graph g, const double* __restrict__ S) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= g.n_edge) return;
    double e[7];
    edge_err(g.Z + 8 * (int64_t)k, S + 8 * (int64_t)g.v0[k], S + 8 * (int64_t)g.v1[k], e);
    double c = e[0] * e[0];
    for (int i = 1; i < 7; ++i) c = c + e[i] * e[i];
    for (int i = 0; i < 7; ++i) g.E[7 * (int64_t)k + i] = e[i];
    g.chi[k] = c;
}

__global__ __launch_bounds__(64) void k_eg_lin(Graph g, const double* __restrict__ S) {
#pragma clang fp contract(off)
    const int l = threadIdx.x & 31, k = blockIdx.x * 2 + (threadIdx.x >> 5);
    const int side = l / 14, d = (l % 14) >> 1, sgn = l & 1;
    double e[7] = {0, 0, 0, 0, 0, 0, 0};
    bool act = k < g.n_edge && l < 28;
    if (act) act = g.slot[side ? g.v1[k] : g.v0[k]] >= 0;
    if (act) {
        const double *S0 = S + 8 * (int64_t)g.v0[k], *S1 = S + 8 * (int64_t)g.v1[k];
        const double step = (g.fix_scale && d == 6) ? 0.0 : 1e-9;              // VertexSim3Expmap::oplusImpl: update[6] = 0
        double u[7], X[8], T[8];
        for (int i = 0; i < 7; ++i) u[i] = (i == d) ? (sgn ? -step : step) : 0.0;
        sim3::exp7(u, X);
        sim3::mul(X, side ? S1 : S0, T);
        edge_err(g.Z + 8 * (int64_t)k, side ? S0 : T, side ? T : S1, e);
    }
    const double scalar = 1.0 / (2 * 1e-9);
    double* Jc = g.J + ((2 * (int64_t)(k < g.n_edge ? k : 0) + side % 2) * 7 + d) * 7;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double o = __shfl_xor(e[i], 1, 64);                              // (every lane of the wave takes part)
        if (act && !sgn) Jc[i] = scalar * (e[i] - o);
    }
}

// H is dense, row-major, pitch ld, zero on entry; bvec has D n_free entries
__global__ __launch_bounds__(64) void k_eg_asm(Graph g, double* __restrict__ H, double* __restrict__ bvec) {
#pragma clang fp contract(off)
    const int fi = blockIdx.x, v = g.free_v[fi], lane = threadIdx.x, a = lane / 7, b = lane % 7, D = g.D;
    if (lane >= 49 || a >= D || b >= D) return;
    double hii = 0, bi = 0;
    for (int p = g.inc_off[v]; p < g.inc_off[v + 1]; ++p) {
        const int ent = g.inc[p], k = ent >> 1, s = ent & 1;
        const double* Je = g.J + 98 * (int64_t)k;
        const double *Ja = Je + (7 * s + a) * 7, *Jb = Je + (7 * s + b) * 7;
        double t = Ja[0] * Jb[0];
        for (int r = 1; r < 7; ++r) t = t + Ja[r] * Jb[r];
        hii = hii + t;
        const int fo = g.slot[s ? g.v0[k] : g.v1[k]];
        if (fo >= 0) {
            const double* Jo = Je + (7 * (1 - s) + b) * 7;
            double t2 = Ja[0] * Jo[0];
            for (int r = 1; r < 7; ++r) t2 = t2 + Ja[r] * Jo[r];
            double* h = H + (size_t)(fi * D + a) * g.ld + fo * D + b;
            *h = *h + t2;                                                       // (this lane is the entry's only writer)
        }
        if (b == 0) {
            const double* e = g.E + 7 * (int64_t)k;
            double t3 = Ja[0] * e[0];
            for (int r = 1; r < 7; ++r) t3 = t3 + Ja[r] * e[r];
            bi = bi - t3;
        }
    }
    H[(size_t)(fi * D + a) * g.ld + fi * D + b] = hii;
    if (b == 0) bvec[fi * D + a] = bi;
}

// A = H + lambda I on the dim unknowns, the identity on the padding; bs = b (0 on the padding)
__global__ __launch_bounds__(256) void k_eg_damp(const double* __restrict__ H, const double* __restrict__ bvec, double* __restrict__ A,
                                                 double* __restrict__ bs, int dim, int ld, double lambda) {
    const size_t n = (size_t)ld * ld;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int i = (int)(e / ld), j = (int)(e % ld);
        double v = (i < dim && j < dim) ? H[e] : 0.0;
        if (i == j) v = i < dim ? v + lambda : 1.0;
        A[e] = v;
        if (j == 0) bs[i] = i < dim ? bvec[i] : 0.0;
    }
}

// x_k = W_k^T (y_k - sum_{j > k} U_kj x_j), k = nb-1 .. 0, with the factor as k_chol_step leaves it: U_kj(m, c) at
// Uf[(j NB + c) ld + k NB + m], W_k^T(m, q) at Winv[k NB NB + m NB + q].  One workgroup of 1024: wave w sums the columns
// c = w, w + 16, ... of a block row (lane = row m), the 16 partial sums meet in a fixed order.
__global__ __launch_bounds__(1024) void k_eg_back(const double* __restrict__ Uf, const double* __restrict__ Winv, const double* __restrict__ y,
                                                  double* x, int ld, int nb) {
    constexpr int NB = ba::NB;
    __shared__ double part[16][NB], r[NB];
    const int t = threadIdx.x, m = t & 63, w = t >> 6;
    for (int k = nb - 1; k >= 0; --k) {
        double acc = 0;
        for (int c = (k + 1) * NB + w; c < nb * NB; c += 16) acc += Uf[(size_t)c * ld + k * NB + m] * x[c];
        part[w][m] = acc;
        __syncthreads();
        if (t < NB) {
            double s = y[k * NB + m];
            for (int q = 0; q < 16; ++q) s -= part[q][m];
            r[m] = s;
        }
        __syncthreads();
        if (t < NB) {
            const double* Wg = Winv + (size_t)k * NB * NB + (size_t)m * NB;
            double v = 0;
            for (int q = 0; q < NB; ++q) v += Wg[q] * r[q];
            x[k * NB + m] = v;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// oplus on every free vertex: St = Sim3(x_v) * S (update[6] = 0 under fix_scale); fixed vertices, and every vertex when the
// factorisation failed (scal[3] != 0: g2o's solve() returned false), are copied
__global__ __launch_bounds__(64) void k_eg_update(Graph g, const double* __restrict__ x, const double* __restrict__ scal,
                                                  const double* __restrict__ S, double* __restrict__ St) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= g.n_kf) return;
    const int fi = g.slot[v];
    double T[8];
    for (int i = 0; i < 8; ++i) T[i] = S[8 * (int64_t)v + i];
    if (fi >= 0 && scal[3] == 0.0) {
        double u[7], X[8], Sv[8];
        for (int i = 0; i < 7; ++i) u[i] = i < g.D ? x[fi * g.D + i] : 0.0;
        for (int i = 0; i < 8; ++i) Sv[i] = T[i];
        sim3::exp7(u, X);
        sim3::mul(X, Sv, T);
    }
    for (int i = 0; i < 8; ++i) St[8 * (int64_t)v + i] = T[i];
}

// one wave.  scal[0] = sum of the edges' chi2 (edge k on lane k % 64, ascending, then the xor butterfly); with x: scal[1] =
// computeScale() = sum x_j (lambda x_j + b_j), unknown a of free vertex fi on lane (7 fi + a) % 64; with H: scal[2] = max |H_jj|
__global__ __launch_bounds__(64) void k_eg_reduce(Graph g, const double* __restrict__ x, const double* __restrict__ bvec, double lambda,
                                                  const double* __restrict__ H, double* __restrict__ scal) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double c = 0;
    for (int k = lane; k < g.n_edge; k += 64) c = c + g.chi[k];
    c = wave_sum(c);
    if (lane == 0) scal[0] = c;
    if (x) {
        double a = 0;
        for (int j7 = lane; j7 < 7 * g.n_free; j7 += 64) {
            const int fi = j7 / 7, q = j7 % 7;
            if (q >= g.D) continue;
            const int j = fi * g.D + q;
            a = a + x[j] * (lambda * x[j] + bvec[j]);
        }
        a = wave_sum(a);
        if (lane == 0) scal[1] = a;
    }
    if (H) {
        double md = 0;
        for (int j = lane; j < g.D * g.n_free; j += 64) md = fmax(fabs(H[(size_t)j * g.ld + j]), md);
        for (int o = 32; o > 0; o >>= 1) md = fmax(md, __shfl_xor(md, o, 64));
        if (lane == 0) scal[2] = md;
    }
}

// Optimizer.cc:1016-1047: correctedSwr.map(Srw.map(P)), Srw the vertex's INITIAL estimate (vScw)
__global__ __launch_bounds__(256) void k_eg_points(int n_pt, const double* __restrict__ P, const int32_t* __restrict__ ref,
                                                   const double* __restrict__ S_in, const double* __restrict__ S_out, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pt) return;
    const double *Si = S_in + 8 * (int64_t)ref[p], *So = S_out + 8 * (int64_t)ref[p];
    double X[3] = {P[3 * (int64_t)p], P[3 * (int64_t)p + 1], P[3 * (int64_t)p + 2]}, r[3], c[3], Sw[8];
    sim3::rot(Si + 3, X, r);
    for (int i = 0; i < 3; ++i) c[i] = Si[7] * r[i] + Si[i];
    sim3::inv(So, Sw);
    sim3::rot(Sw + 3, c, r);
    for (int i = 0; i < 3; ++i) out[3 * (int64_t)p + i] = Sw[7] * r[i] + Sw[i];
}

// what can be refused without a device: QSP_OK, or the code with the message set
inline int validate(int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge, const int32_t* edge_v0,
                    const int32_t* edge_v1, const double* meas, int32_t fix_scale, int32_t n_iter, int32_t n_pt, const double* pt_in,
                    const int32_t* pt_ref, const double* sim3_out, const double* pt_out, int* n_free_out) {
    if (n_kf < 0 || n_edge < 0 || n_pt < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: negative count");
    // the CSR of incident edges holds (edge << 1 | side) and 2 n_edge offsets in int32
    if (n_edge >= (1 << 30)) return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_essential_graph_optimize: 2^30 edges or more");
    if (n_iter < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: n_iter must not be negative");
    if (!sim3_in || !fixed || !sim3_out) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: null argument");
    if (n_edge && (!edge_v0 || !edge_v1 || !meas)) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: null edge array");
    if (n_pt && (!pt_in || !pt_ref || !pt_out)) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: null point array");
    for (int k = 0; k < n_edge; ++k) {
        if (edge_v0[k] < 0 || edge_v0[k] >= n_kf || edge_v1[k] < 0 || edge_v1[k] >= n_kf)
            return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: edge vertex out of range");
        if (edge_v0[k] == edge_v1[k]) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: an edge joins a vertex to itself");
    }
    for (int p = 0; p < n_pt; ++p)
        if (pt_ref[p] < 0 || pt_ref[p] >= n_kf) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_optimize: pt_ref out of range");
    int n_free = 0;
    for (int v = 0; v < n_kf; ++v) n_free += fixed[v] ? 0 : 1;
    *n_free_out = n_free;
    if (n_edge && (int64_t)(fix_scale ? 6 : 7) * n_free > DIM_MAX)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_essential_graph_optimize: more than 10208 unknowns (dense factorisation); a sparse one is out of scope");
    return QSP_OK;
}

// The device side of one call: the set-up that qsp_essential_graph_optimize and qsp_essential_graph_stages share, and the two
// steps the Levenberg-Marquardt loop is made of.  Device block: [S0 | Z | P | ints] (one upload from one staging buffer)
// [Sa Sb E chi J b bs y x scal Pout Winv H A Uf]; it goes back to the buffer cache when the call ends.
struct Run {
    int device = 0, n_kf = 0, n_edge = 0, n_free = 0, n_pt = 0, D = 7, dim = 0, dimp = 0, nb = 0, chol_lds = 0;
    size_t mat = 0;
    DeviceBlock blk;
    Graph g;
    double *S0 = nullptr, *Sa = nullptr, *Sb = nullptr, *P = nullptr, *Po = nullptr, *H = nullptr, *A = nullptr, *Uf = nullptr, *W = nullptr,
           *bv = nullptr, *bs = nullptr, *y = nullptr, *x = nullptr, *scal = nullptr;
    const int32_t* ref = nullptr;

    // a validated graph with n_edge > 0 and n_free > 0: device, layout, host side of the graph, upload; Sa = S0
    int setup(const char* who, int device_, int32_t n_kf_, const double* sim3_in, const uint8_t* fixed, int n_free_, int32_t n_edge_, const int32_t* edge_v0,
              const int32_t* edge_v1, const double* meas, int32_t fix_scale, int32_t n_pt_, const double* pt_in, const int32_t* pt_ref) {
        QSP_TRY(use_device(device_, who));
        device = device_; n_kf = n_kf_; n_edge = n_edge_; n_free = n_free_; n_pt = n_pt_;
        constexpr int NB = ba::NB;
        D = fix_scale ? 6 : 7; dim = D * n_free; dimp = (dim + NB - 1) / NB * NB; nb = dimp / NB;
        const size_t nk = (size_t)n_kf, ne = (size_t)n_edge, np = (size_t)n_pt;
        mat = (size_t)dimp * dimp;
        const size_t i_v0 = 0, i_v1 = ne, i_slot = 2 * ne, i_free = i_slot + nk, i_off = i_free + (size_t)n_free, i_inc = i_off + nk + 1,
                     i_ref = i_inc + 2 * ne, n_int = i_ref + np;
        StagingLayout L;
        const size_t oS0 = L.take<double>(8 * nk), oZ = L.take<double>(8 * ne), oP = L.take<double>(3 * np), oI = L.take<int32_t>(n_int);
        L.begin_scratch();                                         // (the results come down array by array: S is Sa or Sb)
        const size_t oSa = L.take<double>(8 * nk), oSb = L.take<double>(8 * nk), oE = L.take<double>(7 * ne), oChi = L.take<double>(ne),
                     oJ = L.take<double>(98 * ne), oB = L.take<double>(dimp), oBs = L.take<double>(dimp), oY = L.take<double>(dimp),
                     oX = L.take<double>(dimp), oScal = L.take<double>(8), oPo = L.take<double>(3 * np),
                     oW = L.take<double>((size_t)nb * NB * NB), oH = L.take<double>(mat), oA = L.take<double>(mat), oUf = L.take<double>(mat);
        std::vector<char> hd;
        if (!host_staging(hd, L.up_bytes()))
            return qsp_fail(QSP_ERR_UNSUPPORTED, (std::string(who) + ": out of host memory for a graph of this size").c_str());
        // host side of the graph: free list, slots, CSR of incident edges in insertion order
        int32_t* hi = ptr<int32_t>(hd.data(), oI);
        memcpy(hi + i_v0, edge_v0, sizeof(int32_t) * ne);
        memcpy(hi + i_v1, edge_v1, sizeof(int32_t) * ne);
        for (int v = 0, f = 0; v < n_kf; ++v) {
            hi[i_slot + v] = fixed[v] ? -1 : f;
            if (!fixed[v]) hi[i_free + f++] = v;
        }
        int32_t* off = hi + i_off;                                 // counts at v + 1, starts, then each start walks to its end ...
        for (size_t k = 0; k < ne; ++k) { off[edge_v0[k] + 1]++; off[edge_v1[k] + 1]++; }
        for (size_t v = 0; v < nk; ++v) off[v + 1] += off[v];
        for (size_t k = 0; k < ne; ++k) {
            hi[i_inc + off[edge_v0[k]]++] = (int32_t)(k << 1);
            hi[i_inc + off[edge_v1[k]]++] = (int32_t)(k << 1) | 1;
        }
        for (size_t v = nk; v > 0; --v) off[v] = off[v - 1];       // ... and is moved back: off[v] is the start of v again
        off[0] = 0;
        if (np) memcpy(hi + i_ref, pt_ref, sizeof(int32_t) * np);
        memcpy(&hd[oS0], sim3_in, sizeof(double) * 8 * nk);
        memcpy(&hd[oZ], meas, sizeof(double) * 8 * ne);
        if (np) memcpy(&hd[oP], pt_in, sizeof(double) * 3 * np);
        QSP_TRY(blk.take(device, L.total()));
        QSP_TRY(blk.upload(hd.data(), L.up_bytes()));
        char* d = blk.data();
        const int32_t* di = ptr<int32_t>(d, oI);
        auto dd = [d](size_t o) { return ptr<double>(d, o); };
        QSP_HIP(hipMemcpy(dd(oSa), dd(oS0), sizeof(double) * 8 * nk, hipMemcpyDeviceToDevice));
        chol_lds = (int)(sizeof(double) * ba::CHOL_LDS_DOUBLES);
        {   // the factorisation kernels' LDS size: once per device and process
            static std::mutex mu;
            static bool done[64];
            std::lock_guard<std::mutex> lk(mu);
            if (!done[device & 63]) {
                QSP_HIP(hipFuncSetAttribute((const void*)ba::k_chol_first, hipFuncAttributeMaxDynamicSharedMemorySize, chol_lds));
                QSP_HIP(hipFuncSetAttribute((const void*)ba::k_chol_step, hipFuncAttributeMaxDynamicSharedMemorySize, chol_lds));
                done[device & 63] = true;
            }
        }
        g.n_kf = n_kf; g.n_edge = n_edge; g.n_free = n_free; g.D = D; g.fix_scale = fix_scale ? 1 : 0; g.ld = dimp;
        g.v0 = di + i_v0; g.v1 = di + i_v1; g.slot = di + i_slot; g.free_v = di + i_free; g.inc_off = di + i_off; g.inc = di + i_inc;
        g.Z = dd(oZ); g.E = dd(oE); g.chi = dd(oChi); g.J = dd(oJ);
        S0 = dd(oS0); Sa = dd(oSa); Sb = dd(oSb); P = dd(oP); Po = dd(oPo); H = dd(oH); A = dd(oA); Uf = dd(oUf); W = dd(oW);
        bv = dd(oB); bs = dd(oBs); y = dd(oY); x = dd(oX); scal = dd(oScal);
        ref = di + i_ref;
        return QSP_OK;
    }

    // computeActiveErrors, activeRobustChi2, buildSystem at S: E, chi, J, H, b; h[0] = chi2, h[2] = max |H_jj|
    int linearise(const double* S, double* h) {
        const dim3 ge((n_edge + 63) / 64), gl((n_edge + 1) / 2);
        hipLaunchKernelGGL(k_eg_err, ge, dim3(64), 0, 0, g, S);
        hipLaunchKernelGGL(k_eg_lin, gl, dim3(64), 0, 0, g, S);
        QSP_HIP(hipMemsetAsync(H, 0, sizeof(double) * mat, 0));
        QSP_HIP(hipMemsetAsync(scal, 0, sizeof(double) * 8, 0));
        hipLaunchKernelGGL(k_eg_asm, dim3(n_free), dim3(64), 0, 0, g, H, bv);
        hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(64), 0, 0, g, (const double*)nullptr, (const double*)nullptr, 0.0, (const double*)H, scal);
        QSP_HIP(hipGetLastError());
        QSP_HIP(hipMemcpy(h, scal, sizeof(double) * 4, hipMemcpyDeviceToHost));
        return QSP_OK;
    }

    // one trial: (H + lambda I) x = b, St = exp(x) S, the errors at St (E and chi are overwritten); h[0] = chi2 at St,
    // h[1] = computeScale(), h[3] != 0: the factorisation failed
    int trial(const double* S, double* St, double lambda, double* h) {
        const dim3 ge((n_edge + 63) / 64), gk((n_kf + 63) / 64);
        const dim3 gd((unsigned)std::min<size_t>((mat + 255) / 256, 4096));
        QSP_HIP(hipMemsetAsync(scal, 0, sizeof(double) * 8, 0));
        hipLaunchKernelGGL(k_eg_damp, gd, dim3(256), 0, 0, (const double*)H, (const double*)bv, A, bs, dim, dimp, lambda);
        hipLaunchKernelGGL(ba::k_chol_first, dim3(1), dim3(ba::CHOL_THREADS), (size_t)chol_lds, 0, (const double*)A, W, (const double*)bs, y, dimp,
                           scal);
        for (int k = 0; k + 1 < nb; ++k)
            hipLaunchKernelGGL(ba::k_chol_step, dim3(nb - k - 1, nb - k - 1), dim3(ba::CHOL_THREADS), (size_t)chol_lds, 0, A, Uf, W, bs, y, dimp, k,
                               scal);
        hipLaunchKernelGGL(k_eg_back, dim3(1), dim3(1024), 0, 0, (const double*)Uf, (const double*)W, (const double*)y, x, dimp, nb);
        hipLaunchKernelGGL(k_eg_update, gk, dim3(64), 0, 0, g, (const double*)x, (const double*)scal, S, St);
        hipLaunchKernelGGL(k_eg_err, ge, dim3(64), 0, 0, g, (const double*)St);
        hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(64), 0, 0, g, (const double*)x, (const double*)bv, lambda, (const double*)nullptr, scal);
        QSP_HIP(hipGetLastError());
        QSP_HIP(hipMemcpy(h, scal, sizeof(double) * 4, hipMemcpyDeviceToHost));
        return QSP_OK;
    }
};

}  // namespace eg
}  // namespace qsp

extern "C" int qsp_essential_graph_optimize(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                                            const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale,
                                            int32_t n_iter, double lambda_init, int32_t n_pt, const double* pt_in,
                                            const int32_t* pt_ref, double* sim3_out, double* pt_out, qsp_essential_trace* trace) {
    using namespace qsp;
    using namespace qsp::eg;
    if (n_kf == 0) return QSP_OK;
    int n_free = 0;
    int rc = validate(n_kf, sim3_in, fixed, n_edge, edge_v0, edge_v1, meas, fix_scale, n_iter, n_pt, pt_in, pt_ref, sim3_out, pt_out, &n_free);
    if (rc) return rc;
    qsp_essential_trace tr;
    memset(&tr, 0, sizeof(tr));
    if (n_edge == 0 || n_free == 0) {                          // nothing to optimise: the input comes back as it is
        memmove(sim3_out, sim3_in, sizeof(double) * 8 * (size_t)n_kf);
        if (n_pt) memmove(pt_out, pt_in, sizeof(double) * 3 * (size_t)n_pt);
        if (trace) *trace = tr;
        return QSP_OK;
    }
    const size_t nk = (size_t)n_kf, np = (size_t)n_pt;
    std::vector<char> down_bytes;
    if (!host_staging(down_bytes, sizeof(double) * (8 * nk + 3 * np)))
        return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_essential_graph_optimize: out of host memory for a graph of this size");
    double* down = ptr<double>(down_bytes.data(), 0);
    Run r;
    if ((rc = r.setup("qsp_essential_graph_optimize", device, n_kf, sim3_in, fixed, n_free, n_edge, edge_v0, edge_v1, meas, fix_scale, n_pt, pt_in, pt_ref))) return rc;
    double *S = r.Sa, *St = r.Sb;
    double h[4], lambda = 0, ni = 2;
    int nbad = 0, done = 0;
    for (int it = 0; it < n_iter; ++it) {
        if ((rc = r.linearise(S, h))) return rc;
        double cur = h[0];
        const double ini = cur;
        if (it == 0) {                                         // computeLambdaInit: the user's value when it is positive
            lambda = lambda_init > 0 ? lambda_init : 1e-5 * h[2];
            ni = 2;
            nbad = 0;
        }
        int qmax = 0, accepted = 0;
        double rho = 0;
        do {
            if ((rc = r.trial(S, St, lambda, h))) return rc;
            const bool ok = h[3] == 0.0;
            const double tempChi = ok ? h[0] : DBL_MAX;
            double scale = ok ? h[1] : 0.0;                    // (a failed solve leaves x = 0)
            scale += 1e-3;
            rho = (cur - tempChi) / scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 2 * rho - 1;
                alpha = 1. - alpha * alpha * alpha;
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                cur = tempChi;
                std::swap(S, St);
                accepted = 1;
            } else {
                lambda *= ni;
                ni *= 2;
                accepted = 0;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (done < TRACE_MAX) {
            tr.trace[done][0] = cur;
            tr.trace[done][1] = lambda;
            tr.trace[done][2] = (double)qmax;
            tr.trace[done][3] = (double)accepted;
        }
        ++done;
        if (qmax == 10 || rho == 0) break;
        if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
        if (nbad >= 3) break;
    }
    tr.iters = done;
    if (np) hipLaunchKernelGGL(k_eg_points, dim3((n_pt + 255) / 256), dim3(256), 0, 0, n_pt, (const double*)r.P, r.ref, (const double*)r.S0,
                               (const double*)S, r.Po);
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_HIP(hipMemcpy(down, S, sizeof(double) * 8 * nk, hipMemcpyDeviceToHost));
    if (np) QSP_HIP(hipMemcpy(down + 8 * nk, r.Po, sizeof(double) * 3 * np, hipMemcpyDeviceToHost));
    memcpy(sim3_out, down, sizeof(double) * 8 * nk);
    if (np) memcpy(pt_out, down + 8 * nk, sizeof(double) * 3 * np);
    if (trace) *trace = tr;
    return QSP_OK;
}

// qsp_essential_graph_stages: one Run::linearise and one Run::trial at the input states, every buffer copied down
extern "C" int qsp_essential_graph_stages(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                                          const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale,
                                          double lambda, double* E, double* chi, double* J, double* H, double* b, double* x,
                                          double* sim3_trial, double* info) {
    using namespace qsp;
    using namespace qsp::eg;
    if (!E || !chi || !J || !H || !b || !x || !sim3_trial || !info) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_stages: null output");
    if (!(lambda > 0) || !std::isfinite(lambda)) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_stages: lambda must be positive and finite");
    int n_free = 0;
    int rc = validate(n_kf, sim3_in, fixed, n_edge, edge_v0, edge_v1, meas, fix_scale, 0, 0, nullptr, nullptr, sim3_trial, nullptr, &n_free);
    if (rc) return rc;
    if (n_edge == 0 || n_free == 0) return qsp_fail(QSP_ERR_INVALID, "qsp_essential_graph_stages: no edge or no free vertex, nothing to show");
    const size_t nk = (size_t)n_kf, ne = (size_t)n_edge, dim = (size_t)(fix_scale ? 6 : 7) * n_free;
    const size_t oE = 0, oChi = oE + 7 * ne, oJ = oChi + ne, oH = oJ + 98 * ne, oB = oH + dim * dim, oX = oB + dim, oS = oX + dim, n_down = oS + 8 * nk;
    std::vector<char> down_bytes;
    if (!host_staging(down_bytes, sizeof(double) * n_down))
        return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_essential_graph_stages: out of host memory for a graph of this size");
    double* down = ptr<double>(down_bytes.data(), 0);
    Run r;
    if ((rc = r.setup("qsp_essential_graph_stages", device, n_kf, sim3_in, fixed, n_free, n_edge, edge_v0, edge_v1, meas, fix_scale, 0, nullptr, nullptr))) return rc;
    double hl[4], ht[4];
    if ((rc = r.linearise(r.Sa, hl))) return rc;
    // the trial's k_eg_err overwrites E and chi: what the linearisation wrote comes down first
    QSP_HIP(hipMemcpy(&down[oE], r.g.E, sizeof(double) * 7 * ne, hipMemcpyDeviceToHost));
    QSP_HIP(hipMemcpy(&down[oChi], r.g.chi, sizeof(double) * ne, hipMemcpyDeviceToHost));
    QSP_HIP(hipMemcpy(&down[oJ], r.g.J, sizeof(double) * 98 * ne, hipMemcpyDeviceToHost));
    QSP_HIP(hipMemcpy2D(&down[oH], sizeof(double) * dim, r.H, sizeof(double) * r.dimp, sizeof(double) * dim, dim, hipMemcpyDeviceToHost));
    QSP_HIP(hipMemcpy(&down[oB], r.bv, sizeof(double) * dim, hipMemcpyDeviceToHost));
    if ((rc = r.trial(r.Sa, r.Sb, lambda, ht))) return rc;
    QSP_HIP(hipMemcpy(&down[oX], r.x, sizeof(double) * dim, hipMemcpyDeviceToHost));
    QSP_HIP(hipMemcpy(&down[oS], r.Sb, sizeof(double) * 8 * nk, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < ne; ++k)                            // k_eg_lin writes nothing for a fixed vertex: that side reads as zeros
        for (int s = 0; s < 2; ++s)
            if (fixed[s ? edge_v1[k] : edge_v0[k]]) memset(&down[oJ + (2 * k + s) * 49], 0, sizeof(double) * 49);
    memcpy(E, &down[oE], sizeof(double) * 7 * ne);
    memcpy(chi, &down[oChi], sizeof(double) * ne);
    memcpy(J, &down[oJ], sizeof(double) * 98 * ne);
    memcpy(H, &down[oH], sizeof(double) * dim * dim);
    memcpy(b, &down[oB], sizeof(double) * dim);
    memcpy(x, &down[oX], sizeof(double) * dim);
    memcpy(sim3_trial, &down[oS], sizeof(double) * 8 * nk);
    info[0] = hl[0]; info[1] = hl[2]; info[2] = ht[0]; info[3] = ht[1]; info[4] = ht[3]; info[5] = (double)r.dim; info[6] = (double)r.nb;
    return QSP_OK;
}
