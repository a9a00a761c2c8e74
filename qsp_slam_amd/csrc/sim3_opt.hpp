// sim3_opt.hpp -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1050-1245) for ALL loop candidates of a key frame in one
// launch.  Compiled in c_abi.cpp.
//
// The reference's caller (LoopClosing::ComputeSim3, src/LoopClosing.cc) walks its candidate key frames one after another and
// builds, solves and tears down one g2o graph each: one free VertexSim3Expmap (7 unknowns: rotation, translation, log scale),
// fixed points, and per match the pair EdgeSim3ProjectXYZ (x1 = cam1(S12 X2)) / EdgeInverseSim3ProjectXYZ (x2 = cam2(S12^-1 X1))
// (Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h), both with Huber(sqrt(th2)) and g2o's NUMERIC Jacobian
// (Thirdparty/g2o/g2o/core/base_binary_edge.hpp: central differences through the vertex's oplus, delta 1e-9).  optimize(5), the
// pairs with a chi2 above th2 leave, optimize(10 or 5) on the rest, final count.  The candidates are independent: here ONE WAVE
// owns one candidate, lane = match (strided), every sum is an xor-butterfly all-reduce so that all 64 lanes hold the same totals
// in the same bits, and every lane then runs the 7x7 solve and the LM control flow redundantly in registers, as
// k_ellipsoid_prior_fit does.  A candidate's arithmetic depends on nothing but its own data and its lanes, so its result has the
// same bits alone, in any batch and at any position.
//
// The difference quotient multiplies the rounding of an error evaluation by 5e8.  Every function below therefore evaluates with
// contraction OFF: plain IEEE multiplies and adds in the order written, which a float64 restatement on any host reproduces
// operation for operation (tests/sim3_oracle.py); what is left between the two is the libm of exp / sin / cos.
//
// The 14 perturbed states of an iteration (and their inverses) are the same for every match: they are computed once and parked
// in LDS.  A match's 4x7 Jacobian is parked in the lane's own LDS column while the loop over the 7 directions runs (that loop
// is not unrolled: 28 error evaluations in flight would spill), and read back with constant indices for J^T W J.
#pragma once
#include <float.h>

#include "se3.hpp"
#include "staging.hpp"
#include "wave.hpp"

namespace qsp {
namespace sim3 {

struct In {
    int n_cand, fix_scale;
    const int32_t* off;                            // [n_cand + 1]
    const double *K1, *K2, *S0;                    // [n_cand][4], [n_cand][4], [n_cand][8] tx ty tz qx qy qz qw s
    const double *P1, *P2, *o1, *o2, *i1, *i2;     // [n_match][3], [3], [2], [2], [1], [1]
    double th2, delta;
};
struct Out {                                       // per candidate
    double S[8];
    double trace[2][10][3];                        // chi2, lambda, trials per (optimize call, iteration)
    int32_t iters[2];
    int32_t n_inliers, pad;
};

// Eigen's quaternion * vector and quaternion * quaternion; q = x y z w, not normalised anywhere (g2o::Sim3 does not either)
__device__ inline void rot(const double* q, const double* v, double* o) {
#pragma clang fp contract(off)
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    o[0] = (v[0] + q[3] * ux) + (q[1] * uz - q[2] * uy);
    o[1] = (v[1] + q[3] * uy) + (q[2] * ux - q[0] * uz);
    o[2] = (v[2] + q[3] * uz) + (q[0] * uy - q[1] * ux);
}
__device__ inline void qmul(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    c[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    c[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    c[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    c[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
// Quaterniond(Matrix3d), Eigen's branches with constant indices (ba::R_to_quat indexes by the largest diagonal entry, which
// would put the matrix into scratch); not normalised
template <int I>
__device__ inline void quat_of_branch(const double* m, double* q) {
#pragma clang fp contract(off)
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(m[4 * I] - m[4 * J] - m[4 * K] + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3 * K + J] - m[3 * J + K]) * t;
    q[J] = (m[3 * J + I] + m[3 * I + J]) * t;
    q[K] = (m[3 * K + I] + m[3 * I + K]) * t;
}
__device__ inline void quat_of(const double* m, double* q) {
#pragma clang fp contract(off)
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else if (m[4] > m[0]) {
        if (m[8] > m[4]) quat_of_branch<2>(m, q); else quat_of_branch<1>(m, q);
    } else {
        if (m[8] > m[0]) quat_of_branch<2>(m, q); else quat_of_branch<0>(m, q);
    }
}
// S = (t[3], q[4], s).  c = a * b, Thirdparty/g2o/g2o/types/sim3.h operator*
__device__ inline void mul(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    double rt[3], q[4];
    rot(a + 3, b, rt);
    qmul(a + 3, b + 3, q);
    for (int i = 0; i < 3; ++i) c[i] = a[7] * rt[i] + a[i];
    for (int i = 0; i < 4; ++i) c[3 + i] = q[i];
    c[7] = a[7] * b[7];
}
__device__ inline void inv(const double* a, double* c) {          // Sim3::inverse
#pragma clang fp contract(off)
    const double qc[4] = {-a[3], -a[4], -a[5], a[6]}, f = -1.0 / a[7];
    const double v[3] = {f * a[0], f * a[1], f * a[2]};
    rot(qc, v, c);
    for (int i = 0; i < 4; ++i) c[3 + i] = qc[i];
    c[7] = 1.0 / a[7];
}
// Sim3(const Vector7d& update): omega (3), upsilon (3), sigma
__device__ inline void exp7(const double* u, double* S) {
#pragma clang fp contract(off)
    const double sigma = u[6];
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double Om[9], Om2[9], R[9];
    ba::skew3(u, Om);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    const double s = exp(sigma), eps = 0.00001;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
            for (int i = 0; i < 9; ++i) R[i] = (I[i] + Om[i]) + Om2[i];
        } else {
            const double theta2 = theta * theta, sn = sin(theta), cs = cos(theta);
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
            const double a = sn / theta, b = (1 - cs) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = (I[i] + a * Om[i]) + b * Om2[i];
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
            for (int i = 0; i < 9; ++i) R[i] = (I[i] + Om[i]) + Om2[i];
        } else {
            const double sn = sin(theta), cs = cos(theta);
            const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = (I[i] + ra * Om[i]) + rb * Om2[i];
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    quat_of(R, S + 3);                                           // Quaterniond(R): no normalisation
    for (int i = 0; i < 3; ++i) {
        const double w0 = (A * Om[3 * i] + B * Om2[3 * i]) + C * I[3 * i], w1 = (A * Om[3 * i + 1] + B * Om2[3 * i + 1]) + C * I[3 * i + 1],
                     w2 = (A * Om[3 * i + 2] + B * Om2[3 * i + 2]) + C * I[3 * i + 2];
        S[i] = (w0 * u[3] + w1 * u[4]) + w2 * u[5];
    }
    S[7] = s;
}
// obs - cam(project(S.map(X))): EdgeSim3ProjectXYZ::computeError with (S12, P2c, K1, obs1), EdgeInverseSim3ProjectXYZ's with
// (S12^-1, P1c, K2, obs2)
__device__ inline void edge_error(const double* S, const double* X, const double* K, const double* obs, double* e) {
#pragma clang fp contract(off)
    double r[3];
    rot(S + 3, X, r);
    const double x = S[7] * r[0] + S[0], y = S[7] * r[1] + S[1], z = S[7] * r[2] + S[2];
    e[0] = obs[0] - ((x / z) * K[0] + K[2]);
    e[1] = obs[1] - ((y / z) * K[1] + K[3]);
}

__device__ inline void huber(double e, double delta, double& rho0, double& rho1) {      // RobustKernelHuber::robustify
#pragma clang fp contract(off)
    const double dsqr = delta * delta;
    if (e <= dsqr) { rho0 = e; rho1 = 1.0; return; }
    const double sq = sqrt(e);
    rho0 = 2 * sq * delta - dsqr;
    rho1 = delta / sq;
}

constexpr int N = 7, NT = N * (N + 1) / 2, NV = NT + N + 1;

__global__ __launch_bounds__(64) void k_sim3_opt(In in, uint8_t* __restrict__ inlier, double* __restrict__ chi, Out* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double pert[N][4][8];        // exp(+d) S, exp(-d) S and their inverses, per direction
    __shared__ double Jl[4 * N][64];        // the lane's match: rows e12.u e12.v e21.u e21.v, column-major by direction
    __shared__ double tot[NV];              // the wave's sums: H, b, robust chi2 (the trials read them from here, not from registers)
    const int w = blockIdx.x, lane = threadIdx.x;
    const int m0 = in.off[w], m1 = in.off[w + 1], n = m1 - m0;
    const double* K1 = in.K1 + 4 * (int64_t)w;
    const double* K2 = in.K2 + 4 * (int64_t)w;
    double S[8];
    for (int i = 0; i < 8; ++i) S[i] = in.S0[8 * (int64_t)w + i];
    Out* O = out + w;
    if (lane == 0) {
        for (int i = 0; i < 8; ++i) O->S[i] = S[i];
        for (int i = 0; i < 60; ++i) (&O->trace[0][0][0])[i] = 0.0;
        O->iters[0] = O->iters[1] = 0;
        O->n_inliers = 0;
        O->pad = 0;
    }
    for (int k = m0 + lane; k < m1; k += 64) inlier[k] = 1;
    if (n == 0) return;

    // computeActiveErrors + activeRobustChi2 at T: every active edge keeps its chi2 (a rejected last trial leaves its values there)
    auto chi2_at = [&](const double* T) {
        double Ti[8];
        inv(T, Ti);
        double a = 0;
        for (int k = m0 + lane; k < m1; k += 64) {
            if (!inlier[k]) continue;
            double e[2], r0, r1;
            edge_error(T, in.P2 + 3 * (int64_t)k, K1, in.o1 + 2 * (int64_t)k, e);
            const double c1 = in.i1[k] * (e[0] * e[0] + e[1] * e[1]);
            edge_error(Ti, in.P1 + 3 * (int64_t)k, K2, in.o2 + 2 * (int64_t)k, e);
            const double c2 = in.i2[k] * (e[0] * e[0] + e[1] * e[1]);
            chi[2 * (int64_t)k] = c1;
            chi[2 * (int64_t)k + 1] = c2;
            huber(c1, in.delta, r0, r1);
            a += r0;
            huber(c2, in.delta, r0, r1);
            a += r0;
        }
        return wave_sum(a);
    };

    int n_more = 5, n_left = n;
    for (int pass = 0; pass < 2; ++pass) {
        const int n_iter = pass == 0 ? 5 : n_more;
        int done = 0, nbad = 0;
        double cur = 0, lambda = 0, ni = 2;
        for (int it = 0; it < n_iter; ++it) {
            // ---- the 14 perturbed estimates: estimate <- Sim3(+-delta e_d) * estimate, update[6] = 0 under fix_scale -------
            __syncthreads();
#pragma unroll 1
            for (int d = 0; d < N; ++d) {
                double u[N] = {0, 0, 0, 0, 0, 0, 0}, E[8], T[8], Ti[8];
                const double step = (in.fix_scale && d == 6) ? 0.0 : 1e-9;
                for (int sgn = 0; sgn < 2; ++sgn) {
                    for (int i = 0; i < N; ++i) u[i] = (i == d) ? (sgn ? -step : step) : 0.0;
                    exp7(u, E);
                    mul(E, S, T);
                    inv(T, Ti);
                    if (lane == 0)
                        for (int i = 0; i < 8; ++i) { pert[d][sgn][i] = T[i]; pert[d][2 + sgn][i] = Ti[i]; }
                }
            }
            __syncthreads();
            // ---- buildSystem: H (upper triangle, 28), b (7), robust chi2 ----------------------------------------------------
            double Si[8];
            inv(S, Si);
            double v[NV];
            for (int i = 0; i < NV; ++i) v[i] = 0;
            for (int k = m0 + lane; k < m1; k += 64) {
                if (!inlier[k]) continue;
                const double *P1 = in.P1 + 3 * (int64_t)k, *P2 = in.P2 + 3 * (int64_t)k, *o1 = in.o1 + 2 * (int64_t)k,
                             *o2 = in.o2 + 2 * (int64_t)k;
                const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll 1
                for (int d = 0; d < N; ++d) {
                    double a[2], b[2];
                    edge_error(pert[d][0], P2, K1, o1, a);
                    edge_error(pert[d][1], P2, K1, o1, b);
                    Jl[d][lane] = scalar * (a[0] - b[0]);
                    Jl[N + d][lane] = scalar * (a[1] - b[1]);
                    edge_error(pert[d][2], P1, K2, o2, a);
                    edge_error(pert[d][3], P1, K2, o2, b);
                    Jl[2 * N + d][lane] = scalar * (a[0] - b[0]);
                    Jl[3 * N + d][lane] = scalar * (a[1] - b[1]);
                }
                double e[4], r0, r1, om[4];
                edge_error(S, P2, K1, o1, e);
                edge_error(Si, P1, K2, o2, e + 2);
                const double c1 = in.i1[k] * (e[0] * e[0] + e[1] * e[1]), c2 = in.i2[k] * (e[2] * e[2] + e[3] * e[3]);
                huber(c1, in.delta, r0, r1);
                v[NT + N] += r0;
                om[0] = om[1] = r1 * in.i1[k];
                huber(c2, in.delta, r0, r1);
                v[NT + N] += r0;
                om[2] = om[3] = r1 * in.i2[k];
                double J[4][N];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int d = 0; d < N; ++d) J[r][d] = Jl[r * N + d][lane];
                int q = 0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[NT + i] -= J[r][i] * om[r] * e[r];
#pragma unroll
                    for (int j = i; j < N; ++j) {
                        double s2 = 0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) s2 += J[r][i] * om[r] * J[r][j];
                        v[q++] += s2;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double t = wave_sum(v[i]);
                if (lane == 0) tot[i] = t;
            }
            __syncthreads();
            cur = tot[NT + N];
            const double ini = cur;
            if (it == 0) {                                               // computeLambdaInit, every optimize() call
                double md = 0;
                int q = 0;
                for (int i = 0; i < N; ++i) { md = fmax(fabs(tot[q]), md); q += N - i; }
                lambda = 1e-5 * md; ni = 2; nbad = 0;
            }
            int qmax = 0;
            double rho = 0;
            do {                                                         // LM trials, as k_pose_opt / k_ellipsoid_prior_fit
                double bk[8], x[N] = {0, 0, 0, 0, 0, 0, 0}, Am[N][N];
                for (int i = 0; i < 8; ++i) bk[i] = S[i];
                int q = 0;
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = i; j < N; ++j) { Am[i][j] = tot[q]; Am[j][i] = tot[q]; ++q; }
#pragma unroll
                for (int i = 0; i < N; ++i) Am[i][i] += lambda;
                bool ok = true;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double dd = Am[j][j];
#pragma unroll
                    for (int q2 = 0; q2 < j; ++q2) dd -= Am[j][q2] * Am[j][q2];
                    if (!(dd > 0) || !isfinite(dd)) ok = false;
                    const double l = sqrt(dd);
                    Am[j][j] = l;
#pragma unroll
                    for (int i = j + 1; i < N; ++i) {
                        double s2 = Am[i][j];
#pragma unroll
                        for (int q2 = 0; q2 < j; ++q2) s2 -= Am[i][q2] * Am[j][q2];
                        Am[i][j] = s2 / l;
                    }
                }
                if (ok) {
                    double y[N];
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        double s2 = tot[NT + i];
#pragma unroll
                        for (int q2 = 0; q2 < i; ++q2) s2 -= Am[i][q2] * y[q2];
                        y[i] = s2 / Am[i][i];
                    }
#pragma unroll
                    for (int i = N - 1; i >= 0; --i) {
                        double s2 = y[i];
#pragma unroll
                        for (int q2 = i + 1; q2 < N; ++q2) s2 -= Am[q2][i] * x[q2];
                        x[i] = s2 / Am[i][i];
                    }
                    double u[N], E[8], T[8];
                    for (int i = 0; i < N; ++i) u[i] = x[i];
                    if (in.fix_scale) u[6] = 0;                          // VertexSim3Expmap::oplusImpl
                    exp7(u, E);
                    mul(E, S, T);
                    for (int i = 0; i < 8; ++i) S[i] = T[i];
                }
                double tempChi = chi2_at(S);
                if (!ok) tempChi = DBL_MAX;
                rho = cur - tempChi;
                double scale = 1e-3;
                for (int i = 0; i < N; ++i) scale += x[i] * (lambda * x[i] + tot[NT + i]);
                rho /= scale;
                if (rho > 0 && isfinite(tempChi)) {
                    double alpha = 2 * rho - 1;
                    alpha = 1. - alpha * alpha * alpha;
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2;
                    cur = tempChi;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    for (int i = 0; i < 8; ++i) S[i] = bk[i];
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            ++done;
            if (lane == 0) {
                O->trace[pass][it][0] = cur;
                O->trace[pass][it][1] = lambda;
                O->trace[pass][it][2] = (double)qmax;
            }
            if (qmax == 10 || rho == 0) break;
            if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
            if (nbad >= 3) break;
        }
        // ---- a pair leaves when either of its chi2 is above th2 (:1189-1207, :1223-1238) -------------------------------------
        double bad = 0;
        for (int k = m0 + lane; k < m1; k += 64) {
            if (!inlier[k]) continue;
            if (chi[2 * (int64_t)k] > in.th2 || chi[2 * (int64_t)k + 1] > in.th2) { inlier[k] = 0; bad += 1.0; }
        }
        const int n_bad = (int)wave_sum(bad);
        if (lane == 0) O->iters[pass] = done;
        if (pass == 0) {
            if (n - n_bad < 10) return;                                  // :1215-1216: 0 inliers, S12 as it came
            n_more = n_bad > 0 ? 10 : 5;
            n_left = n - n_bad;
        } else if (lane == 0) {
            O->n_inliers = n_left - n_bad;
            for (int i = 0; i < 8; ++i) O->S[i] = S[i];
        }
    }
}

}  // namespace sim3
}  // namespace qsp

extern "C" int qsp_sim3_optimize_batch(int device, int32_t n_cand, const int32_t* match_off, const double* K1, const double* K2,
                                       const double* sim3_in, const double* P1c, const double* P2c, const double* obs1,
                                       const double* obs2, const double* info1, const double* info2, double th2, int32_t fix_scale,
                                       double* sim3_out, uint8_t* inlier, int32_t* n_inliers, qsp_sim3_trace* trace) {
    using namespace qsp;
    if (n_cand < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: negative candidate count");
    if (n_cand == 0) return QSP_OK;
    if (!match_off || !K1 || !K2 || !sim3_in || !sim3_out || !n_inliers)
        return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: null argument");
    if (match_off[0] != 0) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: offsets start at 0");
    for (int i = 0; i < n_cand; ++i)
        if (match_off[i + 1] < match_off[i]) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: offsets must not decrease");
    const size_t nm = (size_t)match_off[n_cand], nc = (size_t)n_cand;
    if (nm && (!P1c || !P2c || !obs1 || !obs2 || !info1 || !info2 || !inlier))
        return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: null match array");
    if (!(th2 >= 0)) return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: th2 must not be negative");
    QSP_TRY(use_device(device, "qsp_sim3_optimize_batch"));
    // up      [K1 | K2 | S0 | P1 | P2 | o1 | o2 | i1 | i2 | off]
    // scratch [chi]
    // down    [Out x n_cand | inlier]
    StagingLayout L;
    const size_t aK1 = L.take<double>(4 * nc), aK2 = L.take<double>(4 * nc), aS0 = L.take<double>(8 * nc), aP1 = L.take<double>(3 * nm),
                 aP2 = L.take<double>(3 * nm), ao1 = L.take<double>(2 * nm), ao2 = L.take<double>(2 * nm), ai1 = L.take<double>(nm),
                 ai2 = L.take<double>(nm), a_off = L.take<int32_t>(nc + 1);
    L.begin_scratch();
    const size_t a_chi = L.take<double>(2 * nm);
    L.begin_down();
    const size_t a_out = L.take<sim3::Out>(nc), a_inl = L.take<uint8_t>(nm);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes()))
        return qsp_fail(QSP_ERR_INVALID, "qsp_sim3_optimize_batch: out of host memory for the staging buffers");
    put(up, aK1, K1, 32 * nc); put(up, aK2, K2, 32 * nc); put(up, aS0, sim3_in, 64 * nc); put(up, aP1, P1c, 24 * nm); put(up, aP2, P2c, 24 * nm);
    put(up, ao1, obs1, 16 * nm); put(up, ao2, obs2, 16 * nm); put(up, ai1, info1, 8 * nm); put(up, ai2, info2, 8 * nm);
    put(up, a_off, match_off, 4 * (nc + 1));
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    sim3::In in;
    in.n_cand = n_cand; in.fix_scale = fix_scale ? 1 : 0;
    in.off = ptr<int32_t>(d, a_off);
    in.K1 = ptr<double>(d, aK1); in.K2 = ptr<double>(d, aK2); in.S0 = ptr<double>(d, aS0); in.P1 = ptr<double>(d, aP1);
    in.P2 = ptr<double>(d, aP2); in.o1 = ptr<double>(d, ao1); in.o2 = ptr<double>(d, ao2); in.i1 = ptr<double>(d, ai1);
    in.i2 = ptr<double>(d, ai2);
    in.th2 = th2;
    in.delta = (double)sqrtf((float)th2);                                  // const float deltaHuber = sqrt(th2), :1099
    hipLaunchKernelGGL(sim3::k_sim3_opt, dim3(n_cand), dim3(64), 0, 0, in, ptr<uint8_t>(d, a_inl), ptr<double>(d, a_chi),
                       ptr<sim3::Out>(d, a_out));
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const sim3::Out* O = ptr<sim3::Out>(down.data(), L.in_down(a_out));
    for (size_t c = 0; c < nc; ++c) {
        memcpy(sim3_out + 8 * c, O[c].S, sizeof(double) * 8);
        n_inliers[c] = O[c].n_inliers;
        if (trace) {
            trace[c].iters[0] = O[c].iters[0];
            trace[c].iters[1] = O[c].iters[1];
            memcpy(trace[c].trace, O[c].trace, sizeof(O[c].trace));
        }
    }
    if (nm) memcpy(inlier, down.data() + L.in_down(a_inl), nm);
    return QSP_OK;
}
