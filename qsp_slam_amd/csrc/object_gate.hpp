// object_gate.hpp -- the map-point gate of LocalMapping::ProcessDetectedObjects, batched (include/qsp_hip.h, qsp_object_gates):
// MapObject::RemoveOutliersSimple + ComputeCuboidPCA (reference src/MapObject.cc:275-313, 361-475) or RemoveOutliersModel
// (:316-358) per object.  ONE WORKGROUP of 256 lanes per object, every object of the call in one launch.
//
// Layout.  An object of at most QSP_GATE_LDS_POINTS points is copied to LDS once and every pass reads it there; a larger one is
// read again from global memory in every pass.  The passes are the same code either way (one pointer), so are the results.
//   PCA:   sum -> mean0 | erase + survivor sum -> mean | scatter | lane 0: Jacobi, R, R^-1 | 4 radix-select passes | lane 0: box,
//          pose | flags.      MODEL: vertex min / max | lane 0: M^-1, bounds | flags.
// Sums.  Lane t adds its points t, t + 256, ... in that order in double, the 64 lanes of a wave are folded by shuffles
// (32, 16, ... 1), the four wave sums go through LDS and are added as (w0 + w1) + (w2 + w3): a fixed tree over the point index,
// no floating-point atomics, so an object's bits do not depend on the batch around it.
// Order statistics.  Radix select over the order-preserving integer key of the float32 box coordinate: four 8-bit passes from the
// top byte, all six selections (3 axes x {lo, hi}) in one sweep of the points per pass, one 256-bin integer LDS histogram per
// selection (integer atomics: the counts do not depend on arrival order).  After a pass one lane per selection walks its
// histogram to the bin that holds its rank and extends its prefix.  The key found is the key std::sort would leave at that
// index, ties included.  -0.0 is folded onto +0.0 before the key is taken.
// The keys are taken about the box-frame mean (R^-1 x - R^-1 m): a shift leaves the order, x(hi) - x(lo) and, after adding
// R^-1 m back in double, the centre what they were, and keeps the float32 rounding of a key relative to the object's size
// instead of to its distance from the world origin.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "staging.hpp"

namespace qsp {
namespace gate {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsPoints = QSP_GATE_LDS_POINTS;
constexpr int kSel = 6;   // 3 axes x {lo, hi}

struct GateIn {
    const int32_t* mode;
    const int32_t* pts_off;
    const float* pts;
    const float* T_wo;
    const int32_t* vert_off;
    const float* verts;
};
struct GateOut {   // device buffers, all present and zeroed before the launch
    uint8_t* erased;
    uint8_t* outlier;
    float* whl;
    float* R;
    float* centre_w;
    float* T_wo_pca;
    int32_t* status;
};

struct OpSum {
    static __device__ __forceinline__ double f(double a, double b) { return a + b; }
};
struct OpMin {
    static __device__ __forceinline__ double f(double a, double b) { return b < a ? b : a; }
};

// v[0..K) of every lane -> the block's result in every lane, in the fixed tree of the header comment
template <int K, class Op>
__device__ __forceinline__ void block_reduce(double (&v)[K], double (*red)[8]) {
    static_assert(K <= 8, "red holds 8 values per wave");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x = Op::f(x, __shfl_down(x, o, 64));
        v[k] = x;
    }
    __syncthreads();   // the previous reduction's readers are done with red
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[w][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = Op::f(Op::f(red[0][k], red[1][k]), Op::f(red[2][k], red[3][k]));
}

__host__ __device__ __forceinline__ uint32_t float_key(float f) {   // a < b  <=>  key(a) < key(b); -0.0 and +0.0 share a key
    const uint32_t u = __builtin_bit_cast(uint32_t, f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_float(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__host__ __device__ __forceinline__ void inverse3(const double (&a)[3][3], double det, double (&inv)[3][3]) {   // cofactors
    const double d = 1.0 / det;
    inv[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d;
    inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d;
    inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d;
    inv[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d;
    inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d;
    inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d;
    inv[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d;
    inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d;
    inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d;
}
__host__ __device__ __forceinline__ double det3(const double (&a)[3][3]) {
    return a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}

// one Jacobi rotation that annihilates a[P][Q] of the symmetric a (both triangles kept), accumulated into the columns of v
template <int P, int Q>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    constexpr int O = 3 - P - Q;   // the third index
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double aop = a[O][P], aoq = a[O][Q];
    a[O][P] = a[P][O] = c * aop - s * aoq;
    a[O][Q] = a[Q][O] = s * aop + c * aoq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}
template <int I, int J>
__host__ __device__ __forceinline__ void sort_pair(double (&e)[3], double (&v)[3][3]) {   // eigenvalue I <= eigenvalue J afterwards
    if (e[J] < e[I]) {
        const double t = e[I]; e[I] = e[J]; e[J] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double u = v[k][I]; v[k][I] = v[k][J]; v[k][J] = u; }
    }
}
// eigenvectors of the symmetric a in the columns of v, eigenvalues ascending: cyclic Jacobi, rows (0,1) (0,2) (1,2) per sweep.
// The sweeps end when the off-diagonal entries no longer register against the diagonal in double (or are exactly 0, as for a single
// point); convergence is quadratic, 5 to 8 sweeps in practice, and the bound of 32 only keeps a non-finite matrix from looping.
__host__ __device__ inline void eigen3(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (off == 0.0 || dia + off == dia) break;
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    double e[3] = {a[0][0], a[1][1], a[2][2]};
    sort_pair<0, 1>(e, v);
    sort_pair<1, 2>(e, v);
    sort_pair<0, 1>(e, v);
}

struct GateShared {
    float pts[3 * kLdsPoints];
    uint32_t hist[kSel * 256];
    double red[kWaves][8];
    double m[24];              // PCA: R^-1 (9), R^-1 mean (3), centre (3), 1.2 dim / 2 (3); MODEL: M^-1 (9), t (3), lo (3), hi (3)
    double R[9];
    uint32_t prefix[kSel], rank[kSel];
};

__device__ inline void gate_pca(const GateOut& out, GateShared& S, const float* P, int64_t p0, int n0, int obj) {
    const int tid = threadIdx.x;
    // pass 1: the mean of all points
    double a3[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n0; i += kThreads) {
        a3[0] += (double)P[3 * (int64_t)i];
        a3[1] += (double)P[3 * (int64_t)i + 1];
        a3[2] += (double)P[3 * (int64_t)i + 2];
    }
    block_reduce<3, OpSum>(a3, S.red);
    if (n0 == 0) {
        if (tid == 0) out.status[obj] = QSP_GATE_BAD;
        return;
    }
    const double m0x = a3[0] / n0, m0y = a3[1] / n0, m0z = a3[2] / n0;
    auto is_erased = [&](double x, double y, double z) {
        const double dx = x - m0x, dy = y - m0y, dz = z - m0z;
        return sqrt(dx * dx + dy * dy + dz * dz) > 1.0;
    };
    // pass 2: erase, and the survivors' mean
    double a4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n0; i += kThreads) {
        const double x = P[3 * (int64_t)i], y = P[3 * (int64_t)i + 1], z = P[3 * (int64_t)i + 2];
        if (is_erased(x, y, z)) {
            out.erased[p0 + i] = 1;
        } else {
            a4[0] += x; a4[1] += y; a4[2] += z; a4[3] += 1.0;
        }
    }
    block_reduce<4, OpSum>(a4, S.red);
    const int n = (int)a4[3];
    if (n == 0) {
        if (tid == 0) out.status[obj] = QSP_GATE_BAD;
        return;
    }
    const double mx = a4[0] / n, my = a4[1] / n, mz = a4[2] / n;
    // pass 3: the scatter
    double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n0; i += kThreads) {
        const double x = P[3 * (int64_t)i], y = P[3 * (int64_t)i + 1], z = P[3 * (int64_t)i + 2];
        if (is_erased(x, y, z)) continue;
        const double dx = x - mx, dy = y - my, dz = z - mz;
        c6[0] += dx * dx; c6[1] += dx * dy; c6[2] += dx * dz; c6[3] += dy * dy; c6[4] += dy * dz; c6[5] += dz * dz;
    }
    block_reduce<6, OpSum>(c6, S.red);
    const int lo = (int)(0.05 * n), hi = (int)(0.95 * n);
    if (tid == 0) {
        double A[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}}, V[3][3];
        eigen3(A, V);
        int big = 0;   // the sign convention of v2: its largest-magnitude component is positive
        if (fabs(V[1][2]) > fabs(V[big][2])) big = 1;
        if (fabs(V[2][2]) > fabs(V[big][2])) big = 2;
        const double s2 = (big == 0 ? V[0][2] : big == 1 ? V[1][2] : V[2][2]) < 0.0 ? -1.0 : 1.0;
        double R[3][3], Ri[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { R[k][0] = V[k][1]; R[k][1] = V[k][0]; R[k][2] = -s2 * V[k][2]; }
        if (det3(R) < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) R[k][0] = -R[k][0];
        }
        if (R[1][1] > 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { R[k][0] = -R[k][0]; R[k][1] = -R[k][1]; }
        }
        inverse3(R, det3(R), Ri);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { S.R[3 * i + j] = R[i][j]; S.m[3 * i + j] = Ri[i][j]; }
            S.m[9 + i] = Ri[i][0] * mx + Ri[i][1] * my + Ri[i][2] * mz;
        }
    }
    if (tid < kSel) { S.prefix[tid] = 0u; S.rank[tid] = (uint32_t)((tid & 1) ? hi : lo); }
    for (int j = tid; j < kSel * 256; j += kThreads) S.hist[j] = 0u;
    __syncthreads();
    double Ri[9], cm[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) Ri[j] = S.m[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) cm[j] = S.m[9 + j];
    // passes 4-7: radix select, top byte first
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t himask = pass ? (0xFFFFFFFFu << (shift + 8)) : 0u;
        uint32_t pre[kSel];
#pragma unroll
        for (int s = 0; s < kSel; ++s) pre[s] = S.prefix[s];
        for (int i = tid; i < n0; i += kThreads) {
            const double x = P[3 * (int64_t)i], y = P[3 * (int64_t)i + 1], z = P[3 * (int64_t)i + 2];
            if (is_erased(x, y, z)) continue;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const uint32_t key = float_key((float)(Ri[3 * ax] * x + Ri[3 * ax + 1] * y + Ri[3 * ax + 2] * z - cm[ax]));
                const uint32_t bin = (key >> shift) & 255u;
                if ((key & himask) == pre[2 * ax]) atomicAdd(&S.hist[(2 * ax) * 256 + bin], 1u);
                if ((key & himask) == pre[2 * ax + 1]) atomicAdd(&S.hist[(2 * ax + 1) * 256 + bin], 1u);
            }
        }
        __syncthreads();
        if (tid < kSel) {
            const uint32_t r = S.rank[tid];
            uint32_t c = 0u;
            int b = 0;
            for (; b < 255; ++b) {
                const uint32_t h = S.hist[tid * 256 + b];
                if (r < c + h) break;
                c += h;
            }
            S.prefix[tid] |= (uint32_t)b << shift;
            S.rank[tid] = r - c;
        }
        __syncthreads();
        for (int j = tid; j < kSel * 256; j += kThreads) S.hist[j] = 0u;
        __syncthreads();
    }
    if (tid == 0) {
        double dim[3], cen[3], cw[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double xl = (double)key_float(S.prefix[2 * ax]), xh = (double)key_float(S.prefix[2 * ax + 1]);
            dim[ax] = xh - xl;
            cen[ax] = (xh + xl) / 2.0 + cm[ax];
            S.m[12 + ax] = cen[ax];
            S.m[15 + ax] = 1.2 * dim[ax] / 2.0;
            out.whl[3 * obj + ax] = (float)dim[ax];
        }
        float* T = out.T_wo_pca + 16 * (int64_t)obj;
        const double k = 0.40 * dim[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cw[i] = S.R[3 * i] * cen[0] + S.R[3 * i + 1] * cen[1] + S.R[3 * i + 2] * cen[2];
            out.centre_w[3 * obj + i] = (float)cw[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                out.R[9 * (int64_t)obj + 3 * i + j] = (float)S.R[3 * i + j];
                T[4 * i + j] = (float)(k * S.R[3 * i + j]);
            }
            T[4 * i + 3] = (float)cw[i];
        }
        T[15] = 1.0f;   // T[12..14] are 0 already
        out.status[obj] = QSP_GATE_OK;
    }
    __syncthreads();
    // pass 8: the box's outliers among the survivors
    double cen[3], half[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { cen[j] = S.m[12 + j]; half[j] = S.m[15 + j]; }
    for (int i = tid; i < n0; i += kThreads) {
        const double x = P[3 * (int64_t)i], y = P[3 * (int64_t)i + 1], z = P[3 * (int64_t)i + 2];
        if (is_erased(x, y, z)) continue;
        bool o = false;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) o = o || fabs(Ri[3 * ax] * x + Ri[3 * ax + 1] * y + Ri[3 * ax + 2] * z - cen[ax]) > half[ax];
        if (o) out.outlier[p0 + i] = 1;
    }
}

__device__ inline void gate_model(const GateIn& in, const GateOut& out, GateShared& S, const float* P, int64_t p0, int n0, int obj) {
    const int tid = threadIdx.x;
    const int64_t v0 = in.vert_off[obj];
    const int nv = in.vert_off[obj + 1] - in.vert_off[obj];
    if (nv <= 10) {
        if (tid == 0) out.status[obj] = QSP_GATE_SKIPPED;
        return;
    }
    const float* V = in.verts + 3 * v0;
    const double inf = (double)INFINITY;
    double mm[6] = {inf, inf, inf, inf, inf, inf};   // min x y z, then min of the negated coordinates (= -max)
    for (int i = tid; i < nv; i += kThreads) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double c = (double)V[3 * (int64_t)i + ax];
            mm[ax] = OpMin::f(mm[ax], c);
            mm[3 + ax] = OpMin::f(mm[3 + ax], -c);
        }
    }
    block_reduce<6, OpMin>(mm, S.red);
    if (tid == 0) {
        const float* T = in.T_wo + 16 * (int64_t)obj;
        double M[3][3], Mi[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) M[i][j] = (double)T[4 * i + j];
            S.m[9 + i] = (double)T[4 * i + 3];
        }
        const double det = det3(M), scale = cbrt(det);
        inverse3(M, det, Mi);
        const double fac[3] = {1.2, 1.5, 1.2};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) S.m[3 * i + j] = Mi[i][j];
            S.m[12 + i] = fac[i] * mm[i];
            S.m[15 + i] = fac[i] * -mm[3 + i];
            out.whl[3 * obj + i] = (float)((-mm[3 + i] - mm[i]) * scale);
        }
        out.status[obj] = QSP_GATE_OK;
    }
    __syncthreads();
    double Mi[9], t[3], lo[3], hi[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) Mi[j] = S.m[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) { t[j] = S.m[9 + j]; lo[j] = S.m[12 + j]; hi[j] = S.m[15 + j]; }
    for (int i = tid; i < n0; i += kThreads) {
        const double x = (double)P[3 * (int64_t)i] - t[0], y = (double)P[3 * (int64_t)i + 1] - t[1], z = (double)P[3 * (int64_t)i + 2] - t[2];
        bool o = false;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double c = Mi[3 * ax] * x + Mi[3 * ax + 1] * y + Mi[3 * ax + 2] * z;
            o = o || c > hi[ax] || c < lo[ax];
        }
        if (o) out.outlier[p0 + i] = 1;
    }
}

__global__ void __launch_bounds__(kThreads) k_object_gate(GateIn in, GateOut out) {
    __shared__ GateShared S;
    const int obj = blockIdx.x, tid = threadIdx.x;
    const int64_t p0 = in.pts_off[obj];
    const int n0 = in.pts_off[obj + 1] - in.pts_off[obj];
    const float* P = in.pts + 3 * p0;
    if (n0 <= kLdsPoints) {
        for (int j = tid; j < 3 * n0; j += kThreads) S.pts[j] = P[j];
        P = S.pts;
    }
    __syncthreads();
    if (in.mode[obj] == QSP_GATE_MODEL) gate_model(in, out, S, P, p0, n0, obj);
    else gate_pca(out, S, P, p0, n0, obj);
}

}  // namespace gate

}  // namespace qsp

extern "C" int qsp_object_gates(int device, const qsp_object_gate_in* in, qsp_object_gate_out* out) {
    using namespace qsp;
    if (!in || !out) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: null argument");
    const int32_t n = in->n_obj;
    if (n < 0) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: negative object count");
    if (n == 0) return QSP_OK;
    if (!in->mode || !in->pts_off) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: mode / pts_off missing");
    if (in->pts_off[0] != 0) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: offsets start at 0");
    bool any_model = false;
    for (int i = 0; i < n; ++i) {
        if (in->pts_off[i + 1] < in->pts_off[i]) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: offsets must not decrease");
        if (in->mode[i] != QSP_GATE_PCA && in->mode[i] != QSP_GATE_MODEL) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: mode outside {0, 1}");
        any_model = any_model || in->mode[i] == QSP_GATE_MODEL;
    }
    if (any_model && (!in->T_wo || !in->vert_off || !in->verts))
        return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: a MODEL object needs T_wo, vert_off and verts");
    if (in->vert_off) {
        if (in->vert_off[0] != 0) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: vertex offsets start at 0");
        for (int i = 0; i < n; ++i)
            if (in->vert_off[i + 1] < in->vert_off[i]) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: vertex offsets must not decrease");
    }
    const size_t np = (size_t)in->pts_off[n], nv = (any_model && in->vert_off) ? (size_t)in->vert_off[n] : 0;
    if (np && !in->pts_world) return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: pts_world missing");
    for (int i = 0; i < n; ++i)
        if (in->pts_off[i + 1] - in->pts_off[i] > QSP_GATE_MAX_POINTS)
            return qsp_fail(QSP_ERR_UNSUPPORTED, "qsp_object_gates: more than 2^20 points in one object");
    QSP_TRY(use_device(device, "qsp_object_gates"));
    // up   [mode | pts_off | pts | T_wo | vert_off | verts]      (the last three are empty without a MODEL object)
    // down [erased | outlier | whl | R | centre_w | T_wo_pca | status], zeroed before the launch
    const size_t no = (size_t)n, nm = any_model ? no : 0;
    StagingLayout L;
    const size_t a_mode = L.take<int32_t>(no), a_poff = L.take<int32_t>(no + 1), a_pts = L.take<float>(3 * np), a_Two = L.take<float>(16 * nm),
                 a_voff = L.take<int32_t>(nm ? nm + 1 : 0), a_verts = L.take<float>(3 * nv);
    L.begin_down();
    const size_t a_erased = L.take<uint8_t>(np), a_outlier = L.take<uint8_t>(np), a_whl = L.take<float>(3 * no), a_R = L.take<float>(9 * no),
                 a_centre = L.take<float>(3 * no), a_Tpca = L.take<float>(16 * no), a_status = L.take<int32_t>(no);
    std::vector<char> up, down;
    if (!host_staging(up, L.up_bytes()) || !host_staging(down, L.down_bytes()))
        return qsp_fail(QSP_ERR_INVALID, "qsp_object_gates: out of host memory for the staging buffers");
    put(up, a_mode, in->mode, 4 * no); put(up, a_poff, in->pts_off, 4 * (no + 1)); put(up, a_pts, in->pts_world, 12 * np);
    if (any_model) { put(up, a_Two, in->T_wo, 64 * no); put(up, a_voff, in->vert_off, 4 * (no + 1)); put(up, a_verts, in->verts, 12 * nv); }
    DeviceBlock blk;
    QSP_TRY(blk.take(device, L.total()));
    QSP_TRY(blk.upload(up.data(), L.up_bytes()));
    char* d = blk.data();
    gate::GateIn gi{ptr<int32_t>(d, a_mode), ptr<int32_t>(d, a_poff), ptr<float>(d, a_pts), nullptr, nullptr, nullptr};
    if (any_model) { gi.T_wo = ptr<float>(d, a_Two); gi.vert_off = ptr<int32_t>(d, a_voff); gi.verts = ptr<float>(d, a_verts); }
    gate::GateOut go{ptr<uint8_t>(d, a_erased), ptr<uint8_t>(d, a_outlier), ptr<float>(d, a_whl), ptr<float>(d, a_R),
                     ptr<float>(d, a_centre), ptr<float>(d, a_Tpca), ptr<int32_t>(d, a_status)};
    QSP_HIP(hipMemsetAsync(d + L.down_begin(), 0, L.down_bytes(), 0));
    hipLaunchKernelGGL(gate::k_object_gate, dim3(n), dim3(gate::kThreads), 0, 0, gi, go);
    QSP_HIP(hipGetLastError());
    // outputs are written only once everything has succeeded
    QSP_TRY(blk.download(down.data(), L.down_begin(), L.down_bytes()));
    const char* h = down.data();
    if (out->erased && np) std::memcpy(out->erased, h + L.in_down(a_erased), np);
    if (out->outlier && np) std::memcpy(out->outlier, h + L.in_down(a_outlier), np);
    if (out->whl) std::memcpy(out->whl, h + L.in_down(a_whl), sizeof(float) * 3 * no);
    if (out->R) std::memcpy(out->R, h + L.in_down(a_R), sizeof(float) * 9 * no);
    if (out->centre_w) std::memcpy(out->centre_w, h + L.in_down(a_centre), sizeof(float) * 3 * no);
    if (out->T_wo_pca) std::memcpy(out->T_wo_pca, h + L.in_down(a_Tpca), sizeof(float) * 16 * no);
    if (out->status) std::memcpy(out->status, h + L.in_down(a_status), sizeof(int32_t) * no);
    return QSP_OK;
}
