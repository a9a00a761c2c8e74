// se3.hpp -- SE3, quaternion and 3x3 helpers in FP64, shared by the bundle adjustment, the pose optimiser and the Sim3 code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace qsp {
namespace ba {

// ---------------------------------------------------------------------------------------------------------------
// SE3 helpers on (tx ty tz qx qy qz qw), following g2o's SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h)
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void quat_to_R(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                 tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
__host__ __device__ inline void R_to_quat(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}
__host__ __device__ inline void quat_normalize(double* q) {
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
__host__ __device__ inline void quat_mul(const double* a, const double* b, double* c) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    c[0] = aw * bx + ax * bw + ay * bz - az * by;
    c[1] = aw * by + ay * bw + az * bx - ax * bz;
    c[2] = aw * bz + az * bw + ax * by - ay * bx;
    c[3] = aw * bw - ax * bx - ay * by - az * bz;
}
__host__ __device__ inline void quat_rot(const double* q, const double* v, double* o) {
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    const double uvx = 2 * (uy * v[2] - uz * v[1]), uvy = 2 * (uz * v[0] - ux * v[2]), uvz = 2 * (ux * v[1] - uy * v[0]);
    o[0] = v[0] + w * uvx + (uy * uvz - uz * uvy);
    o[1] = v[1] + w * uvy + (uz * uvx - ux * uvz);
    o[2] = v[2] + w * uvz + (ux * uvy - uy * uvx);
}
__host__ __device__ inline void se3_mul(const double* a, const double* b, double* c) {
    double rt[3], q[4];
    quat_rot(a + 3, b, rt);
    quat_mul(a + 3, b + 3, q);
    c[0] = a[0] + rt[0]; c[1] = a[1] + rt[1]; c[2] = a[2] + rt[2];
    quat_normalize(q);
    c[3] = q[0]; c[4] = q[1]; c[5] = q[2]; c[6] = q[3];
}
__host__ __device__ inline void se3_inv(const double* a, double* c) {
    const double q[4] = {-a[3], -a[4], -a[5], a[6]}, mt[3] = {-a[0], -a[1], -a[2]};
    double t[3];
    quat_rot(q, mt, t);
    c[0] = t[0]; c[1] = t[1]; c[2] = t[2]; c[3] = q[0]; c[4] = q[1]; c[5] = q[2]; c[6] = q[3];
}
__host__ __device__ inline void se3_map(const double* a, const double* x, double* o) {
    double r[3];
    quat_rot(a + 3, x, r);
    o[0] = r[0] + a[0]; o[1] = r[1] + a[1]; o[2] = r[2] + a[2];
}
__host__ __device__ inline void skew3(const double* v, double* m) {
    m[0] = 0; m[1] = -v[2]; m[2] = v[1]; m[3] = v[2]; m[4] = 0; m[5] = -v[0]; m[6] = -v[1]; m[7] = v[0]; m[8] = 0;
}
__host__ __device__ inline void mat3mul(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ inline void se3_exp(const double* u, double* pose) {   // se3quat.h:273-305
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double Om[9], Om2[9], R[9], V[9];
    skew3(u, Om);
    mat3mul(Om, Om, Om2);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) { R[i] = I[i] + Om[i] + Om2[i]; V[i] = R[i]; }
    } else {
        const double s = sin(theta), c = cos(theta);
        const double a = s / theta, b = (1 - c) / (theta * theta), g = (theta - s) / pow(theta, 3);
        for (int i = 0; i < 9; ++i) { R[i] = I[i] + a * Om[i] + b * Om2[i]; V[i] = I[i] + b * Om[i] + g * Om2[i]; }
    }
    double q[4];
    R_to_quat(R, q);
    quat_normalize(q);
    for (int i = 0; i < 3; ++i) pose[i] = V[3 * i] * u[3] + V[3 * i + 1] * u[4] + V[3 * i + 2] * u[5];
    pose[3] = q[0]; pose[4] = q[1]; pose[5] = q[2]; pose[6] = q[3];
}
__device__ inline void se3_log(const double* pose, double* out) {   // se3quat.h:228-265
    double R[9];
    quat_to_R(pose + 3, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double om[3], Om[9], Om2[9], Vi[9];
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (d > 0.99999) {
        for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
        skew3(om, Om);
        mat3mul(Om, Om, Om2);
        for (int i = 0; i < 9; ++i) Vi[i] = I[i] - 0.5 * Om[i] + (1. / 12.) * Om2[i];
    } else {
        const double theta = acos(d);
        const double f = theta / (2 * sqrt(1 - d * d));
        for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
        skew3(om, Om);
        mat3mul(Om, Om, Om2);
        const double g = (1 - theta / (2 * tan(theta / 2))) / (theta * theta);
        for (int i = 0; i < 9; ++i) Vi[i] = I[i] - 0.5 * Om[i] + g * Om2[i];
    }
    out[0] = om[0]; out[1] = om[1]; out[2] = om[2];
    for (int i = 0; i < 3; ++i) out[3 + i] = Vi[3 * i] * pose[0] + Vi[3 * i + 1] * pose[1] + Vi[3 * i + 2] * pose[2];
}

}  // namespace ba
}  // namespace qsp
