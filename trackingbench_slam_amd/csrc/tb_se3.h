/* FP64 SE(3) helpers shared by the pose-optimisation and local-BA kernels: the g2o SE3Quat /
 * Eigen quaternion operations that VertexSE3Expmap and EdgeSE3ProjectXYZ(OnlyPose) use, restated for
 * the device (see k_pose.hip for the reference call sites). */
#ifndef TB_SE3_H
#define TB_SE3_H
#include "tb_device.h"

struct PoSE3 { double qx, qy, qz, qw, tx, ty, tz; };

__device__ inline void po_quat_from_R(const double* R, PoSE3& s) {
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        s.qw = 0.5 * t;
        t = 0.5 / t;
        s.qx = (R[7] - R[5]) * t;
        s.qy = (R[2] - R[6]) * t;
        s.qz = (R[3] - R[1]) * t;
    } else if (R[0] >= R[4] && R[0] >= R[8]) { /* Eigen picks the largest diagonal entry: i = 0 */
        t = sqrt(R[0] - R[4] - R[8] + 1.0);
        s.qx = 0.5 * t;
        t = 0.5 / t;
        s.qw = (R[7] - R[5]) * t;
        s.qy = (R[3] + R[1]) * t;
        s.qz = (R[6] + R[2]) * t;
    } else if (R[4] > R[0] && R[4] >= R[8]) { /* i = 1 */
        t = sqrt(R[4] - R[8] - R[0] + 1.0);
        s.qy = 0.5 * t;
        t = 0.5 / t;
        s.qw = (R[2] - R[6]) * t;
        s.qz = (R[7] + R[5]) * t;
        s.qx = (R[1] + R[3]) * t;
    } else { /* i = 2 */
        t = sqrt(R[8] - R[0] - R[4] + 1.0);
        s.qz = 0.5 * t;
        t = 0.5 / t;
        s.qw = (R[3] - R[1]) * t;
        s.qx = (R[2] + R[6]) * t;
        s.qy = (R[5] + R[7]) * t;
    }
}
__device__ inline void po_normalize(PoSE3& s) {
    if (s.qw < 0) { s.qx = -s.qx; s.qy = -s.qy; s.qz = -s.qz; s.qw = -s.qw; }
    const double n = sqrt(s.qx * s.qx + s.qy * s.qy + s.qz * s.qz + s.qw * s.qw);
    s.qx /= n; s.qy /= n; s.qz /= n; s.qw /= n;
}
__device__ inline void po_rot(const PoSE3& s, const double* v, double* o) {
    double uv0 = s.qy * v[2] - s.qz * v[1], uv1 = s.qz * v[0] - s.qx * v[2], uv2 = s.qx * v[1] - s.qy * v[0];
    uv0 += uv0; uv1 += uv1; uv2 += uv2;
    const double c0 = s.qy * uv2 - s.qz * uv1, c1 = s.qz * uv0 - s.qx * uv2, c2 = s.qx * uv1 - s.qy * uv0;
    o[0] = v[0] + s.qw * uv0 + c0;
    o[1] = v[1] + s.qw * uv1 + c1;
    o[2] = v[2] + s.qw * uv2 + c2;
}
__device__ inline void po_map(const PoSE3& s, const double* X, double* o) {
    po_rot(s, X, o);
    o[0] += s.tx; o[1] += s.ty; o[2] += s.tz;
}
__device__ inline void po_to_R(const PoSE3& s, double* R) {
    const double tx = 2 * s.qx, ty = 2 * s.qy, tz = 2 * s.qz;
    const double twx = tx * s.qw, twy = ty * s.qw, twz = tz * s.qw;
    const double txx = tx * s.qx, txy = ty * s.qx, txz = tz * s.qx;
    const double tyy = ty * s.qy, tyz = tz * s.qy, tzz = tz * s.qz;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
__device__ inline PoSE3 po_from_Rt(const double* R, const double* t) {
    PoSE3 s;
    po_quat_from_R(R, s);
    po_normalize(s);
    s.tx = t[0]; s.ty = t[1]; s.tz = t[2];
    return s;
}
/* SE3Quat::exp(update) * T */
__device__ inline PoSE3 po_exp_mul(const double* u, const PoSE3& T) {
    const double om[3] = {u[0], u[1], u[2]};
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double Om2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
    double a, b, c, d;
    if (theta < 0.00001) { a = 1.0; b = 0.5; c = 0.5; d = 1.0 / 6.0; }
    else {
        a = sin(theta) / theta;
        b = (1 - cos(theta)) / (theta * theta);
        c = b;
        d = (theta - sin(theta)) / (theta * theta * theta);
    }
    double R[9], V[9], t[3];
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = I + a * Om[i] + b * Om2[i];
        V[i] = I + c * Om[i] + d * Om2[i];
    }
    for (int i = 0; i < 3; i++) t[i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
    const PoSE3 E = po_from_Rt(R, t);
    PoSE3 r;
    r.qw = E.qw * T.qw - E.qx * T.qx - E.qy * T.qy - E.qz * T.qz;
    r.qx = E.qw * T.qx + E.qx * T.qw + E.qy * T.qz - E.qz * T.qy;
    r.qy = E.qw * T.qy + E.qy * T.qw + E.qz * T.qx - E.qx * T.qz;
    r.qz = E.qw * T.qz + E.qz * T.qw + E.qx * T.qy - E.qy * T.qx;
    const double tt[3] = {T.tx, T.ty, T.tz};
    double rt[3];
    po_rot(E, tt, rt);
    r.tx = E.tx + rt[0]; r.ty = E.ty + rt[1]; r.tz = E.tz + rt[2];
    po_normalize(r);
    return r;
}
/* A * B, normalised like po_exp_mul's product */
__device__ inline PoSE3 po_mul(const PoSE3& A, const PoSE3& B) {
    PoSE3 r;
    r.qw = A.qw * B.qw - A.qx * B.qx - A.qy * B.qy - A.qz * B.qz;
    r.qx = A.qw * B.qx + A.qx * B.qw + A.qy * B.qz - A.qz * B.qy;
    r.qy = A.qw * B.qy + A.qy * B.qw + A.qz * B.qx - A.qx * B.qz;
    r.qz = A.qw * B.qz + A.qz * B.qw + A.qx * B.qy - A.qy * B.qx;
    const double bt[3] = {B.tx, B.ty, B.tz};
    double rt[3];
    po_rot(A, bt, rt);
    r.tx = A.tx + rt[0]; r.ty = A.ty + rt[1]; r.tz = A.tz + rt[2];
    po_normalize(r);
    return r;
}
__device__ inline PoSE3 po_inverse(const PoSE3& T) {
    PoSE3 r;
    r.qx = -T.qx; r.qy = -T.qy; r.qz = -T.qz; r.qw = T.qw;
    const double t[3] = {T.tx, T.ty, T.tz};
    double rt[3];
    po_rot(r, t, rt);
    r.tx = -rt[0]; r.ty = -rt[1]; r.tz = -rt[2];
    return r;
}
/* Below PO_SMALL_ANGLE the coefficients of Log and of the inverse left Jacobian that cancel take three terms of their series
 * (error below 2e-11 relative at the switch); tests/pose_graph_reference.py switches at the same angle. */
#define PO_SMALL_ANGLE 0.1
/* k of V^-1 = Jl^-1 of SO(3) = I - Omega / 2 + k Omega^2 */
__device__ inline double po_so3_inv_coeff(double theta) {
    if (theta < PO_SMALL_ANGLE) {
        const double t2 = theta * theta;
        return 1.0 / 12 + t2 / 720 + t2 * t2 / 30240;
    }
    const double h = 0.5 * theta;
    return (1.0 - h * cos(h) / sin(h)) / (theta * theta);
}
/* o = (I - Omega / 2 + k Omega^2) v, Omega = [om]x */
__device__ inline void po_so3_inv_apply(const double* om, double k, const double* v, double* o) {
    const double c[3] = {om[1] * v[2] - om[2] * v[1], om[2] * v[0] - om[0] * v[2], om[0] * v[1] - om[1] * v[0]};
    const double cc[3] = {om[1] * c[2] - om[2] * c[1], om[2] * c[0] - om[0] * c[2], om[0] * c[1] - om[1] * c[0]};
    for (int i = 0; i < 3; i++) o[i] = v[i] - 0.5 * c[i] + k * cc[i];
}
/* r = (omega, upsilon) with SE3Quat::exp(r) = T, the angle in [0, pi]; T normalised (qw >= 0) */
__device__ inline void po_log(const PoSE3& T, double* r) {
    const double n = sqrt(T.qx * T.qx + T.qy * T.qy + T.qz * T.qz);
    const double theta = 2.0 * atan2(n, T.qw);
    const double s = theta < 0.00001 ? 2.0 / T.qw : theta / n;
    r[0] = T.qx * s; r[1] = T.qy * s; r[2] = T.qz * s;
    const double t[3] = {T.tx, T.ty, T.tz};
    po_so3_inv_apply(r, po_so3_inv_coeff(theta), t, r + 3);
}
/* Ad(T) = [[R, 0], [[t]x R, R]] for the (omega, upsilon) ordering, row-major 6x6 */
__device__ inline void po_adjoint(const PoSE3& T, double* A) {
    double R[9];
    po_to_R(T, R);
    const double tx[9] = {0, -T.tz, T.ty, T.tz, 0, -T.tx, -T.ty, T.tx, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            A[i * 6 + j] = R[i * 3 + j];
            A[i * 6 + 3 + j] = 0.0;
            A[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
            A[(3 + i) * 6 + j] = tx[i * 3] * R[j] + tx[i * 3 + 1] * R[3 + j] + tx[i * 3 + 2] * R[6 + j];
        }
}
__device__ inline void po_mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
/* inverse left Jacobian of SE(3) at r = (omega, upsilon), row-major 6x6: [[Ji, 0], [-Ji Q Ji, Ji]], Ji = Jl^-1 of SO(3) and
 * Q = Up / 2 + c1 (Om Up + Up Om + Om Up Om) + c2 (Om Om Up + Up Om Om - 3 Om Up Om) + c3 (Om Up Om Om + Om Om Up Om) */
__device__ inline void po_jl_inv(const double* r, double* J) {
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    double c1, c2, c3;
    if (theta < PO_SMALL_ANGLE) {
        const double t2 = theta * theta;
        c1 = 1.0 / 6 - t2 / 120 + t2 * t2 / 5040;
        c2 = 1.0 / 24 - t2 / 720 + t2 * t2 / 40320;
        c3 = 1.0 / 120 - t2 / 2520 + t2 * t2 / 120960;
    } else {
        const double s = sin(theta), c = cos(theta), t2 = theta * theta;
        c1 = (theta - s) / (t2 * theta);
        c2 = (t2 + 2 * c - 2) / (2 * t2 * t2);
        c3 = (2 * theta - 3 * s + theta * c) / (2 * t2 * t2 * theta);
    }
    const double Om[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    const double Up[9] = {0, -r[5], r[4], r[5], 0, -r[3], -r[4], r[3], 0};
    double OU[9], UO[9], OUO[9], OOU[9], UOO[9], OUOO[9], OOUO[9], Om2[9], Ji[9], Q[9], T1[9], T2[9];
    po_mul3(Om, Up, OU);
    po_mul3(Up, Om, UO);
    po_mul3(OU, Om, OUO);
    po_mul3(Om, OU, OOU);
    po_mul3(UO, Om, UOO);
    po_mul3(OUO, Om, OUOO);
    po_mul3(Om, OUO, OOUO);
    po_mul3(Om, Om, Om2);
    const double k = po_so3_inv_coeff(theta);
    for (int i = 0; i < 9; i++) {
        Q[i] = 0.5 * Up[i] + c1 * (OU[i] + UO[i] + OUO[i]) + c2 * (OOU[i] + UOO[i] - 3 * OUO[i]) + c3 * (OUOO[i] + OOUO[i]);
        Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[i] + k * Om2[i];
    }
    po_mul3(Ji, Q, T1);
    po_mul3(T1, Ji, T2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            J[i * 6 + j] = Ji[i * 3 + j];
            J[i * 6 + 3 + j] = 0.0;
            J[(3 + i) * 6 + j] = -T2[i * 3 + j];
            J[(3 + i) * 6 + 3 + j] = Ji[i * 3 + j];
        }
}
/* un-pivoted Cholesky solve of the 6x6 system; false if not positive definite */
__device__ inline bool po_chol6(const double* H, double lambda, const double* b, double* x) {
    double A[36];
    for (int i = 0; i < 36; i++) A[i] = H[i];
    for (int i = 0; i < 6; i++) A[i * 6 + i] += lambda;
    for (int j = 0; j < 6; j++) {
        double d = A[j * 6 + j];
        for (int k = 0; k < j; k++) d -= A[j * 6 + k] * A[j * 6 + k];
        if (!(d > 0) || !isfinite(d)) return false;
        d = sqrt(d);
        A[j * 6 + j] = d;
        for (int i = j + 1; i < 6; i++) {
            double s = A[i * 6 + j];
            for (int k = 0; k < j; k++) s -= A[i * 6 + k] * A[j * 6 + k];
            A[i * 6 + j] = s / d;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s -= A[i * 6 + k] * y[k];
        y[i] = s / A[i * 6 + i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++) s -= A[k * 6 + i] * x[k];
        x[i] = s / A[i * 6 + i];
    }
    return true;
}

__device__ __forceinline__ double po_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
/* block sum of NV per-thread values; result valid in every thread; red: LDS >= 4*NV doubles */
template <int NV>
__device__ __forceinline__ void po_block_sum(double (&v)[NV], double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = po_wave_sum(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = (red[i] + red[NV + i]) + (red[2 * NV + i] + red[3 * NV + i]);
}

#endif
