/* FP64 Sim(3) helpers of the Sim(3) pose graph (k_pgo_sim3.hip), beside tb_se3.h whose quaternion operations they use: an element
 * S = (s, R, t) acts as X' = s R X + t, the tangent vector is (omega, upsilon, sigma) -- the solvers' (omega, upsilon) with the
 * log-scale appended, as g2o's Sim3 has it. tests/pose_graph_sim3_reference.py states the same in numpy and derives the series'
 * lengths; the constants below are its SMALL, SMALL_S, N_THETA, N_SIGMA and JL_ORDER. */
#ifndef TB_SIM3_H
#define TB_SIM3_H
#include "tb_se3.h"

struct PoSim3 { PoSE3 T; double s; };   /* T: the unit quaternion of R (qw >= 0) and t */

#define S3_SMALL 0.1     /* rotation angle below which W's coefficients take their series in theta */
#define S3_SMALL_S 0.1   /* |sigma| below which g_k takes its series in sigma */
#define S3_N_SIGMA 8     /* terms of that series (truncation 3e-13 relative at the switch) */
#define S3_JL_ORDER 22   /* highest power of ad(r) in Jl^-1: the Jacobians within 1e-9 for |omega| <= 2, |upsilon| <= 5, |sigma| <= 1 */

/* g_k(sigma) = int_0^1 tau^k e^(sigma tau) dtau, k = 0 .. kmax (kmax <= 8) */
__device__ inline void s3_g(double sigma, int kmax, double* g) {
    if (fabs(sigma) < S3_SMALL_S) {
        for (int k = 0; k <= kmax; k++) {
            double term = 1.0, acc = 0.0;
            for (int m = 0; m < S3_N_SIGMA; m++) {
                acc += term / (double)(m + k + 1);
                term *= sigma / (double)(m + 1);
            }
            g[k] = acc;
        }
    } else {
        const double es = exp(sigma);
        g[0] = (es - 1.0) / sigma;
        for (int k = 1; k <= kmax; k++) g[k] = (es - k * g[k - 1]) / sigma;
    }
}

/* W = C I + A Omega + B Omega^2 = int_0^1 e^(sigma tau) exp(tau Omega) dtau, row-major 3x3 */
__device__ inline void s3_W(const double* om, double sigma, double* W) {
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    double A, B, C;
    if (theta < S3_SMALL) {
        double g[9];
        s3_g(sigma, 8, g);
        const double t2 = theta * theta;
        A = g[1] - t2 * (g[3] / 6 - t2 * (g[5] / 120 - t2 * g[7] / 5040));
        B = g[2] / 2 - t2 * (g[4] / 24 - t2 * (g[6] / 720 - t2 * g[8] / 40320));
        C = g[0];
    } else {
        double g[1];
        s3_g(sigma, 0, g);
        C = g[0];
        const double es = exp(sigma), sn = sin(theta), cs = cos(theta), d = sigma * sigma + theta * theta;
        A = (es * (sigma * sn - theta * cs) + theta) / (theta * d);
        B = (C - (es * (sigma * cs + theta * sn) - sigma) / d) / (theta * theta);
    }
    const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double Om2[9];
    po_mul3(Om, Om, Om2);
    for (int i = 0; i < 9; i++) W[i] = ((i % 4 == 0) ? C : 0.0) + A * Om[i] + B * Om2[i];
}

/* the quaternion products of po_mul, without its translation */
__device__ inline void s3_quat_mul(const PoSE3& A, const PoSE3& B, PoSE3& r) {
    r.qw = A.qw * B.qw - A.qx * B.qx - A.qy * B.qy - A.qz * B.qz;
    r.qx = A.qw * B.qx + A.qx * B.qw + A.qy * B.qz - A.qz * B.qy;
    r.qy = A.qw * B.qy + A.qy * B.qw + A.qz * B.qx - A.qx * B.qz;
    r.qz = A.qw * B.qz + A.qz * B.qw + A.qx * B.qy - A.qy * B.qx;
}
/* A B = (sA sB, RA RB, sA RA tB + tA), normalised like po_mul's product */
__device__ inline PoSim3 s3_mul(const PoSim3& A, const PoSim3& B) {
    PoSim3 r;
    s3_quat_mul(A.T, B.T, r.T);
    const double bt[3] = {B.T.tx, B.T.ty, B.T.tz};
    double rt[3];
    po_rot(A.T, bt, rt);
    r.T.tx = A.s * rt[0] + A.T.tx; r.T.ty = A.s * rt[1] + A.T.ty; r.T.tz = A.s * rt[2] + A.T.tz;
    r.s = A.s * B.s;
    po_normalize(r.T);
    return r;
}
/* (1 / s, R', -(R' t) / s) */
__device__ inline PoSim3 s3_inverse(const PoSim3& S) {
    PoSim3 r;
    r.T.qx = -S.T.qx; r.T.qy = -S.T.qy; r.T.qz = -S.T.qz; r.T.qw = S.T.qw;
    const double t[3] = {S.T.tx, S.T.ty, S.T.tz};
    double rt[3];
    po_rot(r.T, t, rt);
    r.T.tx = -rt[0] / S.s; r.T.ty = -rt[1] / S.s; r.T.tz = -rt[2] / S.s;
    r.s = 1.0 / S.s;
    return r;
}
/* Exp(u), u = (omega, upsilon, sigma): R as po_exp_mul forms it, t = W upsilon, s = e^sigma */
__device__ inline PoSim3 s3_exp(const double* u) {
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double Om[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
    double Om2[9], R[9], W[9], t[3];
    po_mul3(Om, Om, Om2);
    double a, b;
    if (theta < 0.00001) { a = 1.0; b = 0.5; }
    else { a = sin(theta) / theta; b = (1 - cos(theta)) / (theta * theta); }
    for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * Om[i] + b * Om2[i];
    s3_W(u, u[6], W);
    for (int i = 0; i < 3; i++) t[i] = W[i * 3] * u[3] + W[i * 3 + 1] * u[4] + W[i * 3 + 2] * u[5];
    PoSim3 r;
    r.T = po_from_Rt(R, t);
    r.s = exp(u[6]);
    return r;
}
/* r = (omega, upsilon, sigma) with Exp(r) = S, the angle in [0, pi]; S normalised (qw >= 0): upsilon = W^-1 t by the adjugate */
__device__ inline void s3_log(const PoSim3& S, double* r) {
    const double n = sqrt(S.T.qx * S.T.qx + S.T.qy * S.T.qy + S.T.qz * S.T.qz);
    const double theta = 2.0 * atan2(n, S.T.qw);
    const double k = theta < 0.00001 ? 2.0 / S.T.qw : theta / n;
    r[0] = S.T.qx * k; r[1] = S.T.qy * k; r[2] = S.T.qz * k;
    r[6] = log(S.s);
    double W[9];
    s3_W(r, r[6], W);
    const double c00 = W[4] * W[8] - W[5] * W[7], c01 = W[5] * W[6] - W[3] * W[8], c02 = W[3] * W[7] - W[4] * W[6];
    const double det = W[0] * c00 + W[1] * c01 + W[2] * c02;
    const double t[3] = {S.T.tx, S.T.ty, S.T.tz};
    const double inv[9] = {c00, W[2] * W[7] - W[1] * W[8], W[1] * W[5] - W[2] * W[4],
                           c01, W[0] * W[8] - W[2] * W[6], W[2] * W[3] - W[0] * W[5],
                           c02, W[1] * W[6] - W[0] * W[7], W[0] * W[4] - W[1] * W[3]};
    for (int i = 0; i < 3; i++) r[3 + i] = (inv[i * 3] * t[0] + inv[i * 3 + 1] * t[1] + inv[i * 3 + 2] * t[2]) / det;
}
/* Ad(S)(omega, upsilon, sigma) = (R omega, s R upsilon + [t]x R omega - sigma t, sigma), row-major 7x7 */
__device__ inline void s3_adjoint(const PoSim3& S, double* A) {
    double R[9];
    po_to_R(S.T, R);
    const double tx[9] = {0, -S.T.tz, S.T.ty, S.T.tz, 0, -S.T.tx, -S.T.ty, S.T.tx, 0};
    const double t[3] = {S.T.tx, S.T.ty, S.T.tz};
    for (int i = 0; i < 49; i++) A[i] = 0.0;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            A[i * 7 + j] = R[i * 3 + j];
            A[(3 + i) * 7 + 3 + j] = S.s * R[i * 3 + j];
            A[(3 + i) * 7 + j] = tx[i * 3] * R[j] + tx[i * 3 + 1] * R[3 + j] + tx[i * 3 + 2] * R[6 + j];
        }
        A[(3 + i) * 7 + 6] = -t[i];
    }
    A[48] = 1.0;
}
/* C = A B, row-major 7x7 */
__device__ inline void s3_mul7(const double* A, const double* B, double* C) {
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) {
            double s = 0.0;
            for (int k = 0; k < 7; k++) s += A[i * 7 + k] * B[k * 7 + j];
            C[i * 7 + j] = s;
        }
}
/* B_n / n! for the even n = 0 .. 22 (Bernoulli numbers, exact rationals rounded once) */
__device__ static const double S3_JL_COEFF[S3_JL_ORDER / 2 + 1] = {
    1.0, 8.3333333333333329e-02, -1.3888888888888889e-03, 3.3068783068783071e-05, -8.2671957671957675e-07, 2.0876756987868100e-08,
    -5.2841901386874932e-10, 1.3382536530684679e-11, -3.3896802963225827e-13, 8.5860620562778452e-15, -2.1748686985580619e-16,
    5.5090028283602295e-18};
/* inverse left Jacobian of Sim(3) at r: sum_{n <= S3_JL_ORDER} B_n / n! ad(r)^n = I - ad / 2 + (Horner in ad^2 over the even orders),
 * ad(r) = [[Omega, 0, 0], [Upsilon, Omega + sigma I, -upsilon], [0, 0, 0]]; the same count for every input */
__device__ inline void s3_jl_inv(const double* r, double* J) {
    double M[49], P[49], T[49];
    for (int i = 0; i < 49; i++) M[i] = 0.0;
    const double Om[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    const double Up[9] = {0, -r[5], r[4], r[5], 0, -r[3], -r[4], r[3], 0};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            M[i * 7 + j] = Om[i * 3 + j];
            M[(3 + i) * 7 + j] = Up[i * 3 + j];
            M[(3 + i) * 7 + 3 + j] = Om[i * 3 + j] + (i == j ? r[6] : 0.0);
        }
        M[(3 + i) * 7 + 6] = -r[3 + i];
    }
    s3_mul7(M, M, P);
    for (int i = 0; i < 49; i++) J[i] = (i % 8 == 0) ? S3_JL_COEFF[S3_JL_ORDER / 2] : 0.0;
#pragma unroll 1
    for (int n = S3_JL_ORDER / 2 - 1; n >= 0; n--) {
        s3_mul7(J, P, T);
        for (int i = 0; i < 49; i++) J[i] = T[i] + ((i % 8 == 0) ? S3_JL_COEFF[n] : 0.0);
    }
    for (int i = 0; i < 49; i++) J[i] -= 0.5 * M[i];
}

#endif
