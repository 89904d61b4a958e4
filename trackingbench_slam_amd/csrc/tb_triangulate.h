/* The per-point code of the two-view linear triangulation (LocalBA::LinearTriangle with the acceptance gates of
 * include/tb_capi.h, tb_linear_triangle_batch_dev): shared by k_triangulate.hip and k_two_view.hip, which triangulates under
 * the poses it has just found. float64, one operation per statement, only + - * / sqrt, in the order
 * tests/triangulate_reference.py writes down. Everything in registers: every index is a compile-time constant after unrolling. */
#ifndef TB_TRIANGULATE_H
#define TB_TRIANGULATE_H

#include "tb_device.h"

#define TRI_SWEEPS 6

/* one Jacobi rotation on the pair (P, Q), the shim's formulas; skipped only where M[P][Q] == 0 */
template <int P, int Q>
__device__ __forceinline__ void tri_rotate(double (&M)[4][4], double (&V)[4][4]) {
    if (M[P][Q] == 0.0) return;
    const double num = M[Q][Q] - M[P][P];
    const double den = 2.0 * M[P][Q];
    const double th = num / den;
    double r = th * th;
    r = r + 1.0;
    r = sqrt(r);
    r = fabs(th) + r;
    const double t = (th >= 0.0 ? 1.0 : -1.0) / r;
    double c = t * t;
    c = c + 1.0;
    c = sqrt(c);
    c = 1.0 / c;
    const double s = t * c;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double a = M[k][P], b = M[k][Q];
        const double ca = c * a, sb = s * b, sa = s * a, cb = c * b;
        M[k][P] = ca - sb;
        M[k][Q] = sa + cb;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double a = M[P][k], b = M[Q][k];
        const double ca = c * a, sb = s * b, sa = s * a, cb = c * b;
        M[P][k] = ca - sb;
        M[Q][k] = sa + cb;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double a = V[k][P], b = V[k][Q];
        const double ca = c * a, sb = s * b, sa = s * a, cb = c * b;
        V[k][P] = ca - sb;
        V[k][Q] = sa + cb;
    }
}

/* row r of T applied to (X, 1) */
__device__ __forceinline__ double tri_row(const double (&T)[16], int r, double X, double Y, double Z) {
    double a = T[r * 4 + 0] * X;
    const double b = T[r * 4 + 1] * Y;
    a = a + b;
    const double c = T[r * 4 + 2] * Z;
    a = a + c;
    return a + T[r * 4 + 3];
}

__device__ __forceinline__ double tri_dot(double ax, double ay, double az, double bx, double by, double bz) {
    double d = ax * bx;
    const double e = ay * by;
    d = d + e;
    const double f = az * bz;
    return d + f;
}

/* squared pixel error of X in the view T, times inv_sigma2 */
__device__ __forceinline__ double tri_chi2(const double (&T)[16], double X, double Y, double Z, double z, double u, double v, double fx,
                                           double fy, double cx, double cy, double inv_sigma2) {
    double pu = tri_row(T, 0, X, Y, Z) / z;
    pu = fx * pu;
    pu = pu + cx;
    double pv = tri_row(T, 1, X, Y, Z) / z;
    pv = fy * pv;
    pv = pv + cy;
    const double du = pu - u, dv = pv - v;
    const double e0 = du * du, e1 = dv * dv;
    const double e = e0 + e1;
    return e * inv_sigma2;
}

/* one point pair: pixels (u0, v0) in the view T0 and (u1, v1) in the view T1 (row-major 4 x 4), inv_sigma2 s0 / s1. Returns the
 * flag 1..5 (the first failing gate decides) and the float32 point, which is meaningful wherever the flag is not 2. */
__device__ __forceinline__ int tri_point(const double (&T0)[16], const double (&T1)[16], double u0, double v0, double u1, double v1,
                                         double s0, double s1, double fx, double fy, double cx, double cy, double cos_parallax_max,
                                         double chi2_max, float& Xf, float& Yf, float& Zf) {
    int flag;
    double x0 = u0 - cx, y0 = v0 - cy, x1 = u1 - cx, y1 = v1 - cy;
    x0 = x0 / fx; y0 = y0 / fy; x1 = x1 / fx; y1 = y1 / fy;
    double A[4][4], M[4][4], V[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double a0 = x0 * T0[8 + c], a1 = y0 * T0[8 + c], a2 = x1 * T1[8 + c], a3 = y1 * T1[8 + c];
        A[0][c] = a0 - T0[c];
        A[1][c] = a1 - T0[4 + c];
        A[2][c] = a2 - T1[c];
        A[3][c] = a3 - T1[4 + c];
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = r; c < 4; c++) {
            double m = A[0][r] * A[0][c];
            const double m1 = A[1][r] * A[1][c];
            m = m + m1;
            const double m2 = A[2][r] * A[2][c];
            m = m + m2;
            const double m3 = A[3][r] * A[3][c];
            m = m + m3;
            M[r][c] = m;
            M[c][r] = m;
            V[r][c] = r == c ? 1.0 : 0.0;
            V[c][r] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < TRI_SWEEPS; sweep++) {
        tri_rotate<0, 1>(M, V);
        tri_rotate<0, 2>(M, V);
        tri_rotate<0, 3>(M, V);
        tri_rotate<1, 2>(M, V);
        tri_rotate<1, 3>(M, V);
        tri_rotate<2, 3>(M, V);
    }
    /* the column at the smallest diagonal entry, the lowest index on a tie */
    double best = M[0][0], h0 = V[0][0], h1 = V[1][0], h2 = V[2][0], h3 = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (M[k][k] < best) { best = M[k][k]; h0 = V[0][k]; h1 = V[1][k]; h2 = V[2][k]; h3 = V[3][k]; }
    const double X = h0 / h3, Y = h1 / h3, Z = h2 / h3;
    Xf = (float)X; Yf = (float)Y; Zf = (float)Z;
    const double z0 = tri_row(T0, 2, X, Y, Z), z1 = tri_row(T1, 2, X, Y, Z);
    /* the pixels' rays in the world frame: R^T (x, y, 1) */
    double r0[3], r1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double a = T0[k] * x0;
        const double b = T0[4 + k] * y0;
        a = a + b;
        r0[k] = a + T0[8 + k];
        double c = T1[k] * x1;
        const double d = T1[4 + k] * y1;
        c = c + d;
        r1[k] = c + T1[8 + k];
    }
    const double n0 = sqrt(tri_dot(r0[0], r0[1], r0[2], r0[0], r0[1], r0[2]));
    const double n1 = sqrt(tri_dot(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2]));
    const double nn = n0 * n1;
    const double cosv = tri_dot(r0[0], r0[1], r0[2], r1[0], r1[1], r1[2]) / nn;
    const double c0 = tri_chi2(T0, X, Y, Z, z0, u0, v0, fx, fy, cx, cy, s0);
    const double c1 = tri_chi2(T1, X, Y, Z, z1, u1, v1, fx, fy, cx, cy, s1);
    if (h3 == 0.0 || !isfinite(Xf) || !isfinite(Yf) || !isfinite(Zf)) flag = 2;
    else if (!(z0 > 0.0) || !(z1 > 0.0)) flag = 3;
    else if (!(cosv < cos_parallax_max)) flag = 4;
    else if (c0 > chi2_max || c1 > chi2_max) flag = 5;
    else flag = 1;
    return flag;
}

#endif
