/* Sim(3) from 3D-3D rows: Horn's closed form inside a RANSAC with a least-squares refit (tb_sim3_ransac_batch_dev,
 * include/tb_capi.h; DESIGN.md 9n has the derivation, tests/sim3_reference.py is the definition, statement for statement).
 *
 * One 256-thread workgroup per problem. Thread t owns the hypotheses t, t + 256, ...: it draws the sample (k_pnp's rule), runs
 * Horn's solver in registers (float64, one operation per statement, only + - * / sqrt fabs and comparisons, fixed loop counts;
 * the library builds with -ffp-contract=off; the 4 x 4 Jacobi is tb_triangulate.h's rotation) and scores its transform against
 * every row. The rows and the two projections of each row's own points sit in LDS as doubles, one chunk of S3_CHUNK at a time,
 * and all lanes read the same row at once: a broadcast, no bank conflict. A problem of at most one chunk is staged once. A
 * thread's best (count, hypothesis, q, s, t) stays in its registers; the winner is one max-reduction over the packed key
 * (count + 1, -hypothesis) and its owner hands (q, s, t) over through LDS. The refit walks the rows with lanes as rows (thread t
 * takes rows t, t + 256, ...) in three passes -- centroids, centred moments, scale -- each ending in the fixed butterfly, solves
 * in every thread redundantly, and is counted with the arithmetic that counted the hypotheses. The mask is written with the
 * same function.
 *
 * Work: FP64 VALU, about 70 operations and four divisions per row and hypothesis and about 1500 per hypothesis for the solver;
 * not HBM (DESIGN.md 9n has the measured times). */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_triangulate.h"

#define S3_T 256
#define S3_CHUNK 256 /* rows per LDS chunk: 24 KiB of doubles */
#define S3_DRAWS 8
#define S3_SWEEPS 5  /* tests/test_sim3_reference.py: with the correction below, 4 agree with eigh to 1e-12; plus one */
#define S3_SPLIT 134217729.0 /* 2^27 + 1: Veltkamp's splitter */
#define S3_DEGENERATE 1e-6
#define S3_DBL_MAX 1.7976931348623157e308

__device__ __forceinline__ unsigned long long s3_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ bool s3_finite(double v) { return fabs(v) <= S3_DBL_MAX; }

__device__ __forceinline__ double s3_dot(const double (&a)[3], const double (&b)[3]) {
    double d = a[0] * b[0];
    d = d + a[1] * b[1];
    return d + a[2] * b[2];
}

__device__ __forceinline__ void s3_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* R12 (row-major) of the unit quaternion w x y z */
__device__ __forceinline__ void s3_rotation(const double (&q)[4], double (&R)[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, xz = x * z, yz = y * z;
    const double wx = w * x, wy = w * y, wz = w * z;
    double d = yy + zz;
    d = 2.0 * d;
    R[0] = 1.0 - d;
    d = xx + zz;
    d = 2.0 * d;
    R[4] = 1.0 - d;
    d = xx + yy;
    d = 2.0 * d;
    R[8] = 1.0 - d;
    d = xy - wz;
    R[1] = 2.0 * d;
    d = xz + wy;
    R[2] = 2.0 * d;
    d = xy + wz;
    R[3] = 2.0 * d;
    d = yz - wx;
    R[5] = 2.0 * d;
    d = xz - wy;
    R[6] = 2.0 * d;
    d = yz + wx;
    R[7] = 2.0 * d;
}

/* p = fl(a b) and a b = p + e exactly (Dekker; no fused multiply-add). s3_two_prod and s3_two_sum are exact only while the
 * compiler performs every statement as written: the Makefile's -ffp-contract=off and -fno-fast-math are load-bearing here (a
 * contracted or reassociated build would still compile and would silently lose the correction below) */
__device__ __forceinline__ void s3_two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    double c = S3_SPLIT * a;
    double d = c - a;
    const double ah = c - d, al = a - ah;
    c = S3_SPLIT * b;
    d = c - b;
    const double bh = c - d, bl = b - bh;
    e = ah * bh;
    e = e - p;
    e = e + ah * bl;
    e = e + al * bh;
    e = e + al * bl;
}

/* s = fl(a + b) and a + b = s + e exactly (Knuth) */
__device__ __forceinline__ void s3_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = s - bb;
    e = a - e;
    const double f = b - bb;
    e = e + f;
}

/* the quaternion of R12 from M[i][j] = sum Pr2[i] Pr1[j] (row-major): Horn's N, the Jacobi sweeps, the column k at the largest
 * diagonal entry (the lowest index on a tie), one first-order correction of that column from its residual r = N v - lam v against
 * the N the sweeps started from (every product and partial sum of r carried with its rounding error, rounded once at the end):
 * v + sum_(i != k) (v_i . r) / (lam_k - lam_i) v_i, a term left out where its denominator is 0; then w >= 0 */
__device__ __forceinline__ void s3_quaternion(const double (&M)[9], double (&q)[4]) {
    double N[4][4], V[4][4], N0[4][4];
    double a = M[0] + M[4];
    N[0][0] = a + M[8];
    a = M[0] - M[4];
    N[1][1] = a - M[8];
    a = M[4] - M[0];
    N[2][2] = a - M[8];
    a = M[8] - M[0];
    N[3][3] = a - M[4];
    N[0][1] = M[5] - M[7];
    N[0][2] = M[6] - M[2];
    N[0][3] = M[1] - M[3];
    N[1][2] = M[1] + M[3];
    N[1][3] = M[6] + M[2];
    N[2][3] = M[5] + M[7];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < i) N[i][j] = N[j][i];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) N0[i][j] = N[i][j];
    for (int sweep = 0; sweep < S3_SWEEPS; sweep++) {
        tri_rotate<0, 1>(N, V);
        tri_rotate<0, 2>(N, V);
        tri_rotate<0, 3>(N, V);
        tri_rotate<1, 2>(N, V);
        tri_rotate<1, 3>(N, V);
        tri_rotate<2, 3>(N, V);
    }
    double best = N[0][0];
    int kidx = 0;
    q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (N[k][k] > best) { best = N[k][k]; kidx = k; q[0] = V[0][k]; q[1] = V[1][k]; q[2] = V[2][k]; q[3] = V[3][k]; }
    double r[4];
    const double nlam = -best;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double hi, lo;
        s3_two_prod(N0[j][0], q[0], hi, lo);
#pragma unroll
        for (int m = 1; m < 5; m++) {
            double p, e, t;
            s3_two_prod(m < 4 ? N0[j][m < 4 ? m : 0] : nlam, m < 4 ? q[m < 4 ? m : 0] : q[j], p, e);
            s3_two_sum(hi, p, hi, t);
            t = t + e;
            lo = lo + t;
        }
        r[j] = hi + lo;
    }
    double o[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double c = V[0][i] * r[0];
        c = c + V[1][i] * r[1];
        c = c + V[2][i] * r[2];
        c = c + V[3][i] * r[3];
        const double d = best - N[i][i];
        const double coef = (kidx != i && d != 0.0) ? c / d : 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = o[j] + coef * V[j][i];
    }
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = o[3];
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
}

/* t12 = O1 - s (R12 O2) */
__device__ __forceinline__ void s3_translation(const double (&R)[9], double s, const double (&O1)[3], const double (&O2)[3], double (&t)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double a = R[3 * i] * O2[0];
        a = a + R[3 * i + 1] * O2[1];
        a = a + R[3 * i + 2] * O2[2];
        a = s * a;
        t[i] = O1[i] - a;
    }
}

/* what the score uses of (q, s, t12) */
struct S3Transform {
    double sR12[9], t12[3], sR21[9], t21[3];
};

/* false: the transform is void (s not finite or not above 0, or an entry of t12, t21, s21 not finite) */
__device__ __forceinline__ bool s3_derive(const double (&q)[4], double s, const double (&t)[3], S3Transform& T) {
    double R[9];
    s3_rotation(q, R);
    const double s21 = 1.0 / s;
    bool ok = s > 0.0 && s3_finite(s) && s3_finite(s21);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            T.sR12[3 * i + j] = s * R[3 * i + j];
            T.sR21[3 * i + j] = s21 * R[3 * j + i];
        }
        double b = R[i] * t[0];
        b = b + R[3 + i] * t[1];
        b = b + R[6 + i] * t[2];
        b = -b;
        T.t21[i] = b / s;
        T.t12[i] = t[i];
        ok = ok && s3_finite(t[i]) && s3_finite(T.t21[i]);
    }
    return ok;
}

__device__ __forceinline__ void s3_project(double X, double Y, double Z, double fx, double fy, double cx, double cy, double& u, double& v) {
    u = X / Z;
    u = fx * u;
    u = u + cx;
    v = Y / Z;
    v = fy * v;
    v = v + cy;
}

/* one row as the score reads it: the two points, their own projections, the two weights */
struct S3Row {
    double X1, Y1, Z1, X2, Y2, Z2, u1, v1, u2, v2, w1, w2;
};

__device__ __forceinline__ S3Row s3_row(const tb_sim3_row& r, double fx, double fy, double cx, double cy) {
    S3Row o;
    o.X1 = (double)r.X1; o.Y1 = (double)r.Y1; o.Z1 = (double)r.Z1;
    o.X2 = (double)r.X2; o.Y2 = (double)r.Y2; o.Z2 = (double)r.Z2;
    o.w1 = (double)r.inv_sigma2_1; o.w2 = (double)r.inv_sigma2_2;
    s3_project(o.X1, o.Y1, o.Z1, fx, fy, cx, cy, o.u1, o.v1);
    s3_project(o.X2, o.Y2, o.Z2, fx, fy, cx, cy, o.u2, o.v2);
    return o;
}

/* the inlier rule on one row */
__device__ __forceinline__ bool s3_inlier(const S3Transform& T, const S3Row& r, double fx, double fy, double cx, double cy, double chi2_max) {
    double Q1[3], Q2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double a = T.sR12[3 * i] * r.X2;
        a = a + T.sR12[3 * i + 1] * r.Y2;
        a = a + T.sR12[3 * i + 2] * r.Z2;
        Q1[i] = a + T.t12[i];
        double b = T.sR21[3 * i] * r.X1;
        b = b + T.sR21[3 * i + 1] * r.Y1;
        b = b + T.sR21[3 * i + 2] * r.Z1;
        Q2[i] = b + T.t21[i];
    }
    double pu, pv;
    s3_project(Q1[0], Q1[1], Q1[2], fx, fy, cx, cy, pu, pv);
    double du = pu - r.u1, dv = pv - r.v1;
    double e = du * du;
    e = e + dv * dv;
    const double c1 = e * r.w1;
    s3_project(Q2[0], Q2[1], Q2[2], fx, fy, cx, cy, pu, pv);
    du = pu - r.u2;
    dv = pv - r.v2;
    e = du * du;
    e = e + dv * dv;
    const double c2 = e * r.w2;
    return r.Z1 > 0.0 && r.Z2 > 0.0 && Q1[2] > 0.0 && Q2[2] > 0.0 && c1 <= chi2_max && c2 <= chi2_max;
}

/* Horn on the three points of a sample (P[point][coordinate]); a sum over the points is ((0 + v0) + v1) + v2. False: void. */
__device__ __forceinline__ bool s3_sample(const double (&P1)[3][3], const double (&P2)[3][3], int fixed_scale, double (&q)[4], double& s,
                                          double (&t)[3]) {
    bool ok = true;
#pragma unroll
    for (int set = 0; set < 2; set++) {
        const double (&P)[3][3] = set == 0 ? P1 : P2;
        double a[3], b[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            ok = ok && s3_finite(P[0][k]) && s3_finite(P[1][k]) && s3_finite(P[2][k]);
            a[k] = P[1][k] - P[0][k];
            b[k] = P[2][k] - P[0][k];
        }
        ok = ok && P[0][2] > 0.0 && P[1][2] > 0.0 && P[2][2] > 0.0;
        s3_cross(a, b, c);
        const double cc = s3_dot(c, c), aa = s3_dot(a, a), bb = s3_dot(b, b);
        double lim = S3_DEGENERATE * aa;
        lim = lim * bb;
        ok = ok && cc > lim;
    }
    double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double a = 0.0 + P1[0][k];
        a = a + P1[1][k];
        a = a + P1[2][k];
        O1[k] = a / 3.0;
        double b = 0.0 + P2[0][k];
        b = b + P2[1][k];
        b = b + P2[2][k];
        O2[k] = b / 3.0;
    }
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Pr1[p][k] = P1[p][k] - O1[k];
            Pr2[p][k] = P2[p][k] - O2[k];
        }
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double a = 0.0 + Pr2[0][i] * Pr1[0][j];
            a = a + Pr2[1][i] * Pr1[1][j];
            M[3 * i + j] = a + Pr2[2][i] * Pr1[2][j];
        }
    s3_quaternion(M, q);
    double R[9];
    s3_rotation(q, R);
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        double P3[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double a = R[3 * i] * Pr2[p][0];
            a = a + R[3 * i + 1] * Pr2[p][1];
            P3[i] = a + R[3 * i + 2] * Pr2[p][2];
        }
        nom = nom + s3_dot(Pr1[p], P3);
        den = den + s3_dot(P3, P3);
    }
    s = fixed_scale ? 1.0 : nom / den;
    s3_translation(R, s, O1, O2, t);
    return ok;
}

/* the refit's sum: every thread's partial sums acc[] meet in the butterfly t ^ 1, 2, ..., 128 (the wave's six steps by
 * shuffles; the four wave sums through LDS as (w0 + w1) + (w2 + w3), which is what the steps 64 and 128 give lane 0). Called
 * by the whole block; every thread gets the same bits. */
template <int K>
__device__ __forceinline__ void s3_block_sum(double (&acc)[K], double (*red)[9]) {
#pragma unroll
    for (int e = 0; e < K; e++) {
#pragma unroll
        for (int d = 1; d < TB_WAVE; d <<= 1) acc[e] = acc[e] + __shfl_xor(acc[e], d, TB_WAVE);
    }
    __syncthreads();
    if (tb_lane() == 0) {
#pragma unroll
        for (int e = 0; e < K; e++) red[threadIdx.x >> 6][e] = acc[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < K; e++) {
        const double lo = red[0][e] + red[1][e];
        const double hi = red[2][e] + red[3][e];
        acc[e] = lo + hi;
    }
}

__device__ __forceinline__ int s3_block_count(int v, int* cnt) {
#pragma unroll
    for (int d = 1; d < TB_WAVE; d <<= 1) v += __shfl_xor(v, d, TB_WAVE);
    __syncthreads();
    if (tb_lane() == 0) cnt[threadIdx.x >> 6] = v;
    __syncthreads();
    return cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ void __launch_bounds__(S3_T)
k_sim3(double fx, double fy, double cx, double cy, const tb_sim3_row* __restrict__ rowsAll, const int32_t* __restrict__ counts, int pitch,
       int H, int fixed_scale, double chi2_max, unsigned long long seed, float* __restrict__ S12, double* __restrict__ srt,
       int32_t* __restrict__ consensus, uint8_t* __restrict__ inlierAll, int32_t* __restrict__ winner, int32_t* __restrict__ flags) {
    __shared__ S3Row rows[S3_CHUNK];
    __shared__ double red[S3_T / TB_WAVE][9];
    __shared__ double winQ[8];
    __shared__ unsigned long long wkey[S3_T / TB_WAVE];
    __shared__ int cnt4[S3_T / TB_WAVE];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[p], 0), pitch);
    const tb_sim3_row* R = rowsAll + (size_t)p * pitch;

    unsigned long long bestKey = 0; /* (count + 1) << 16 | (1023 - h); 0 = nothing */
    double bestQ[8];                /* q, t12, s */
#pragma unroll
    for (int k = 0; k < 8; k++) bestQ[k] = 0.0;

    if (n >= 3) { /* block-uniform */
        const bool resident = n <= S3_CHUNK;
        auto stage = [&](int base) {
            const int i = base + tid;
            if (tid < S3_CHUNK && i < n) rows[tid] = s3_row(R[i], fx, fy, cx, cy);
        };
        if (resident) {
            stage(0);
            __syncthreads();
        }
        for (int h0 = 0; h0 < H; h0 += S3_T) {
            const int h = h0 + tid;
            bool valid = h < H;
            double q[4] = {1.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0}, s = 1.0;
            S3Transform T;
            if (valid) {
                /* draws until three distinct rows or S3_DRAWS are used up */
                int i0 = -1, i1 = -1, i2 = -1;
                for (int k = 0; k < S3_DRAWS; k++) {
                    const unsigned long long z = s3_mix(seed + ((unsigned long long)h * 8ull + (unsigned long long)(k + 1)) * 0x9E3779B97F4A7C15ull);
                    const int d = (int)(((z >> 32) * (unsigned long long)n) >> 32);
                    if (i0 < 0) i0 = d;
                    else if (i1 < 0) { if (d != i0) i1 = d; }
                    else if (i2 < 0) { if (d != i0 && d != i1) i2 = d; }
                }
                valid = i2 >= 0;
                if (valid) {
                    double P1[3][3], P2[3][3];
                    const int ix[3] = {i0, i1, i2};
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const tb_sim3_row r = R[ix[i]];   /* ix[i] < n <= pitch */
                        P1[i][0] = (double)r.X1; P1[i][1] = (double)r.Y1; P1[i][2] = (double)r.Z1;
                        P2[i][0] = (double)r.X2; P2[i][1] = (double)r.Y2; P2[i][2] = (double)r.Z2;
                    }
                    valid = s3_sample(P1, P2, fixed_scale, q, s, t);
                    const bool okT = s3_derive(q, s, t, T);
                    valid = valid && okT;
                }
            }
            /* every thread scores its transform (if it has one) against all rows */
            int cnt = 0;
            for (int base = 0; base < n; base += S3_CHUNK) {
                if (!resident) {
                    __syncthreads();
                    stage(base);
                    __syncthreads();
                }
                if (valid) {
                    const int m = min(S3_CHUNK, n - base);
                    for (int i = 0; i < m; i++) cnt += s3_inlier(T, rows[i], fx, fy, cx, cy, chi2_max) ? 1 : 0;
                }
            }
            if (valid) {
                const unsigned long long key = ((unsigned long long)(cnt + 1) << 16) | (unsigned long long)(1023 - h);
                if (key > bestKey) {
                    bestKey = key;
#pragma unroll
                    for (int k = 0; k < 4; k++) bestQ[k] = q[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) bestQ[4 + k] = t[k];
                    bestQ[7] = s;
                }
            }
        }
    }
    /* the winner: max of the keys, which are distinct wherever they are not 0 */
    unsigned long long k = bestKey;
#pragma unroll
    for (int d = TB_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(k, d, TB_WAVE);
        k = o > k ? o : k;
    }
    __syncthreads(); /* the last pass's row reads are done */
    if (tb_lane() == 0) wkey[tid >> 6] = k;
    __syncthreads();
    unsigned long long win = wkey[0];
#pragma unroll
    for (int w = 1; w < S3_T / TB_WAVE; w++) win = wkey[w] > win ? wkey[w] : win;
    if (win != 0 && bestKey == win) {
#pragma unroll
        for (int i = 0; i < 8; i++) winQ[i] = bestQ[i];
    }
    __syncthreads();
    uint8_t* inl = inlierAll ? inlierAll + (size_t)p * pitch : nullptr;
    if (win == 0) { /* void: the identity, scale 1, an empty mask */
        if (S12 && tid < 16) S12[16 * (size_t)p + tid] = (tid % 5) == 0 ? 1.f : 0.f;
        if (srt && tid < 8) srt[8 * (size_t)p + tid] = (tid == 0 || tid == 7) ? 1.0 : 0.0;
        if (inl)
            for (int i = tid; i < pitch; i += S3_T) inl[i] = 0;
        if (tid == 0) {
            if (consensus) consensus[p] = 0;
            if (winner) { winner[2 * p] = -2; winner[2 * p + 1] = 0; }
            if (flags) flags[p] = 1;
        }
        return;
    }
    double q[4], t[3], s;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = winQ[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = winQ[4 + i];
    s = winQ[7];
    S3Transform T;
    s3_derive(q, s, t, T);
    int best = (int)(win >> 16) - 1;
    int refitted = 0;
    if (best >= 3) { /* block-uniform: the refit on the winner's consensus rows, lanes as rows */
        double a6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += S3_T) {
            const S3Row r = s3_row(R[i], fx, fy, cx, cy);
            if (s3_inlier(T, r, fx, fy, cx, cy, chi2_max)) {
                a6[0] = a6[0] + r.X1; a6[1] = a6[1] + r.Y1; a6[2] = a6[2] + r.Z1;
                a6[3] = a6[3] + r.X2; a6[4] = a6[4] + r.Y2; a6[5] = a6[5] + r.Z2;
            }
        }
        s3_block_sum<6>(a6, red);
        const double m = (double)best;
        const double O1[3] = {a6[0] / m, a6[1] / m, a6[2] / m}, O2[3] = {a6[3] / m, a6[4] / m, a6[5] / m};
        double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += S3_T) {
            const S3Row r = s3_row(R[i], fx, fy, cx, cy);
            if (s3_inlier(T, r, fx, fy, cx, cy, chi2_max)) {
                const double Pr1[3] = {r.X1 - O1[0], r.Y1 - O1[1], r.Z1 - O1[2]}, Pr2[3] = {r.X2 - O2[0], r.Y2 - O2[1], r.Z2 - O2[2]};
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) M[3 * a + b] = M[3 * a + b] + Pr2[a] * Pr1[b];
            }
        }
        s3_block_sum<9>(M, red);
        double qr[4], Rr[9], tr[3], sr = 1.0;
        s3_quaternion(M, qr);
        s3_rotation(qr, Rr);
        if (!fixed_scale) { /* block-uniform */
            double nd[2] = {0.0, 0.0};
            for (int i = tid; i < n; i += S3_T) {
                const S3Row r = s3_row(R[i], fx, fy, cx, cy);
                if (s3_inlier(T, r, fx, fy, cx, cy, chi2_max)) {
                    const double Pr1[3] = {r.X1 - O1[0], r.Y1 - O1[1], r.Z1 - O1[2]}, Pr2[3] = {r.X2 - O2[0], r.Y2 - O2[1], r.Z2 - O2[2]};
                    double P3[3];
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        double v = Rr[3 * a] * Pr2[0];
                        v = v + Rr[3 * a + 1] * Pr2[1];
                        P3[a] = v + Rr[3 * a + 2] * Pr2[2];
                    }
                    nd[0] = nd[0] + s3_dot(Pr1, P3);
                    nd[1] = nd[1] + s3_dot(P3, P3);
                }
            }
            s3_block_sum<2>(nd, red);
            sr = nd[0] / nd[1];
        }
        s3_translation(Rr, sr, O1, O2, tr);
        S3Transform Tr;
        const bool okr = s3_derive(qr, sr, tr, Tr);   /* the same bits in every thread */
        int c = 0;
        if (okr)
            for (int i = tid; i < n; i += S3_T) c += s3_inlier(Tr, s3_row(R[i], fx, fy, cx, cy), fx, fy, cx, cy, chi2_max) ? 1 : 0;
        c = s3_block_count(c, cnt4);
        if (okr && c >= best) {
            refitted = 1;
            best = c;
            T = Tr;
            s = sr;
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = qr[i];
#pragma unroll
            for (int i = 0; i < 3; i++) t[i] = tr[i];
        }
    }
    if (S12 && tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = (r == 3 && c == 3) ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (r == i && c == j) v = (float)(j < 3 ? T.sR12[3 * i + j] : T.t12[i]);
        S12[16 * (size_t)p + tid] = v;
    }
    if (srt && tid < 8) {
        double v = s;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (tid == i) v = q[i];
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (tid == 4 + i) v = t[i];
        srt[8 * (size_t)p + tid] = v;
    }
    if (inl)
        for (int i = tid; i < pitch; i += S3_T) {
            bool in = false;
            if (i < n) in = s3_inlier(T, s3_row(R[i], fx, fy, cx, cy), fx, fy, cx, cy, chi2_max);
            inl[i] = in ? 1 : 0;
        }
    if (tid == 0) {
        if (consensus) consensus[p] = best;
        if (winner) { winner[2 * p] = 1023 - (int)(win & 0xffff); winner[2 * p + 1] = refitted; }
        if (flags) flags[p] = 0;
    }
}

/* ---- the keyframe store's Sim(3) query (tb_kf_store_sim3_dev). Pair c = s * ncand + r (one workgroup each): the 3D-3D rows
 * through the verification's match list, by k_reloc_rows' rule with one more condition -- a match counts where the stored entry
 * trainIdx AND the query key queryIdx both have a map point; the last such match in list order wins a key (win[], in LDS: one int
 * per query key); one row per key that has one, IN KEY ORDER. X1 = the query's Tcw applied to the query key's world point, X2 =
 * the stored keyframe's Tcw applied to its stored world point, both in float64 (one operation per statement) and stored as
 * float32; the weights are invLevelSigma2[octave] of the two keys. A slot of -1, one outside the ring or an empty one is no
 * candidate: no rows, cand_kf -1.
 * The kernel is a template over the row type: tb_sim3_row for the solver, tb_sim3_obs_row for the optimiser's query
 * (tb_kf_store_sim3_refine_dev), which adds the two keys' x, y as (u1, v1), (u2, v2) the way k_reloc_rows takes them for its tb_obs
 * rows. Same keys, same order: row i of a pair is the same match in both lists. */
struct tb_sim3_sigma {
    float v[TB_MAX_LEVELS];
    int n;
};

__device__ __forceinline__ float s3_apply(const float* __restrict__ T, int r, float X, float Y, float Z) {
    double a = (double)T[4 * r] * (double)X;
    a = a + (double)T[4 * r + 1] * (double)Y;
    a = a + (double)T[4 * r + 2] * (double)Z;
    a = a + (double)T[4 * r + 3];
    return (float)a;
}

__device__ __forceinline__ void s3_set_pixels(tb_sim3_row&, const tb_keypoint&, const tb_keypoint&) {}
__device__ __forceinline__ void s3_set_pixels(tb_sim3_obs_row& r, const tb_keypoint& k1, const tb_keypoint& k2) {
    r.u1 = k1.x; r.v1 = k1.y;
    r.u2 = k2.x; r.v2 = k2.y;
}

/* win[q] (LDS, one int per query key below n) = the index of the last match in list order that counts for key q, or -1: the row
 * rule's selection, stated once for the row kernel and for the search query's prep. Every thread of the 256 calls it; it ends on a
 * barrier. */
__device__ __forceinline__ void s3_row_winners(int* win, int n, const tb_match* __restrict__ M, int nm, int nk, const uint8_t* __restrict__ V1,
                                               const uint8_t* __restrict__ V2) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) win[i] = -1;
    __syncthreads();
    for (int k = tid; k < nm; k += 256) {
        const int q = M[k].queryIdx, tr = M[k].trainIdx;
        if (q >= 0 && q < n && tr >= 0 && tr < nk && V2[tr] && V1[q]) atomicMax(&win[q], k);
    }
    __syncthreads();
}

/* the frame s * cap + slot of pair c and its keyframe id, or -1, -1 where the slot is no candidate */
__device__ __forceinline__ void s3_pair_frame(int c, int ncand, int cap, const int32_t* __restrict__ cand_slot, const int32_t* __restrict__ kf_ids,
                                              int& f, int& kf) {
    const int s = c / ncand, slot = cand_slot[c];
    f = -1; kf = -1;
    if (slot >= 0 && slot < cap) {
        kf = kf_ids[(size_t)s * cap + slot];
        if (kf >= 0) f = s * cap + slot; else kf = -1;
    }
}

template <typename Row>
__global__ void __launch_bounds__(256)
k_sim3_rows(int ncand, int cap, const int32_t* __restrict__ cand_slot, const int32_t* __restrict__ kf_ids, const tb_keypoint* __restrict__ q_keys,
            const int32_t* __restrict__ q_counts, const float* __restrict__ q_mp, const uint8_t* __restrict__ q_valid, int q_pitch,
            const float* __restrict__ q_Tcw, const tb_match* __restrict__ matches, const int32_t* __restrict__ match_counts,
            const tb_keypoint* __restrict__ kf_keys, const float* __restrict__ kf_mp, const uint8_t* __restrict__ kf_valid,
            const int32_t* __restrict__ kf_counts, const float* __restrict__ kf_Tcw, int pitch, tb_sim3_sigma sig,
            Row* __restrict__ rows, int32_t* __restrict__ row_counts, int32_t* __restrict__ cand_kf, int32_t* __restrict__ rows_out) {
    extern __shared__ int win[];   /* [q_pitch] */
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int s = c / ncand;
    int f, kf;
    s3_pair_frame(c, ncand, cap, cand_slot, kf_ids, f, kf);
    if (f < 0) {
        if (tid == 0) { row_counts[c] = 0; cand_kf[c] = -1; if (rows_out) rows_out[c] = 0; }
        return;
    }
    const int n = min(max(q_counts[s], 0), q_pitch);
    const int nm = min(max(match_counts[c], 0), pitch);
    const int nk = min(max(kf_counts[f], 0), pitch);
    const tb_keypoint* K1 = q_keys + (size_t)s * q_pitch;
    const float* MP1 = q_mp + 3 * (size_t)s * q_pitch;
    const uint8_t* V1 = q_valid + (size_t)s * q_pitch;
    const float* T1 = q_Tcw + 16 * (size_t)s;
    const tb_match* M = matches + (size_t)c * pitch;
    const tb_keypoint* K2 = kf_keys + (size_t)f * pitch;
    const float* MP2 = kf_mp + 3 * (size_t)f * pitch;
    const uint8_t* V2 = kf_valid + (size_t)f * pitch;
    const float* T2 = kf_Tcw + 16 * (size_t)f;
    Row* O = rows + (size_t)c * pitch;
    s3_row_winners(win, n, M, nm, nk, V1, V2);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        Row r = {};
        if (i < n) {
            const int k = win[i];
            ok = k >= 0;
            if (ok) {
                const int j = M[k].trainIdx;
                const float a0 = MP1[3 * i], a1 = MP1[3 * i + 1], a2 = MP1[3 * i + 2];
                const float b0 = MP2[3 * j], b1 = MP2[3 * j + 1], b2 = MP2[3 * j + 2];
                r.X1 = s3_apply(T1, 0, a0, a1, a2); r.Y1 = s3_apply(T1, 1, a0, a1, a2); r.Z1 = s3_apply(T1, 2, a0, a1, a2);
                r.X2 = s3_apply(T2, 0, b0, b1, b2); r.Y2 = s3_apply(T2, 1, b0, b1, b2); r.Z2 = s3_apply(T2, 2, b0, b1, b2);
                r.inv_sigma2_1 = sig.v[min(max(K1[i].octave, 0), sig.n - 1)];
                r.inv_sigma2_2 = sig.v[min(max(K2[j].octave, 0), sig.n - 1)];
                s3_set_pixels(r, K1[i], K2[j]);
            }
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) O[at] = r; /* at <= i < n <= q_pitch <= pitch */
    }
    if (tid == 0) { row_counts[c] = base; cand_kf[c] = kf; if (rows_out) rows_out[c] = base; }
}

/* Per sequence (one thread each): the candidate with the largest consensus, ties to the lower rank, candidates that are absent
 * left out; it is the answer when its consensus reaches min_consensus. best_rank -1: best_kf -1, the identity and scale 1.
 * keep_kf / keep_srt (nullable): the store's own copy of best_kf / best_srt, which tb_kf_store_sim3_graph_dev reads. */
__device__ __forceinline__ int s3_select_rank(int ncand, int min_consensus, const int32_t* __restrict__ cand_kf,
                                              const int32_t* __restrict__ cand_consensus, int s) {
    int best = -1, most = -1;
    for (int r = 0; r < ncand; r++) {
        const size_t c = (size_t)s * ncand + r;
        if (cand_kf[c] < 0) continue;
        const int ni = cand_consensus[c];
        if (ni > most) { most = ni; best = r; }
    }
    if (best >= 0 && most < min_consensus) best = -1;
    return best;
}

__global__ void __launch_bounds__(256)
k_sim3_select(int nseq, int ncand, int min_consensus, const int32_t* __restrict__ cand_kf, const int32_t* __restrict__ cand_consensus,
              const float* __restrict__ cand_S12, const double* __restrict__ cand_srt, int32_t* __restrict__ best_rank,
              int32_t* __restrict__ best_kf, float* __restrict__ best_S12, double* __restrict__ best_srt, int32_t* __restrict__ keep_kf,
              double* __restrict__ keep_srt) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseq) return;
    const int best = s3_select_rank(ncand, min_consensus, cand_kf, cand_consensus, s);
    const size_t cb = (size_t)s * ncand + (best >= 0 ? best : 0);
    if (best_rank) best_rank[s] = best;
    if (best_kf) best_kf[s] = best >= 0 ? cand_kf[cb] : -1;
    if (best_S12)
        for (int i = 0; i < 16; i++) best_S12[16 * (size_t)s + i] = best >= 0 ? cand_S12[16 * cb + i] : ((i & 3) == (i >> 2) ? 1.f : 0.f);
    if (best_srt)
        for (int i = 0; i < 8; i++) best_srt[8 * (size_t)s + i] = best >= 0 ? cand_srt[8 * cb + i] : ((i == 0 || i == 7) ? 1.0 : 0.0);
    if (keep_kf) keep_kf[s] = best >= 0 ? cand_kf[cb] : -1;
    if (keep_srt)
        for (int i = 0; i < 8; i++) keep_srt[8 * (size_t)s + i] = best >= 0 ? cand_srt[8 * cb + i] : ((i == 0 || i == 7) ? 1.0 : 0.0);
}

/* ---- the keyframe store's SearchBySim3 query (tb_kf_store_sim3_search_dev) around the operator of k_sim3_search.hip.
 * k_sim3_search_prep, pair c = s * ncand + r (one workgroup each): the pair is skipped (skip[c] = 1) without a candidate or with a
 * consensus below 3; otherwise the camera points of EVERY key of both sides, formed as k_sim3_rows forms X1 and X2, and the
 * `already matched` bytes: the rows of the Sim(3) query's list are walked again by the row rule (row `at` of the list belongs to
 * the at-th key with a winner), and where the RANSAC's mask of that row is 1 the query key and the stored key are matched and
 * wink[i] keeps the index of the row's match in the verification's list, for the merge. The operator reads the query frame at
 * fr1[c] = s and the stored keyframe at fr2[c] = s * cap + slot, in place. */
__global__ void __launch_bounds__(256)
k_sim3_search_prep(int ncand, int cap, const int32_t* __restrict__ cand_slot, const int32_t* __restrict__ kf_ids, const int32_t* __restrict__ q_counts,
                   const float* __restrict__ q_mp, const uint8_t* __restrict__ q_valid, int q_pitch, const float* __restrict__ q_Tcw,
                   const tb_match* __restrict__ matches, const int32_t* __restrict__ match_counts, const float* __restrict__ kf_mp,
                   const uint8_t* __restrict__ kf_valid, const int32_t* __restrict__ kf_counts, const float* __restrict__ kf_Tcw, int pitch,
                   const int32_t* __restrict__ cand_consensus, const uint8_t* __restrict__ inlier, float* __restrict__ pts1,
                   float* __restrict__ pts2, uint8_t* __restrict__ m1, uint8_t* __restrict__ m2, int32_t* __restrict__ wink,
                   int32_t* __restrict__ skip, int32_t* __restrict__ fr1, int32_t* __restrict__ fr2) {
    extern __shared__ int win[];   /* [q_pitch] */
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int s = c / ncand;
    int f, kf;
    s3_pair_frame(c, ncand, cap, cand_slot, kf_ids, f, kf);
    const bool skipped = f < 0 || cand_consensus[c] < 3;
    if (tid == 0) { skip[c] = skipped ? 1 : 0; fr1[c] = s; fr2[c] = f < 0 ? 0 : f; }
    uint8_t* M1 = m1 + (size_t)c * q_pitch;
    uint8_t* M2 = m2 + (size_t)c * pitch;
    int32_t* W = wink + (size_t)c * q_pitch;
    for (int i = tid; i < q_pitch; i += 256) { M1[i] = 0; W[i] = -1; }
    for (int j = tid; j < pitch; j += 256) M2[j] = 0;
    if (skipped) return;
    const int n = min(max(q_counts[s], 0), q_pitch);
    const int nm = min(max(match_counts[c], 0), pitch);
    const int nk = min(max(kf_counts[f], 0), pitch);
    const float* MP1 = q_mp + 3 * (size_t)s * q_pitch;
    const uint8_t* V1 = q_valid + (size_t)s * q_pitch;
    const float* T1 = q_Tcw + 16 * (size_t)s;
    const tb_match* M = matches + (size_t)c * pitch;
    const float* MP2 = kf_mp + 3 * (size_t)f * pitch;
    const uint8_t* V2 = kf_valid + (size_t)f * pitch;
    const float* T2 = kf_Tcw + 16 * (size_t)f;
    const uint8_t* I = inlier + (size_t)c * pitch;
    float* P1 = pts1 + 3 * (size_t)c * q_pitch;
    float* P2 = pts2 + 3 * (size_t)c * pitch;
    for (int i = tid; i < n; i += 256) {
        const float a0 = MP1[3 * i], a1 = MP1[3 * i + 1], a2 = MP1[3 * i + 2];
        P1[3 * i] = s3_apply(T1, 0, a0, a1, a2); P1[3 * i + 1] = s3_apply(T1, 1, a0, a1, a2); P1[3 * i + 2] = s3_apply(T1, 2, a0, a1, a2);
    }
    for (int j = tid; j < nk; j += 256) {
        const float b0 = MP2[3 * j], b1 = MP2[3 * j + 1], b2 = MP2[3 * j + 2];
        P2[3 * j] = s3_apply(T2, 0, b0, b1, b2); P2[3 * j + 1] = s3_apply(T2, 1, b0, b1, b2); P2[3 * j + 2] = s3_apply(T2, 2, b0, b1, b2);
    }
    s3_row_winners(win, n, M, nm, nk, V1, V2);   /* its barriers also order the zeroes above before the ones below */
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const int k = i < n ? win[i] : -1;
        const int at = tb_block_ordered_slot(k >= 0, base, wsum);
        if (k >= 0 && I[at]) { M1[i] = 1; M2[M[k].trainIdx] = 1; W[i] = k; }
    }
}

/* Pair c (one workgroup each), after the operator: the widened match list -- in ascending query key i the match of the RANSAC-inlier
 * row of i (wink[i], copied from the verification's list as it stands) or the new pair of i (the operator's list is in ascending i
 * and, at cap = pitch, never truncated: the n-th new key owns its n-th entry), one entry a key. A skipped pair has none. */
__global__ void __launch_bounds__(256)
k_sim3_search_merge(int ncand, const int32_t* __restrict__ q_counts, int q_pitch, int pitch, const tb_match* __restrict__ matches,
                    const int32_t* __restrict__ wink, const int32_t* __restrict__ skip, const int32_t* __restrict__ match1,
                    const int32_t* __restrict__ match2, const tb_match* __restrict__ pairs, tb_match* __restrict__ wide,
                    int32_t* __restrict__ wide_counts) {
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n = skip[c] ? 0 : min(max(q_counts[c / ncand], 0), q_pitch);
    const tb_match* M = matches + (size_t)c * pitch;
    const tb_match* P = pairs + (size_t)c * pitch;
    const int32_t* W = wink + (size_t)c * q_pitch;
    const int32_t* A = match1 + (size_t)c * q_pitch;
    const int32_t* B = match2 + (size_t)c * pitch;
    tb_match* O = wide + (size_t)c * pitch;
    int fresh = 0, all = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int k = -1;
        bool isnew = false;
        if (i < n) {
            k = W[i];
            if (k < 0) { const int j = A[i]; isnew = j >= 0 && j < pitch && B[j] == i; }
        }
        const int pn = tb_block_ordered_slot(isnew, fresh, wsum);
        const int at = tb_block_ordered_slot(k >= 0 || isnew, all, wsum);
        if (k >= 0) O[at] = M[k];            /* at <= i < q_pitch <= pitch */
        else if (isnew) O[at] = P[pn];
    }
    if (tid == 0) wide_counts[c] = all;
}

/* Per sequence (one 64-thread workgroup each): the per-candidate counts to the caller, and those of the candidate the Sim(3) query
 * selected, by its rule (rank -1, or min_consensus < 0 = it selected nothing: zeros) */
__global__ void __launch_bounds__(64)
k_sim3_search_select(int ncand, int min_consensus, const int32_t* __restrict__ cand_kf, const int32_t* __restrict__ cand_consensus,
                     const int32_t* __restrict__ new_counts, const int32_t* __restrict__ wide_counts, const int32_t* __restrict__ stats,
                     int32_t* __restrict__ o_new, int32_t* __restrict__ o_total, int32_t* __restrict__ o_stats, int32_t* __restrict__ b_new,
                     int32_t* __restrict__ b_total) {
    const int s = blockIdx.x;
    for (int r = threadIdx.x; r < ncand; r += 64) {
        const size_t c = (size_t)s * ncand + r;
        if (o_new) o_new[c] = new_counts[c];
        if (o_total) o_total[c] = wide_counts[c];
        if (o_stats) for (int i = 0; i < 8; i++) o_stats[8 * c + i] = stats[8 * c + i];
    }
    if (threadIdx.x != 0 || (!b_new && !b_total)) return;
    const int best = min_consensus < 0 ? -1 : s3_select_rank(ncand, min_consensus, cand_kf, cand_consensus, s);
    const size_t cb = (size_t)s * ncand + (best >= 0 ? best : 0);
    if (b_new) b_new[s] = best >= 0 ? new_counts[cb] : 0;
    if (b_total) b_total[s] = best >= 0 ? wide_counts[cb] : 0;
}

int tbk_sim3_search_prep(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids,
                         const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch, const float* d_q_Tcw,
                         const tb_match* d_matches, const int32_t* d_match_counts, const float* d_kf_mp, const uint8_t* d_kf_valid,
                         const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch, const int32_t* d_cand_consensus, const uint8_t* d_inlier,
                         float* d_pts1, float* d_pts2, uint8_t* d_m1, uint8_t* d_m2, int32_t* d_wink, int32_t* d_skip, int32_t* d_fr1,
                         int32_t* d_fr2) {
    if (npairs <= 0) return TB_OK;
    return tb_launch(ctx, "k_sim3_search_prep", k_sim3_search_prep, dim3(npairs), dim3(256), (size_t)q_pitch * sizeof(int), ncand, cap, d_cand_slot,
                     d_kf_ids, d_q_counts, d_q_mp, d_q_valid, q_pitch, d_q_Tcw, d_matches, d_match_counts, d_kf_mp, d_kf_valid, d_kf_counts,
                     d_kf_Tcw, pitch, d_cand_consensus, d_inlier, d_pts1, d_pts2, d_m1, d_m2, d_wink, d_skip, d_fr1, d_fr2);
}

int tbk_sim3_search_merge(tb_ctx* ctx, int nseq, int ncand, int min_consensus, const int32_t* d_q_counts, int q_pitch, int pitch,
                          const tb_match* d_matches, const int32_t* d_wink, const int32_t* d_skip, const int32_t* d_match1,
                          const int32_t* d_match2, const tb_match* d_pairs, const int32_t* d_new_counts, const int32_t* d_stats,
                          const int32_t* d_cand_kf, const int32_t* d_cand_consensus, tb_match* d_wide, int32_t* d_wide_counts, int32_t* o_new,
                          int32_t* o_total, int32_t* o_stats, int32_t* b_new, int32_t* b_total) {
    const int npairs = nseq * ncand;
    if (npairs <= 0) return TB_OK;
    TB_TRY(tb_launch(ctx, "k_sim3_search_merge", k_sim3_search_merge, dim3(npairs), dim3(256), 0, ncand, d_q_counts, q_pitch, pitch, d_matches,
                     d_wink, d_skip, d_match1, d_match2, d_pairs, d_wide, d_wide_counts));
    if (!o_new && !o_total && !o_stats && !b_new && !b_total) return TB_OK;
    return tb_launch(ctx, "k_sim3_search_select", k_sim3_search_select, dim3(nseq), dim3(64), 0, ncand, min_consensus, d_cand_kf, d_cand_consensus,
                     d_new_counts, d_wide_counts, d_stats, o_new, o_total, o_stats, b_new, b_total);
}

int tbk_sim3_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_row* d_rows, const int32_t* d_counts, int pitch, int hypotheses,
                   int fixed_scale, double chi2_max, unsigned long long seed, float* d_S12, double* d_srt, int32_t* d_consensus,
                   uint8_t* d_inlier, int32_t* d_winner, int32_t* d_flags) {
    if (nproblems <= 0) return TB_OK;
    return tb_launch(ctx, "k_sim3", k_sim3, dim3(nproblems), dim3(S3_T), 0, K[0], K[1], K[2], K[3], d_rows, d_counts, pitch, hypotheses,
                     fixed_scale, chi2_max, seed, d_S12, d_srt, d_consensus, d_inlier, d_winner, d_flags);
}

template <typename Row>
static int s3_rows_launch(tb_ctx* ctx, const char* name, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids,
                          const tb_keypoint* d_q_keys, const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch,
                          const float* d_q_Tcw, const tb_match* d_matches, const int32_t* d_match_counts, const tb_keypoint* d_kf_keys,
                          const float* d_kf_mp, const uint8_t* d_kf_valid, const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch,
                          const float* inv_sigma2, int nlevels, Row* d_rows, int32_t* d_row_counts, int32_t* d_cand_kf, int32_t* d_rows_out) {
    if (npairs <= 0) return TB_OK;
    tb_sim3_sigma sig;
    sig.n = nlevels;
    for (int i = 0; i < TB_MAX_LEVELS; i++) sig.v[i] = i < nlevels ? inv_sigma2[i] : 0.f;
    return tb_launch(ctx, name, k_sim3_rows<Row>, dim3(npairs), dim3(256), (size_t)q_pitch * sizeof(int), ncand, cap, d_cand_slot, d_kf_ids,
                     d_q_keys, d_q_counts, d_q_mp, d_q_valid, q_pitch, d_q_Tcw, d_matches, d_match_counts, d_kf_keys, d_kf_mp, d_kf_valid,
                     d_kf_counts, d_kf_Tcw, pitch, sig, d_rows, d_row_counts, d_cand_kf, d_rows_out);
}

int tbk_sim3_rows(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids, const tb_keypoint* d_q_keys,
                  const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch, const float* d_q_Tcw,
                  const tb_match* d_matches, const int32_t* d_match_counts, const tb_keypoint* d_kf_keys, const float* d_kf_mp,
                  const uint8_t* d_kf_valid, const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch, const float* inv_sigma2, int nlevels,
                  tb_sim3_row* d_rows, int32_t* d_row_counts, int32_t* d_cand_kf, int32_t* d_rows_out) {
    return s3_rows_launch(ctx, "k_sim3_rows", npairs, ncand, cap, d_cand_slot, d_kf_ids, d_q_keys, d_q_counts, d_q_mp, d_q_valid, q_pitch, d_q_Tcw,
                          d_matches, d_match_counts, d_kf_keys, d_kf_mp, d_kf_valid, d_kf_counts, d_kf_Tcw, pitch, inv_sigma2, nlevels, d_rows,
                          d_row_counts, d_cand_kf, d_rows_out);
}

int tbk_sim3_obs_rows(tb_ctx* ctx, int npairs, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids,
                      const tb_keypoint* d_q_keys, const int32_t* d_q_counts, const float* d_q_mp, const uint8_t* d_q_valid, int q_pitch,
                      const float* d_q_Tcw, const tb_match* d_matches, const int32_t* d_match_counts, const tb_keypoint* d_kf_keys,
                      const float* d_kf_mp, const uint8_t* d_kf_valid, const int32_t* d_kf_counts, const float* d_kf_Tcw, int pitch,
                      const float* inv_sigma2, int nlevels, tb_sim3_obs_row* d_rows, int32_t* d_row_counts, int32_t* d_cand_kf) {
    return s3_rows_launch(ctx, "k_sim3_rows_obs", npairs, ncand, cap, d_cand_slot, d_kf_ids, d_q_keys, d_q_counts, d_q_mp, d_q_valid, q_pitch,
                          d_q_Tcw, d_matches, d_match_counts, d_kf_keys, d_kf_mp, d_kf_valid, d_kf_counts, d_kf_Tcw, pitch, inv_sigma2, nlevels,
                          d_rows, d_row_counts, d_cand_kf, nullptr);
}

/* Per sequence (one 64-thread workgroup each), after the optimiser ran on every pair of tb_kf_store_sim3_refine_dev: a thread
 * hands candidates r, r + 64, ... their four outputs to the caller (a skipped pair -- no candidate, or a consensus below 3 -- ran as an empty problem
 * from the identity and is flagged stats[7] = 2 here); thread 0 finds the candidate the Sim(3) query selected, by its rule, copies
 * its four outputs (rank -1: the identity, zeros, stats[7] = 2) and, with use_for_graph, gives the store's kept best_srt the
 * refined srt where its inliers reach min_inliers. */
__global__ void __launch_bounds__(64)
k_sim3_refine_select(int ncand, int min_consensus, int min_inliers, int use_for_graph, const int32_t* __restrict__ cand_kf,
                     const int32_t* __restrict__ cand_consensus, double* __restrict__ srt, float* __restrict__ S12, int32_t* __restrict__ inl,
                     double* __restrict__ stats, double* __restrict__ o_srt, float* __restrict__ o_S12, int32_t* __restrict__ o_inl,
                     double* __restrict__ o_stats, double* __restrict__ b_srt, float* __restrict__ b_S12, int32_t* __restrict__ b_inl,
                     double* __restrict__ b_stats, double* __restrict__ keep_srt) {
    const int s = blockIdx.x;
    for (int r = threadIdx.x; r < ncand; r += 64) {
        const size_t c = (size_t)s * ncand + r;
        if (cand_kf[c] < 0 || cand_consensus[c] < 3) stats[8 * c + 7] = 2.0;
        if (o_srt) for (int i = 0; i < 8; i++) o_srt[8 * c + i] = srt[8 * c + i];
        if (o_S12) for (int i = 0; i < 16; i++) o_S12[16 * c + i] = S12[16 * c + i];
        if (o_inl) o_inl[c] = inl[c];
        if (o_stats) for (int i = 0; i < 8; i++) o_stats[8 * c + i] = stats[8 * c + i];
    }
    __syncthreads();   /* thread 0 reads flags other threads wrote */
    if (threadIdx.x != 0 || min_consensus < 0) return;   /* min_consensus < 0: the Sim(3) query selected nothing */
    const int best = s3_select_rank(ncand, min_consensus, cand_kf, cand_consensus, s);
    const size_t cb = (size_t)s * ncand + (best >= 0 ? best : 0);
    if (b_srt) for (int i = 0; i < 8; i++) b_srt[8 * (size_t)s + i] = best >= 0 ? srt[8 * cb + i] : ((i == 0 || i == 7) ? 1.0 : 0.0);
    if (b_S12) for (int i = 0; i < 16; i++) b_S12[16 * (size_t)s + i] = best >= 0 ? S12[16 * cb + i] : ((i & 3) == (i >> 2) ? 1.f : 0.f);
    if (b_inl) b_inl[s] = best >= 0 ? inl[cb] : 0;
    if (b_stats) for (int i = 0; i < 8; i++) b_stats[8 * (size_t)s + i] = best >= 0 ? stats[8 * cb + i] : (i == 7 ? 2.0 : 0.0);
    if (use_for_graph && best >= 0 && stats[8 * cb + 7] == 0.0 && inl[cb] >= min_inliers)
        for (int i = 0; i < 8; i++) keep_srt[8 * (size_t)s + i] = srt[8 * cb + i];
}

/* Per pair (one thread each), before the optimiser: a pair without a candidate or with a consensus below 3 becomes an empty problem
 * seeded with the identity; every other pair keeps its row count and takes its cand_srt as the seed */
__global__ void __launch_bounds__(256)
k_sim3_refine_prep(int npairs, const int32_t* __restrict__ cand_kf, const int32_t* __restrict__ cand_consensus, const double* __restrict__ cand_srt,
                   const int32_t* __restrict__ row_counts, int32_t* __restrict__ counts, double* __restrict__ seed) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= npairs) return;
    const bool skip = cand_kf[c] < 0 || cand_consensus[c] < 3;
    counts[c] = skip ? 0 : row_counts[c];
    for (int i = 0; i < 8; i++) seed[8 * (size_t)c + i] = skip ? ((i == 0 || i == 7) ? 1.0 : 0.0) : cand_srt[8 * (size_t)c + i];
}

int tbk_sim3_refine_prep(tb_ctx* ctx, int npairs, const int32_t* d_cand_kf, const int32_t* d_cand_consensus, const double* d_cand_srt,
                         const int32_t* d_row_counts, int32_t* d_counts, double* d_seed) {
    if (npairs <= 0) return TB_OK;
    return tb_launch(ctx, "k_sim3_refine_prep", k_sim3_refine_prep, dim3((npairs + 255) / 256), dim3(256), 0, npairs, d_cand_kf, d_cand_consensus,
                     d_cand_srt, d_row_counts, d_counts, d_seed);
}

int tbk_sim3_refine_select(tb_ctx* ctx, int nseq, int ncand, int min_consensus, int min_inliers, int use_for_graph, const int32_t* d_cand_kf,
                           const int32_t* d_cand_consensus, double* d_srt, float* d_S12, int32_t* d_inl, double* d_stats, double* o_srt,
                           float* o_S12, int32_t* o_inl, double* o_stats, double* b_srt, float* b_S12, int32_t* b_inl, double* b_stats,
                           double* d_keep_srt) {
    return tb_launch(ctx, "k_sim3_refine_select", k_sim3_refine_select, dim3(nseq), dim3(64), 0, ncand, min_consensus, min_inliers, use_for_graph,
                     d_cand_kf, d_cand_consensus, d_srt, d_S12, d_inl, d_stats, o_srt, o_S12, o_inl, o_stats, b_srt, b_S12, b_inl, b_stats,
                     d_keep_srt);
}

int tbk_sim3_select(tb_ctx* ctx, int nseq, int ncand, int min_consensus, const int32_t* d_cand_kf, const int32_t* d_cand_consensus,
                    const float* d_cand_S12, const double* d_cand_srt, int32_t* d_best_rank, int32_t* d_best_kf, float* d_best_S12,
                    double* d_best_srt, int32_t* d_keep_kf, double* d_keep_srt) {
    return tb_launch(ctx, "k_sim3_select", k_sim3_select, dim3((nseq + 255) / 256), dim3(256), 0, nseq, ncand, min_consensus, d_cand_kf,
                     d_cand_consensus, d_cand_S12, d_cand_srt, d_best_rank, d_best_kf, d_best_S12, d_best_srt, d_keep_kf, d_keep_srt);
}
