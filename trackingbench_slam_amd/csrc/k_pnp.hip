/* P3P-RANSAC: a pose from 3D-2D rows without a prior (tb_pnp_ransac_batch_dev, include/tb_capi.h; DESIGN.md 9l has the
 * derivation, tests/pnp_reference.py is the definition, statement for statement).
 *
 * One 256-thread workgroup per problem. Thread t owns the hypotheses t, t + 256, ...: it draws the sample, runs the minimal
 * solver in registers (float64, one operation per statement, only + - * / sqrt and comparisons, fixed loop counts; the library
 * builds with -ffp-contract=off) and keeps the depth triples of its up to four solutions. Each solution in turn becomes a pose
 * (twelve doubles in registers) that the thread scores against every row; the rows sit in LDS as doubles, one chunk of PNP_CHUNK
 * at a time, and all lanes read the same row at once: a broadcast, no bank conflict. A problem of at most one chunk is staged
 * once. A thread's counts and its best (count, hypothesis, solution, pose) stay in its registers: no atomics, no LDS for poses.
 * The winner is one max-reduction over the packed key (count + 1, -hypothesis, -solution); its owner hands the pose over through
 * LDS and every thread writes the mask of the rows it walks, with the arithmetic that counted them.
 *
 * Bound: FP64 VALU (about 40 flop per row and solution, about 2000 per hypothesis for the solver); not HBM. */
#include "tb_internal.h"
#include "tb_device.h"

#define PNP_T 256
#define PNP_CHUNK 256 /* rows per LDS chunk: 12 KiB of doubles */
#define PNP_DRAWS 8
#define PNP_BISECTIONS 80
#define PNP_NEWTONS 2
#define PNP_DBL_MAX 1.7976931348623157e308

__device__ __forceinline__ unsigned long long pnp_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double pnp_dot(const double (&a)[3], const double (&b)[3]) {
    double d = a[0] * b[0];
    d = d + a[1] * b[1];
    return d + a[2] * b[2];
}

__device__ __forceinline__ void pnp_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* adjugate of the symmetric 3 x 3 s = (00, 01, 02, 11, 12, 22), same packing */
__device__ __forceinline__ void pnp_adj(const double (&s)[6], double (&a)[6]) {
    a[0] = s[3] * s[5] - s[4] * s[4];
    a[1] = s[2] * s[4] - s[1] * s[5];
    a[2] = s[1] * s[4] - s[2] * s[3];
    a[3] = s[0] * s[5] - s[2] * s[2];
    a[4] = s[1] * s[2] - s[0] * s[4];
    a[5] = s[0] * s[3] - s[1] * s[1];
}

__device__ __forceinline__ double pnp_det(const double (&s)[6], const double (&a)[6]) {
    double d = s[0] * a[0];
    d = d + s[1] * a[1];
    return d + s[2] * a[2];
}

__device__ __forceinline__ double pnp_trace(const double (&a)[6], const double (&b)[6]) {
    double d = a[0] * b[0];
    d = d + a[3] * b[3];
    d = d + a[5] * b[5];
    double e = a[1] * b[1];
    e = e + a[2] * b[2];
    e = e + a[4] * b[4];
    e = 2.0 * e;
    return d + e;
}

/* a' s b */
__device__ __forceinline__ double pnp_quad(const double (&s)[6], const double (&a)[3], const double (&b)[3]) {
    double r[3];
    r[0] = s[0] * b[0];
    r[0] = r[0] + s[1] * b[1];
    r[0] = r[0] + s[2] * b[2];
    r[1] = s[1] * b[0];
    r[1] = r[1] + s[3] * b[1];
    r[1] = r[1] + s[4] * b[2];
    r[2] = s[2] * b[0];
    r[2] = r[2] + s[4] * b[1];
    r[2] = r[2] + s[5] * b[2];
    return pnp_dot(a, r);
}

__device__ __forceinline__ double pnp_cubic(double g, double p2, double p1, double p0) {
    double f = g + p2;
    f = f * g;
    f = f + p1;
    f = f * g;
    return f + p0;
}

/* d' M_ij d */
__device__ __forceinline__ double pnp_side(double di, double dj, double b) {
    double q = di * di;
    q = q + dj * dj;
    double c = b * di;
    c = c * dj;
    c = 2.0 * c;
    return q - c;
}

/* what of a sample the poses of its solutions are made from */
struct PnpSolved {
    double y[3][3];          /* unit bearings */
    double x0[3];            /* the first world point */
    double g1[3], g2[3], g3[3]; /* rows of X^-1, X = (x1 - x0, x2 - x0, their cross product) */
    double L[4][3];          /* depths of the solutions */
    bool ok[4];
};

/* the minimal solver up to the depths: rows r[i] = (u, v, X, Y, Z) */
__device__ __forceinline__ void pnp_solve(const double (&r)[3][5], double fx, double fy, double cx, double cy, PnpSolved& S) {
    double X[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double bx = (r[i][0] - cx) / fx;
        const double by = (r[i][1] - cy) / fy;
        double nn = bx * bx;
        nn = nn + by * by;
        nn = nn + 1.0;
        nn = sqrt(nn);
        S.y[i][0] = bx / nn;
        S.y[i][1] = by / nn;
        S.y[i][2] = 1.0 / nn;
        X[i][0] = r[i][2]; X[i][1] = r[i][3]; X[i][2] = r[i][4];
    }
    const double b12 = pnp_dot(S.y[0], S.y[1]), b13 = pnp_dot(S.y[0], S.y[2]), b23 = pnp_dot(S.y[1], S.y[2]);
    double e1[3], e2[3], e12[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        e1[k] = X[1][k] - X[0][k];
        e2[k] = X[2][k] - X[0][k];
        e12[k] = X[2][k] - X[1][k];
        S.x0[k] = X[0][k];
    }
    const double a12 = pnp_dot(e1, e1), a13 = pnp_dot(e2, e2), a23 = pnp_dot(e12, e12);
    bool good = a12 > 0.0 && a13 > 0.0 && a23 > 0.0;
    const double D1[6] = {a23, -(b12 * a23), 0.0, a23 - a12, b23 * a12, -a12};
    const double D2[6] = {a23, 0.0, -(b13 * a23), -a13, b23 * a13, a23 - a13};
    double A1[6], A2[6];
    pnp_adj(D1, A1);
    pnp_adj(D2, A2);
    const double c0 = pnp_det(D1, A1), c1 = pnp_trace(A1, D2), c2 = pnp_trace(A2, D1), c3 = pnp_det(D2, A2);
    const double p2 = c2 / c3, p1 = c1 / c3, p0 = c0 / c3;
    double bound = fabs(p2);
    if (fabs(p1) > bound) bound = fabs(p1);
    if (fabs(p0) > bound) bound = fabs(p0);
    bound = bound + 1.0;
    double lo = -bound, hi = bound;
    for (int it = 0; it < PNP_BISECTIONS; it++) {
        double mid = lo + hi;
        mid = 0.5 * mid;
        const bool pos = pnp_cubic(mid, p2, p1, p0) > 0.0;
        hi = pos ? mid : hi;
        lo = pos ? lo : mid;
    }
    double g = lo + hi;
    g = 0.5 * g;
    for (int it = 0; it < PNP_NEWTONS; it++) {
        const double f = pnp_cubic(g, p2, p1, p0);
        double df = 3.0 * g;
        df = df + 2.0 * p2;
        df = df * g;
        df = df + p1;
        const double step = f / df;
        g = (df != 0.0) ? g - step : g;
    }
    double D0[6], B[6];
#pragma unroll
    for (int k = 0; k < 6; k++) D0[k] = D1[k] + g * D2[k];
    pnp_adj(D0, B);
    /* p = l x m from the largest diagonal entry of -adj(D0) */
    double best = -B[0], col[3] = {B[0], B[1], B[2]};
    if (-B[3] > best) { best = -B[3]; col[0] = B[1]; col[1] = B[3]; col[2] = B[4]; }
    if (-B[5] > best) { best = -B[5]; col[0] = B[2]; col[1] = B[4]; col[2] = B[5]; }
    good = good && best > 0.0;
    const double sq = sqrt(best);
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = -(col[k] / sq);
    const double N[3][3] = {{D0[0], D0[1] - p[2], D0[2] + p[1]}, {D0[1] + p[2], D0[3], D0[4] - p[0]}, {D0[2] - p[1], D0[4] + p[0], D0[5]}};
    double big = fabs(N[0][0]);
    double pl[2][3] = {{N[0][0], N[0][1], N[0][2]}, {N[0][0], N[1][0], N[2][0]}}; /* l: the row, m: the column of the largest entry */
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            if (rr == 0 && cc == 0) continue;
            if (fabs(N[rr][cc]) > big) {
                big = fabs(N[rr][cc]);
#pragma unroll
                for (int k = 0; k < 3; k++) { pl[0][k] = N[rr][k]; pl[1][k] = N[k][cc]; }
            }
        }
    /* the pose-independent half of R = Y X^-1 */
    double e3[3];
    pnp_cross(e1, e2, e3);
    pnp_cross(e2, e3, S.g1);
    pnp_cross(e3, e1, S.g2);
    pnp_cross(e1, e2, S.g3);
    const double det = pnp_dot(e1, S.g1);
    good = good && det > 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { S.g1[k] = S.g1[k] / det; S.g2[k] = S.g2[k] / det; S.g3[k] = S.g3[k] / det; }
    double asum = a12 + a13;
    asum = asum + a23;
#pragma unroll
    for (int pi = 0; pi < 2; pi++) {
        const double n0 = pl[pi][0], n1 = pl[pi][1], n2 = pl[pi][2];
        const bool k1 = fabs(n1) > fabs(n0);
        const double top = k1 ? fabs(n1) : fabs(n0);
        const bool k2 = fabs(n2) > top;
        /* n x e0 = (0, n2, -n1), n x e1 = (-n2, 0, n0), n x e2 = (n1, -n0, 0); largest |n_k|: u = n x e_(k+1), w = n x e_(k+2) */
        const double x0[3] = {0.0, n2, -n1}, x1[3] = {-n2, 0.0, n0}, x2[3] = {n1, -n0, 0.0};
        double u[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            u[k] = k2 ? x0[k] : (k1 ? x2[k] : x1[k]);
            w[k] = k2 ? x1[k] : (k1 ? x0[k] : x2[k]);
        }
        const double A = pnp_quad(D1, u, u), Bq = pnp_quad(D1, u, w), Cq = pnp_quad(D1, w, w);
        double disc = Bq * Bq;
        disc = disc - A * Cq;
        const bool real = disc >= 0.0;
        const double rt = sqrt(disc);
        double q = (Bq >= 0.0) ? Bq + rt : Bq - rt;
        q = -q;
#pragma unroll
        for (int ri = 0; ri < 2; ri++) {
            const double sg = ri == 0 ? q : Cq, ta = ri == 0 ? A : q;
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = sg * u[k] + ta * w[k];
            double Q = pnp_side(d[0], d[1], b12) + pnp_side(d[0], d[2], b13);
            Q = Q + pnp_side(d[1], d[2], b23);
            double s = asum / Q;
            s = sqrt(s);
            s = (d[0] < 0.0) ? -s : s;
            const int si = 2 * pi + ri;
#pragma unroll
            for (int k = 0; k < 3; k++) S.L[si][k] = s * d[k];
            S.ok[si] = good && real && S.L[si][0] > 0.0 && S.L[si][1] > 0.0 && S.L[si][2] > 0.0;
        }
    }
}

/* the pose (R row-major in P[0..9), t in P[9..12)) of the depths L; false where an entry is not finite */
__device__ __forceinline__ bool pnp_pose(const PnpSolved& S, const double (&L)[3], double (&P)[12]) {
    double c[3][3], f1[3], f2[3], f3[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) c[i][k] = L[i] * S.y[i][k];
#pragma unroll
    for (int k = 0; k < 3; k++) { f1[k] = c[1][k] - c[0][k]; f2[k] = c[2][k] - c[0][k]; }
    pnp_cross(f1, f2, f3);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double v = f1[i] * S.g1[j];
            v = v + f2[i] * S.g2[j];
            P[3 * i + j] = v + f3[i] * S.g3[j];
            fin = fin && fabs(P[3 * i + j]) <= PNP_DBL_MAX;
        }
        double v = P[3 * i] * S.x0[0];
        v = v + P[3 * i + 1] * S.x0[1];
        v = v + P[3 * i + 2] * S.x0[2];
        P[9 + i] = c[0][i] - v;
        fin = fin && fabs(P[9 + i]) <= PNP_DBL_MAX;
    }
    return fin;
}

/* the inlier rule on one row (u, v, X, Y, Z, inv_sigma2) */
__device__ __forceinline__ bool pnp_inlier(const double (&P)[12], double u, double v, double X, double Y, double Z, double w, double fx,
                                           double fy, double cx, double cy, double chi2_max) {
    double pc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double a = P[3 * i] * X;
        a = a + P[3 * i + 1] * Y;
        a = a + P[3 * i + 2] * Z;
        pc[i] = a + P[9 + i];
    }
    double pu = pc[0] / pc[2];
    pu = fx * pu;
    pu = pu + cx;
    double pv = pc[1] / pc[2];
    pv = fy * pv;
    pv = pv + cy;
    const double du = u - pu, dv = v - pv;
    double e = du * du;
    e = e + dv * dv;
    const double c = e * w;
    return pc[2] > 0.0 && c <= chi2_max;
}

__global__ void __launch_bounds__(PNP_T)
k_pnp(double fx, double fy, double cx, double cy, const tb_obs* __restrict__ obsAll, const int32_t* __restrict__ counts, int obs_pitch,
      int H, double chi2_max, unsigned long long seed, const float* __restrict__ Tcw_prior, float* __restrict__ Tcw_out,
      int32_t* __restrict__ consensus, uint8_t* __restrict__ inlierAll, int32_t* __restrict__ winner, int32_t* __restrict__ flags) {
    __shared__ double rows[PNP_CHUNK][6];
    __shared__ double winP[12];
    __shared__ unsigned long long wkey[PNP_T / TB_WAVE];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[p], 0), obs_pitch);
    const tb_obs* obs = obsAll + (size_t)p * obs_pitch;
    const float* prior = Tcw_prior ? Tcw_prior + 16 * (size_t)p : nullptr;

    unsigned long long bestKey = 0; /* (count + 1) << 16 | (1024 - (h + 1)) << 2 | (3 - s); 0 = nothing */
    double bestP[12];
#pragma unroll
    for (int k = 0; k < 12; k++) bestP[k] = 0.0;

    if (n >= 3) { /* block-uniform */
        const bool resident = n <= PNP_CHUNK;
        auto stage = [&](int base) {
            const int i = base + tid;
            if (tid < PNP_CHUNK && i < n) {
                const tb_obs o = obs[i];
                rows[tid][0] = (double)o.u; rows[tid][1] = (double)o.v; rows[tid][2] = (double)o.X;
                rows[tid][3] = (double)o.Y; rows[tid][4] = (double)o.Z; rows[tid][5] = (double)o.inv_sigma2;
            }
        };
        /* one pass: every thread scores its pose (if it has one) against all rows; called by the whole block */
        auto pass = [&](bool valid, const double (&P)[12], int hh, int s) {
            int cnt = 0;
            for (int base = 0; base < n; base += PNP_CHUNK) {
                if (!resident) {
                    __syncthreads();
                    stage(base);
                    __syncthreads();
                }
                if (valid) {
                    const int m = min(PNP_CHUNK, n - base);
                    for (int i = 0; i < m; i++)
                        cnt += pnp_inlier(P, rows[i][0], rows[i][1], rows[i][2], rows[i][3], rows[i][4], rows[i][5], fx, fy, cx, cy, chi2_max) ? 1 : 0;
                }
            }
            if (valid) {
                const unsigned long long key = ((unsigned long long)(cnt + 1) << 16) | ((unsigned long long)(1024 - hh) << 2) | (unsigned long long)(3 - s);
                if (key > bestKey) {
                    bestKey = key;
#pragma unroll
                    for (int k = 0; k < 12; k++) bestP[k] = P[k];
                }
            }
        };
        if (resident) {
            stage(0);
            __syncthreads();
        }
        if (prior) { /* hypothesis -1, thread 0's */
            double P[12];
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) P[3 * i + j] = (double)prior[4 * i + j];
                P[9 + i] = (double)prior[4 * i + 3];
            }
            pass(tid == 0, P, 0, 0);
        }
        for (int h0 = 0; h0 < H; h0 += PNP_T) {
            const int h = h0 + tid;
            PnpSolved S;
            bool have = h < H;
            if (have) {
                /* draws until three distinct rows or PNP_DRAWS are used up */
                int i0 = -1, i1 = -1, i2 = -1;
                for (int k = 0; k < PNP_DRAWS; k++) {
                    const unsigned long long z = pnp_mix(seed + ((unsigned long long)h * 8ull + (unsigned long long)(k + 1)) * 0x9E3779B97F4A7C15ull);
                    const int d = (int)(((z >> 32) * (unsigned long long)n) >> 32);
                    if (i0 < 0) i0 = d;
                    else if (i1 < 0) { if (d != i0) i1 = d; }
                    else if (i2 < 0) { if (d != i0 && d != i1) i2 = d; }
                }
                have = i2 >= 0;
                if (have) {
                    double r[3][5];
                    const int ix[3] = {i0, i1, i2};
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const tb_obs o = obs[ix[i]];
                        r[i][0] = (double)o.u; r[i][1] = (double)o.v; r[i][2] = (double)o.X; r[i][3] = (double)o.Y; r[i][4] = (double)o.Z;
                    }
                    pnp_solve(r, fx, fy, cx, cy, S);
                }
            }
            for (int s = 0; s < 4; s++) {
                double P[12];
                bool valid = false;
                if (have) {
                    const double L[3] = {s == 0 ? S.L[0][0] : s == 1 ? S.L[1][0] : s == 2 ? S.L[2][0] : S.L[3][0],
                                         s == 0 ? S.L[0][1] : s == 1 ? S.L[1][1] : s == 2 ? S.L[2][1] : S.L[3][1],
                                         s == 0 ? S.L[0][2] : s == 1 ? S.L[1][2] : s == 2 ? S.L[2][2] : S.L[3][2]};
                    const bool ok = s == 0 ? S.ok[0] : s == 1 ? S.ok[1] : s == 2 ? S.ok[2] : S.ok[3];
                    const bool fin = pnp_pose(S, L, P);
                    valid = ok && fin;
                }
                pass(valid, P, h + 1, s);
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
    __syncthreads(); /* the last pass's row reads are done before anything else reuses LDS */
    if (tb_lane() == 0) wkey[tid >> 6] = k;
    __syncthreads();
    unsigned long long win = wkey[0];
#pragma unroll
    for (int w = 1; w < PNP_T / TB_WAVE; w++) win = wkey[w] > win ? wkey[w] : win;
    if (win != 0 && bestKey == win) {
#pragma unroll
        for (int i = 0; i < 12; i++) winP[i] = bestP[i];
    }
    __syncthreads();
    uint8_t* inl = inlierAll ? inlierAll + (size_t)p * obs_pitch : nullptr;
    if (win == 0) { /* void: the prior or the identity, an empty mask */
        if (Tcw_out && tid < 16) Tcw_out[16 * (size_t)p + tid] = prior ? prior[tid] : ((tid % 5) == 0 ? 1.f : 0.f);
        if (inl)
            for (int i = tid; i < obs_pitch; i += PNP_T) inl[i] = 0;
        if (tid == 0) {
            if (consensus) consensus[p] = 0;
            if (winner) { winner[2 * p] = -2; winner[2 * p + 1] = 0; }
            if (flags) flags[p] = 1;
        }
        return;
    }
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; i++) P[i] = winP[i];
    if (Tcw_out && tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = (r == 3) ? (c == 3 ? 1.f : 0.f) : 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (r == i && c == j) v = (float)(j < 3 ? P[3 * i + j] : P[9 + i]);
        Tcw_out[16 * (size_t)p + tid] = v;
    }
    if (inl)
        for (int i = tid; i < obs_pitch; i += PNP_T) {
            bool in = false;
            if (i < n) {
                const tb_obs o = obs[i];
                in = pnp_inlier(P, (double)o.u, (double)o.v, (double)o.X, (double)o.Y, (double)o.Z, (double)o.inv_sigma2, fx, fy, cx, cy, chi2_max);
            }
            inl[i] = in ? 1 : 0;
        }
    if (tid == 0) {
        if (consensus) consensus[p] = (int)(win >> 16) - 1;
        if (winner) { winner[2 * p] = 1024 - (int)((win >> 2) & 0x3fff) - 1; winner[2 * p + 1] = 3 - (int)(win & 3); }
        if (flags) flags[p] = 0;
    }
}

/* ---- PnP inside candidate verification (tb_kf_store_pnp_enable): the rows of pair c (one workgroup each) are gathered, in
 * order, from the pair's original rows into the rows a pose stage runs on.
 *   stage 0, after the RANSAC: a pair whose consensus reaches min_consensus takes the PnP path -- its consensus rows and the PnP
 *            pose as the seed; any other pair keeps every row and the stored seed, which is the verification without PnP
 *   stage 1, expand: a pair on the PnP path takes every original row that is an inlier of its optimised pose (the RANSAC's rule
 *            on the float32 pose); any other pair gets no rows, so the second pose stage leaves it alone
 * The outlier flags of the gathered rows are cleared. */
__global__ void __launch_bounds__(256)
k_pnp_gather(int stage, double fx, double fy, double cx, double cy, double chi2_max, int min_consensus, const tb_obs* __restrict__ rows0,
             const int32_t* __restrict__ cnt0, int pitch, const uint8_t* __restrict__ mask, const int32_t* __restrict__ consensus,
             const float* __restrict__ pose_a, const float* __restrict__ pose_b, uint8_t* __restrict__ took, tb_obs* __restrict__ rows,
             int32_t* __restrict__ cnt, uint8_t* __restrict__ outlier, float* __restrict__ seed, int32_t* __restrict__ rows_out) {
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(cnt0[c], 0), pitch);
    const tb_obs* S = rows0 + (size_t)c * pitch;
    tb_obs* D = rows + (size_t)c * pitch;
    uint8_t* OUT = outlier + (size_t)c * pitch;
    const bool take = stage == 0 ? consensus[c] >= min_consensus : took[c] != 0;
    double P[12];
    if (stage == 1) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) P[3 * i + j] = (double)pose_a[16 * (size_t)c + 4 * i + j];
            P[9 + i] = (double)pose_a[16 * (size_t)c + 4 * i + 3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) P[i] = 0.0;
        if (tid < 16) seed[16 * (size_t)c + tid] = take ? pose_a[16 * (size_t)c + tid] : pose_b[16 * (size_t)c + tid];
        if (tid == 0) took[c] = take ? 1 : 0;
    }
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        tb_obs r = {0, 0, 0, 0, 0, 0};
        if (i < n) {
            r = S[i];
            if (stage == 0) ok = !take || mask[(size_t)c * pitch + i] != 0;
            else ok = take && pnp_inlier(P, (double)r.u, (double)r.v, (double)r.X, (double)r.Y, (double)r.Z, (double)r.inv_sigma2, fx, fy, cx, cy, chi2_max);
            OUT[i] = 0;
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) D[at] = r; /* at <= i < pitch */
    }
    if (tid == 0) { cnt[c] = base; if (rows_out && (stage == 0 || take)) rows_out[c] = base; }
}

/* After the second pose stage: a pair on the PnP path adopts its rows, flags, pose and inlier count; any other pair keeps
 * what the first pose stage left. */
__global__ void __launch_bounds__(256)
k_pnp_adopt(const uint8_t* __restrict__ took, int pitch, const tb_obs* __restrict__ rows2, const int32_t* __restrict__ cnt2,
            const uint8_t* __restrict__ outlier2, const float* __restrict__ pose2, const int32_t* __restrict__ ninl2, tb_obs* __restrict__ rows,
            int32_t* __restrict__ cnt, uint8_t* __restrict__ outlier, float* __restrict__ pose, int32_t* __restrict__ ninl) {
    const int c = blockIdx.x, tid = threadIdx.x;
    if (!took[c]) return;
    const int n = min(max(cnt2[c], 0), pitch);
    for (int i = tid; i < n; i += 256) {
        rows[(size_t)c * pitch + i] = rows2[(size_t)c * pitch + i];
        outlier[(size_t)c * pitch + i] = outlier2[(size_t)c * pitch + i];
    }
    if (tid < 16) pose[16 * (size_t)c + tid] = pose2[16 * (size_t)c + tid];
    if (tid == 0) { cnt[c] = n; ninl[c] = ninl2[c]; }
}

int tbk_pnp_gather(tb_ctx* ctx, int npairs, int stage, const double K[4], double chi2_max, int min_consensus, const tb_obs* d_rows0,
                   const int32_t* d_cnt0, int pitch, const uint8_t* d_mask, const int32_t* d_consensus, const float* d_pose_a,
                   const float* d_pose_b, uint8_t* d_took, tb_obs* d_rows, int32_t* d_cnt, uint8_t* d_outlier, float* d_seed,
                   int32_t* d_rows_out) {
    if (npairs <= 0) return TB_OK;
    return tb_launch(ctx, "k_pnp_gather", k_pnp_gather, dim3(npairs), dim3(256), 0, stage, K[0], K[1], K[2], K[3], chi2_max, min_consensus,
                     d_rows0, d_cnt0, pitch, d_mask, d_consensus, d_pose_a, d_pose_b, d_took, d_rows, d_cnt, d_outlier, d_seed, d_rows_out);
}

int tbk_pnp_adopt(tb_ctx* ctx, int npairs, const uint8_t* d_took, int pitch, const tb_obs* d_rows2, const int32_t* d_cnt2,
                  const uint8_t* d_outlier2, const float* d_pose2, const int32_t* d_ninl2, tb_obs* d_rows, int32_t* d_cnt, uint8_t* d_outlier,
                  float* d_pose, int32_t* d_ninl) {
    if (npairs <= 0) return TB_OK;
    return tb_launch(ctx, "k_pnp_adopt", k_pnp_adopt, dim3(npairs), dim3(256), 0, d_took, pitch, d_rows2, d_cnt2, d_outlier2, d_pose2, d_ninl2,
                     d_rows, d_cnt, d_outlier, d_pose, d_ninl);
}

int tbk_pnp_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_obs* d_obs, const int32_t* d_counts, int obs_pitch, int hypotheses,
                  double chi2_max, unsigned long long seed, const float* d_Tcw_prior, float* d_Tcw_out, int32_t* d_consensus,
                  uint8_t* d_inlier, int32_t* d_winner, int32_t* d_flags) {
    if (nproblems <= 0) return TB_OK;
    return tb_launch(ctx, "k_pnp", k_pnp, dim3(nproblems), dim3(PNP_T), 0, K[0], K[1], K[2], K[3], d_obs, d_counts, obs_pitch, hypotheses,
                     chi2_max, seed, d_Tcw_prior, d_Tcw_out, d_consensus, d_inlier, d_winner, d_flags);
}
