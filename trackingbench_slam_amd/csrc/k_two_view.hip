/* Two-view initialisation: a relative pose and first points from 2D-2D rows alone (tb_two_view_batch_dev, include/tb_capi.h;
 * DESIGN.md 9m has the derivation, tests/two_view_reference.py is the definition, statement for statement).
 *
 * One 256-thread workgroup per problem, one launch, no work buffer. The candidate rows (below the count, not skipped) are
 * compacted in index order into dynamic LDS once: 29 bytes per row of the pitch (4 + 2 floats, index, flags), at most 4096
 * rows. Then
 *   RANSAC     thread t owns the hypotheses t, t + 256, ...: it draws eight distinct candidates, solves the 8 x 9 epipolar system
 *              in registers (Gauss-Jordan with partial pivoting; every index is a compile-time constant after unrolling, the row
 *              swaps are selects), turns E into F and scores it against every row from LDS -- all lanes read the same row at
 *              once, a broadcast. Counts and the best (count, hypothesis, E) stay in registers; the winner is one max-reduction
 *              over the packed key, as in k_pnp
 *   refit      lanes are rows: 45 running sums per thread, a butterfly over the 256 threads, then the 9 x 9 Jacobi in LDS, nine
 *              lanes per phase of a rotation
 *   decompose  every thread, redundantly, in registers (3 x 3 Jacobi)
 *   cheirality lanes are rows: four triangulations with tb_triangulate.h's per-point code, integer counts
 *   outputs    the decision is every thread's; the flags under the chosen candidate were kept (3 bits a candidate), an accepted
 *              row is triangulated once more for its point
 * float64, one operation per statement, only + - * / sqrt and comparisons, fixed loop counts (the library builds with
 * -ffp-contract=off).
 *
 * Expected bound: FP64 VALU (about 45 flop and 6 float -> double conversions per row and hypothesis), not HBM. This is by
 * construction, not by measurement: how the time splits between the RANSAC and the stages behind it has not been measured, and
 * staging the rows as doubles (48 bytes a row) to drop the conversions waits for that. */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_triangulate.h"

#define TV_T 256
#define TV_ROW_BYTES 29 /* dynamic LDS per row of the pitch: 4 + 2 floats, two shorts, a byte */
#define TV_DRAWS 16
#define TV_REFIT_SWEEPS 5
#define TV_DECOMP_SWEEPS 6
#define TV_DBL_MAX 1.7976931348623157e308

struct TvParams {
    int hypotheses, refit, min_points;
    double chi2_epi, cos_parallax_max, chi2_max, min_good_ratio, ambiguity_ratio, baseline;
    unsigned long long seed;
};

__device__ __forceinline__ unsigned long long tv_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* the row of the epipolar system of one normalised point pair */
__device__ __forceinline__ void tv_epipolar_row(double x0, double y0, double x1, double y1, double (&a)[9]) {
    a[0] = x1 * x0; a[1] = x1 * y0; a[2] = x1;
    a[3] = y1 * x0; a[4] = y1 * y0; a[5] = y1;
    a[6] = x0; a[7] = y0; a[8] = 1.0;
}

/* the null vector of the 8 x 9 system of eight point pairs; false where the system does not have exactly one free column or
 * the vector is not finite */
__device__ __forceinline__ bool tv_solve8(const double (&x0)[8], const double (&y0)[8], const double (&x1)[8], const double (&y1)[8],
                                          double (&e)[9]) {
    double A[8][9];
#pragma unroll
    for (int i = 0; i < 8; i++) tv_epipolar_row(x0[i], y0[i], x1[i], y1[i], A[i]);
    unsigned used = 0;
    int pivcol[8], nfree = 0, freecol = -1;
#pragma unroll
    for (int r = 0; r < 8; r++) pivcol[r] = -1;
#pragma unroll
    for (int col = 0; col < 9; col++) {
        double bv = -1.0;
        int best = -1;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const double a = fabs(A[r][col]);
            const bool more = !((used >> r) & 1u) && a > bv;
            bv = more ? a : bv;
            best = more ? r : best;
        }
        double scale = 0.0;
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int k = col; k < 9; k++) {
                const double a = fabs(A[r][k]);
                const bool more = !((used >> r) & 1u) && a > scale;
                scale = more ? a : scale;
            }
        const double thr = 1e-12 * scale;
        const bool piv = bv > thr;
        nfree += piv ? 0 : 1;
        freecol = piv ? freecol : col;
        double prow[9];
#pragma unroll
        for (int k = 0; k < 9; k++) prow[k] = 0.0;
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int k = 0; k < 9; k++) prow[k] = best == r ? A[r][k] : prow[k];
        double pc = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) pc = k == col ? prow[k] : pc;
        const double inv = 1.0 / pc;
#pragma unroll
        for (int k = 0; k < 9; k++) prow[k] = prow[k] * inv;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const bool isb = piv && best == r;
            const double f = A[r][col];
            const bool doit = piv && !isb && f != 0.0;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const double t = f * prow[k];
                const double v = A[r][k] - t;
                A[r][k] = isb ? prow[k] : (doit ? v : A[r][k]);
            }
            used |= isb ? (1u << r) : 0u;
            pivcol[r] = isb ? col : pivcol[r];
        }
    }
    bool ok = nfree == 1;
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = freecol == k ? 1.0 : 0.0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) v = freecol == k ? A[r][k] : v;
        v = -v;
#pragma unroll
        for (int k = 0; k < 9; k++) e[k] = pivcol[r] == k ? v : e[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && fabs(e[k]) <= TV_DBL_MAX;
    return ok;
}

/* F = K^-T E K^-1, row-major */
__device__ __forceinline__ void tv_fundamental(const double (&E)[9], double fx, double fy, double cx, double cy, double (&F)[9]) {
    double G[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double g0 = E[3 * i] / fx;
        const double g1 = E[3 * i + 1] / fy;
        const double t = g0 * cx;
        const double u = g1 * cy;
        double g2 = E[3 * i + 2] - t;
        g2 = g2 - u;
        G[i][0] = g0; G[i][1] = g1; G[i][2] = g2;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double f0 = G[0][j] / fx;
        const double f1 = G[1][j] / fy;
        const double t = f0 * cx;
        const double u = f1 * cy;
        double f2 = G[2][j] - t;
        f2 = f2 - u;
        F[j] = f0; F[3 + j] = f1; F[6 + j] = f2;
    }
}

/* the consensus rule on one row */
__device__ __forceinline__ bool tv_inlier(const double (&F)[9], double u0, double v0, double u1, double v1, double w0, double w1,
                                          double chi2_epi) {
    double a = F[0] * u0;
    a = a + F[1] * v0;
    a = a + F[2];
    double b = F[3] * u0;
    b = b + F[4] * v0;
    b = b + F[5];
    double c = F[6] * u0;
    c = c + F[7] * v0;
    c = c + F[8];
    double d = u1 * a;
    d = d + v1 * b;
    d = d + c;
    const double dd = d * d;
    double s = a * a;
    s = s + b * b;
    double e1 = dd / s;
    e1 = e1 * w1;
    a = F[0] * u1;
    a = a + F[3] * v1;
    a = a + F[6];
    b = F[1] * u1;
    b = b + F[4] * v1;
    b = b + F[7];
    s = a * a;
    s = s + b * b;
    double e0 = dd / s;
    e0 = e0 * w0;
    return e1 <= chi2_epi && e0 <= chi2_epi;
}

/* the triangulation's rotation: c and s of the pair whose entries are mpp, mqq, mpq != 0 */
__device__ __forceinline__ void tv_givens(double mpp, double mqq, double mpq, double& c, double& s) {
    const double num = mqq - mpp;
    const double den = 2.0 * mpq;
    const double th = num / den;
    double r = th * th;
    r = r + 1.0;
    r = sqrt(r);
    r = fabs(th) + r;
    const double t = (th >= 0.0 ? 1.0 : -1.0) / r;
    c = t * t;
    c = c + 1.0;
    c = sqrt(c);
    c = 1.0 / c;
    s = t * c;
}

__device__ __forceinline__ void tv_rot(double& a, double& b, double c, double s) {
    const double ca = c * a, sb = s * b, sa = s * a, cb = c * b;
    a = ca - sb;
    b = sa + cb;
}

template <int P, int Q>
__device__ __forceinline__ void tv_rotate3(double (&M)[3][3], double (&V)[3][3]) {
    if (M[P][Q] == 0.0) return;
    double c, s;
    tv_givens(M[P][P], M[Q][Q], M[P][Q], c, s);
#pragma unroll
    for (int k = 0; k < 3; k++) tv_rot(M[k][P], M[k][Q], c, s);
#pragma unroll
    for (int k = 0; k < 3; k++) tv_rot(M[P][k], M[Q][k], c, s);
#pragma unroll
    for (int k = 0; k < 3; k++) tv_rot(V[k][P], V[k][Q], c, s);
}

__device__ __forceinline__ void tv_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* the two rotations and u3 of E */
__device__ __forceinline__ void tv_decompose(const double (&E)[9], double (&Ra)[3][3], double (&Rb)[3][3], double (&u3)[3]) {
    double M[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            double m = E[i] * E[j];
            m = m + E[3 + i] * E[3 + j];
            m = m + E[6 + i] * E[6 + j];
            M[i][j] = m;
            M[j][i] = m;
            V[i][j] = i == j ? 1.0 : 0.0;
            V[j][i] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < TV_DECOMP_SWEEPS; sweep++) {
        tv_rotate3<0, 1>(M, V);
        tv_rotate3<0, 2>(M, V);
        tv_rotate3<1, 2>(M, V);
    }
    double best = M[0][0];
    int k3 = 0;
    if (M[1][1] < best) { best = M[1][1]; k3 = 1; }
    if (M[2][2] < best) { best = M[2][2]; k3 = 2; }
    const double l1 = k3 == 0 ? M[1][1] : M[0][0], l2 = k3 == 2 ? M[1][1] : M[2][2];
    const double s1 = sqrt(l1), s2 = sqrt(l2);
    double v1[3], v2[3], u1[3], u2[3], v3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v1[k] = k3 == 0 ? V[k][1] : V[k][0];
        v2[k] = k3 == 2 ? V[k][1] : V[k][2];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double a = E[3 * r] * v1[0];
        a = a + E[3 * r + 1] * v1[1];
        a = a + E[3 * r + 2] * v1[2];
        u1[r] = a / s1;
        a = E[3 * r] * v2[0];
        a = a + E[3 * r + 1] * v2[1];
        a = a + E[3 * r + 2] * v2[2];
        u2[r] = a / s2;
    }
    tv_cross(u1, u2, u3);
    tv_cross(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double a = u2[i] * v1[j];
            const double b = u1[i] * v2[j];
            const double c = u3[i] * v3[j];
            double d = a - b;
            Ra[i][j] = d + c;
            d = b - a;
            Rb[i][j] = d + c;
        }
}

__global__ void __launch_bounds__(TV_T)
k_two_view(const float* __restrict__ xy0All, const float* __restrict__ xy1All, const int32_t* __restrict__ counts,
           const uint8_t* __restrict__ skipAll, const float* __restrict__ w0All, const float* __restrict__ w1All, int pitch, double fx,
           double fy, double cx, double cy, const float* __restrict__ Tcw0All, TvParams P, float* __restrict__ Tcw1, float* __restrict__ points,
           uint8_t* __restrict__ point_flags, uint8_t* __restrict__ inlierOut, int32_t* __restrict__ consensusOut, int32_t* __restrict__ winner,
           int32_t* __restrict__ goodOut, int32_t* __restrict__ triOut, int32_t* __restrict__ statusOut) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_smem[];   /* TV_ROW_BYTES * pitch */
    float (*rows)[4] = reinterpret_cast<float (*)[4]>(tv_smem);                                  /* u0, v0, u1, v1 of candidate c */
    float (*wts)[2] = reinterpret_cast<float (*)[2]>(tv_smem + 16 * (size_t)pitch);              /* inv_sigma2 in view 0 / view 1 */
    unsigned short* ids = reinterpret_cast<unsigned short*>(tv_smem + 24 * (size_t)pitch);       /* the candidate's row */
    /* by candidate: bit 0 = in the consensus, bits 1 + 3 c .. 3 + 3 c = the triangulation's flag under candidate pose c */
    unsigned short* mask = reinterpret_cast<unsigned short*>(tv_smem + 26 * (size_t)pitch);
    uint8_t* byrow = tv_smem + 28 * (size_t)pitch;   /* by row: 0 = not in the consensus, else 0x80 | the flag under c* */
    __shared__ double red[TV_T / TB_WAVE][45];
    __shared__ double Ms[9][9], Vs[9][9];
    __shared__ double winE[9];
    __shared__ unsigned long long wkey[TV_T / TB_WAVE];
    __shared__ int wsum[4];
    __shared__ int cnts[TV_T / TB_WAVE][9];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t po = (size_t)p * pitch;
    const float* xy0 = xy0All + 2 * po;
    const float* xy1 = xy1All + 2 * po;
    const int nrow = counts ? min(max(counts[p], 0), pitch) : pitch;

    /* the candidates, in index order (a slot never exceeds its row: below the pitch the LDS was sized for) */
    int n = 0;
    for (int i0 = 0; i0 < nrow; i0 += TV_T) {
        const int i = i0 + tid;
        const bool v = i < nrow && !(skipAll && skipAll[po + i]);
        const int k = tb_block_ordered_slot(v, n, wsum);
        if (v) {
            rows[k][0] = xy0[2 * i]; rows[k][1] = xy0[2 * i + 1]; rows[k][2] = xy1[2 * i]; rows[k][3] = xy1[2 * i + 1];
            wts[k][0] = w0All ? w0All[po + i] : 1.f;
            wts[k][1] = w1All ? w1All[po + i] : 1.f;
            ids[k] = (unsigned short)i;
        }
    }
    for (int i = tid; i < pitch; i += TV_T) byrow[i] = 0;
    __syncthreads();

    unsigned long long bestKey = 0; /* (count + 1) << 16 | (1024 - h); 0 = nothing */
    double bestE[9];
#pragma unroll
    for (int k = 0; k < 9; k++) bestE[k] = 0.0;
    if (n >= 8) { /* block-uniform */
        for (int h0 = 0; h0 < P.hypotheses; h0 += TV_T) {
            const int h = h0 + tid;
            bool valid = h < P.hypotheses;
            double E[9], F[9];
            if (valid) {
                int idx[8], cnt = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) idx[j] = -1;
                for (int k = 0; k < TV_DRAWS; k++) {
                    const unsigned long long z =
                        tv_mix(P.seed + ((unsigned long long)h * TV_DRAWS + (unsigned long long)(k + 1)) * 0x9E3779B97F4A7C15ull);
                    const int d = (int)(((z >> 32) * (unsigned long long)n) >> 32);
                    bool dup = false;
#pragma unroll
                    for (int j = 0; j < 8; j++) dup = dup || idx[j] == d;
                    const bool take = !dup && cnt < 8;
#pragma unroll
                    for (int j = 0; j < 8; j++) idx[j] = (take && cnt == j) ? d : idx[j];
                    cnt += take ? 1 : 0;
                }
                valid = cnt == 8;
                if (valid) {
                    double x0[8], y0[8], x1[8], y1[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int c = idx[j]; /* 0 <= c < n */
                        x0[j] = (double)rows[c][0] - cx;
                        x0[j] = x0[j] / fx;
                        y0[j] = (double)rows[c][1] - cy;
                        y0[j] = y0[j] / fy;
                        x1[j] = (double)rows[c][2] - cx;
                        x1[j] = x1[j] / fx;
                        y1[j] = (double)rows[c][3] - cy;
                        y1[j] = y1[j] / fy;
                    }
                    valid = tv_solve8(x0, y0, x1, y1, E);
                }
            }
            if (valid) {
                tv_fundamental(E, fx, fy, cx, cy, F);
                int cnt = 0;
                for (int i = 0; i < n; i++)
                    cnt += tv_inlier(F, (double)rows[i][0], (double)rows[i][1], (double)rows[i][2], (double)rows[i][3], (double)wts[i][0],
                                     (double)wts[i][1], P.chi2_epi) ? 1 : 0;
                const unsigned long long key = ((unsigned long long)(cnt + 1) << 16) | (unsigned long long)(1024 - h);
                if (key > bestKey) {
                    bestKey = key;
#pragma unroll
                    for (int k = 0; k < 9; k++) bestE[k] = E[k];
                }
            }
        }
    }
    /* the winner: max of the keys, which are distinct wherever they are not 0 */
    unsigned long long kk = bestKey;
#pragma unroll
    for (int d = TB_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(kk, d, TB_WAVE);
        kk = o > kk ? o : kk;
    }
    if (lane == 0) wkey[wave] = kk;
    __syncthreads();
    unsigned long long win = wkey[0];
#pragma unroll
    for (int w = 1; w < TV_T / TB_WAVE; w++) win = wkey[w] > win ? wkey[w] : win;
    if (win != 0 && bestKey == win) {
#pragma unroll
        for (int i = 0; i < 9; i++) winE[i] = bestE[i];
    }
    __syncthreads();

    double T0[16];
#pragma unroll
    for (int k = 0; k < 16; k++) T0[k] = Tcw0All ? (double)Tcw0All[16 * (size_t)p + k] : ((k % 5) == 0 ? 1.0 : 0.0);
    auto pose_as_given = [&]() {
        if (Tcw1 && tid < 16) Tcw1[16 * (size_t)p + tid] = Tcw0All ? Tcw0All[16 * (size_t)p + tid] : ((tid % 5) == 0 ? 1.f : 0.f);
    };
    if (win == 0) { /* void */
        pose_as_given();
        for (int i = tid; i < pitch; i += TV_T) {
            if (inlierOut) inlierOut[po + i] = 0;
            if (point_flags) point_flags[po + i] = 0;
        }
        if (tid < 4) {
            if (goodOut) goodOut[4 * p + tid] = 0;
            if (triOut) triOut[4 * p + tid] = 0;
        }
        if (tid == 0) {
            if (consensusOut) consensusOut[p] = 0;
            if (winner) { winner[2 * p] = -1; winner[2 * p + 1] = -1; }
            if (statusOut) statusOut[p] = 1;
        }
        return;
    }
    double E[9], F[9];
#pragma unroll
    for (int i = 0; i < 9; i++) E[i] = winE[i];
    tv_fundamental(E, fx, fy, cx, cy, F);

    if (P.refit) { /* block-uniform */
        double acc[45];
#pragma unroll
        for (int e = 0; e < 45; e++) acc[e] = 0.0;
        for (int c = tid; c < n; c += TV_T) {
            const double u0 = (double)rows[c][0], v0 = (double)rows[c][1], u1 = (double)rows[c][2], v1 = (double)rows[c][3];
            const bool in = tv_inlier(F, u0, v0, u1, v1, (double)wts[c][0], (double)wts[c][1], P.chi2_epi);
            double x0 = u0 - cx, y0 = v0 - cy, x1 = u1 - cx, y1 = v1 - cy;
            x0 = x0 / fx; y0 = y0 / fy; x1 = x1 / fx; y1 = y1 / fy;
            double a[9];
            tv_epipolar_row(x0, y0, x1, y1, a);
            int e = 0;
#pragma unroll
            for (int i = 0; i < 9; i++)
#pragma unroll
                for (int j = i; j < 9; j++, e++) {
                    const double prod = a[i] * a[j];
                    acc[e] = acc[e] + (in ? prod : 0.0);
                }
        }
#pragma unroll
        for (int e = 0; e < 45; e++) {
#pragma unroll
            for (int d = 1; d < TB_WAVE; d <<= 1) acc[e] = acc[e] + __shfl_xor(acc[e], d, TB_WAVE);
            if (lane == 0) red[wave][e] = acc[e];
        }
        __syncthreads();
        if (tid < 81) {
            const int i = tid / 9, j = tid % 9, lo = min(i, j), hi = max(i, j);
            const int e = 9 * lo - (lo * (lo - 1)) / 2 + (hi - lo);
            const double s01 = red[0][e] + red[1][e], s23 = red[2][e] + red[3][e];
            Ms[i][j] = s01 + s23;
            Vs[i][j] = i == j ? 1.0 : 0.0;
        }
        for (int sweep = 0; sweep < TV_REFIT_SWEEPS; sweep++)
            for (int pp = 0; pp < 8; pp++)
                for (int q = pp + 1; q < 9; q++) {
                    __syncthreads();
                    const double mpq = Ms[pp][q];
                    if (mpq == 0.0) continue; /* block-uniform */
                    double c, s;
                    tv_givens(Ms[pp][pp], Ms[q][q], mpq, c, s);
                    __syncthreads();
                    if (tid < 9) tv_rot(Ms[tid][pp], Ms[tid][q], c, s);
                    else if (tid >= TB_WAVE && tid < TB_WAVE + 9) tv_rot(Vs[tid - TB_WAVE][pp], Vs[tid - TB_WAVE][q], c, s);
                    __syncthreads();
                    if (tid < 9) tv_rot(Ms[pp][tid], Ms[q][tid], c, s);
                }
        __syncthreads();
        double best = Ms[0][0];
        int kmin = 0;
        for (int i = 1; i < 9; i++)
            if (Ms[i][i] < best) { best = Ms[i][i]; kmin = i; }
#pragma unroll
        for (int i = 0; i < 9; i++) E[i] = Vs[i][kmin];
        tv_fundamental(E, fx, fy, cx, cy, F);
    }

    /* the consensus of the E that is decomposed */
    int mine[9];
#pragma unroll
    for (int k = 0; k < 9; k++) mine[k] = 0;
    for (int c = tid; c < n; c += TV_T) {
        const bool in = tv_inlier(F, (double)rows[c][0], (double)rows[c][1], (double)rows[c][2], (double)rows[c][3], (double)wts[c][0],
                                  (double)wts[c][1], P.chi2_epi);
        mask[c] = in ? 1 : 0; /* read back by this thread only */
        mine[8] += in ? 1 : 0;
    }

    double Ra[3][3], Rb[3][3], u3[3];
    tv_decompose(E, Ra, Rb, u3);
    const double I4[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    auto candidate = [&](int cnd, double (&T1)[16]) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) T1[4 * i + j] = cnd >= 2 ? Rb[i][j] : Ra[i][j];
            T1[4 * i + 3] = (cnd & 1) ? -u3[i] : u3[i];
        }
        T1[12] = 0.0; T1[13] = 0.0; T1[14] = 0.0; T1[15] = 1.0;
    };
#pragma unroll 1
    for (int cnd = 0; cnd < 4; cnd++) {
        double T1[16];
        candidate(cnd, T1);
        int g = 0, t = 0;
        for (int c = tid; c < n; c += TV_T) {
            if (!(mask[c] & 1)) continue;
            float Xf, Yf, Zf;
            const int flag = tri_point(I4, T1, (double)rows[c][0], (double)rows[c][1], (double)rows[c][2], (double)rows[c][3],
                                       (double)wts[c][0], (double)wts[c][1], fx, fy, cx, cy, P.cos_parallax_max, P.chi2_max, Xf, Yf, Zf);
            mask[c] = (unsigned short)(mask[c] | (flag << (1 + 3 * cnd)));
            g += (flag == 1 || flag == 4) ? 1 : 0;
            t += flag == 1 ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            mine[k] = cnd == k ? g : mine[k];
            mine[4 + k] = cnd == k ? t : mine[4 + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int s = tb_wave_sum(mine[k]);
        if (lane == 0) cnts[wave][k] = s;
    }
    __syncthreads();
    int good[4], tri[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        good[k] = cnts[0][k] + cnts[1][k] + cnts[2][k] + cnts[3][k];
        tri[k] = cnts[0][4 + k] + cnts[1][4 + k] + cnts[2][4 + k] + cnts[3][4 + k];
    }
    const int consensus = cnts[0][8] + cnts[1][8] + cnts[2][8] + cnts[3][8];

    /* the decision */
    int cs = 0, gs = good[0], ts = tri[0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (good[k] > gs) { gs = good[k]; ts = tri[k]; cs = k; }
    const double need = P.min_good_ratio * (double)consensus;
    const double rival = P.ambiguity_ratio * (double)gs;
    bool ambiguous = false;
#pragma unroll
    for (int k = 0; k < 4; k++) ambiguous = ambiguous || (k != cs && (double)good[k] > rival);
    int status = 0;
    if (gs < P.min_points || (double)gs < need) status = 2;
    else if (ambiguous) status = 3;
    else if (ts < P.min_points) status = 4;

    /* the flags under the chosen candidate are the cheirality pass's; only an accepted row of an accepted problem is
     * triangulated once more, for its point */
    double T1[16];
    candidate(cs, T1);
    float* pts = points ? points + 3 * po : nullptr;
    for (int c = tid; c < n; c += TV_T) {
        const int m = mask[c];
        if (!(m & 1)) continue;
        const int flag = (m >> (1 + 3 * cs)) & 7;
        const int i = ids[c];
        byrow[i] = (uint8_t)(0x80 | flag);
        if (pts && status == 0 && flag == 1) {
            float Xf, Yf, Zf;
            tri_point(I4, T1, (double)rows[c][0], (double)rows[c][1], (double)rows[c][2], (double)rows[c][3], (double)wts[c][0],
                      (double)wts[c][1], fx, fy, cx, cy, P.cos_parallax_max, P.chi2_max, Xf, Yf, Zf);
            const double X[3] = {(double)Xf, (double)Yf, (double)Zf};
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double a = P.baseline * X[k];
                d[k] = a - T0[4 * k + 3];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double a = T0[k] * d[0];
                a = a + T0[4 + k] * d[1];
                a = a + T0[8 + k] * d[2];
                pts[3 * i + k] = (float)a;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < pitch; i += TV_T) {
        const uint8_t b = byrow[i];
        if (inlierOut) inlierOut[po + i] = b ? 1 : 0;
        if (point_flags) point_flags[po + i] = b & 0x7f;
    }
    if (status != 0) pose_as_given();
    else if (Tcw1 && tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = (r == 3 && c == 3) ? 1.f : 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (r == i && c == j) {
                    double a = T1[4 * i] * T0[j];
                    a = a + T1[4 * i + 1] * T0[4 + j];
                    a = a + T1[4 * i + 2] * T0[8 + j];
                    if (j == 3) {
                        const double bt = P.baseline * T1[4 * i + 3];
                        a = a + bt;
                    }
                    v = (float)a;
                }
        Tcw1[16 * (size_t)p + tid] = v;
    }
    if (tid < 4) {
        if (goodOut) goodOut[4 * p + tid] = tid == 0 ? good[0] : tid == 1 ? good[1] : tid == 2 ? good[2] : good[3];
        if (triOut) triOut[4 * p + tid] = tid == 0 ? tri[0] : tid == 1 ? tri[1] : tid == 2 ? tri[2] : tri[3];
    }
    if (tid == 0) {
        if (consensusOut) consensusOut[p] = consensus;
        if (winner) { winner[2 * p] = 1024 - (int)(win & 0xffff); winner[2 * p + 1] = cs; }
        if (statusOut) statusOut[p] = status;
    }
}

int tbk_two_view(tb_ctx* ctx, int nproblems, const float* d_xy0, const float* d_xy1, const int32_t* d_counts, const uint8_t* d_skip,
                 const float* d_inv_sigma2_0, const float* d_inv_sigma2_1, int pitch, const double K[4], const float* d_Tcw0,
                 const tb_two_view_params* prm, float* d_Tcw1, float* d_points, uint8_t* d_point_flags, uint8_t* d_inlier,
                 int32_t* d_consensus, int32_t* d_winner, int32_t* d_good, int32_t* d_tri, int32_t* d_status) {
    if (nproblems <= 0) return TB_OK;
    TvParams P;
    P.hypotheses = prm->hypotheses; P.refit = prm->refit; P.min_points = prm->min_points;
    P.chi2_epi = prm->chi2_epi; P.cos_parallax_max = prm->tri.cos_parallax_max; P.chi2_max = prm->tri.chi2_max;
    P.min_good_ratio = prm->min_good_ratio; P.ambiguity_ratio = prm->ambiguity_ratio; P.baseline = prm->baseline;
    P.seed = prm->seed;
    const size_t lds = ((size_t)TV_ROW_BYTES * pitch + 15) & ~(size_t)15;
    TB_TRY(tb_lds_limit(ctx, (const void*)k_two_view, lds));
    return tb_launch(ctx, "k_two_view", k_two_view, dim3(nproblems), dim3(TV_T), lds, d_xy0, d_xy1, d_counts, d_skip, d_inv_sigma2_0,
                     d_inv_sigma2_1, pitch, K[0], K[1], K[2], K[3], d_Tcw0, P, d_Tcw1, d_points, d_point_flags, d_inlier, d_consensus,
                     d_winner, d_good, d_tri, d_status);
}
