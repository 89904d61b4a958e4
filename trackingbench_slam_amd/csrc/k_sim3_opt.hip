/* Batched OptimizeSim3 (tb_sim3_optimize_batch_dev) -- extension, no reference counterpart: ORB-SLAM's Optimizer::OptimizeSim3
 * between the Horn-RANSAC (k_sim3.hip) and the Sim(3) pose graph (k_pgo_sim3.hip). One similarity S12 = (s, R12, t12),
 * X1 = s R12 X2 + t12, is refined on the two-image reprojection cost of pixel rows (tb_sim3_obs_row) under a Huber kernel;
 * include/tb_capi.h states the procedure, DESIGN.md 9p derives it, tests/sim3_opt_reference.py is the same in numpy.
 *
 * One 256-thread workgroup per problem runs the whole procedure -- two LM rounds with the outlier removal between them -- so the
 * call makes no host round trip and takes no work buffer. Thread t owns the rows t, t + 256, ... for the whole call: the
 * problem's slice of the output mask carries the rows' active flags (a thread reads only bytes it wrote itself, so no barrier
 * orders them) and is overwritten with the inlier flags at the end. A linearisation walks a thread's rows in ascending order and
 * adds into 35 registers (the upper triangle of J'WJ, J'We) that start at 0.0, a trial's evaluation into one (the robust chi2);
 * the 256 partial sums meet in the butterfly p[t] + p[t ^ d], d = 1 .. 128 (k_sim3's rule), which leaves the same bits in every
 * thread. The 7 x 7 solve and the trial's Exp run on one lane, as in k_pose; the accept / reject arithmetic is a few operations
 * on values every thread holds with the same bits. fixed_scale solves the same 7 x 7 system with its last row and column replaced
 * by the identity's, which gives the 6 x 6 factorisation's bits and sigma = 0 exactly. No atomics; every sum has a fixed shape, so a problem gives the same bits
 * alone, at any batch position and from run to run.
 *
 * Bound: latency (a dependent chain of up to 15 iterations x up to 10 trials, two block sums each); nothing here is tuned. */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_sim3.h"

#define SO_T 256
#define SO_SUMS 35   /* the linearisation's sums: 28 + 7; the robust chi2 is a block sum of its own */
#define SO_DBL_MAX 1.7976931348623157e308

static_assert(sizeof(tb_sim3_obs_row) == 48, "tb_sim3_obs_row layout");

struct SoShared {
    double red[SO_T / TB_WAVE][SO_SUMS];
    double trial[8];   /* qx qy qz qw, t, s */
    double sc;
    int solved;
    int cnt[SO_T / TB_WAVE];
};

/* what the cost uses of an element: the rotation matrix, t and s */
struct SoState { double R[9], t[3], s; };

__device__ __forceinline__ void so_state(const PoSim3& S, SoState& T) {
    po_to_R(S.T, T.R);
    T.t[0] = S.T.tx; T.t[1] = S.T.ty; T.t[2] = S.T.tz;
    T.s = S.s;
}

struct SoRow { double X1[3], X2[3], uv1[2], uv2[2], w1, w2; };

/* the row in float64; false where a field is not finite or Z1 / Z2 is not above 0 */
__device__ __forceinline__ bool so_row(const tb_sim3_obs_row& r, SoRow& o) {
    o.X1[0] = (double)r.X1; o.X1[1] = (double)r.Y1; o.X1[2] = (double)r.Z1;
    o.X2[0] = (double)r.X2; o.X2[1] = (double)r.Y2; o.X2[2] = (double)r.Z2;
    o.uv1[0] = (double)r.u1; o.uv1[1] = (double)r.v1; o.uv2[0] = (double)r.u2; o.uv2[1] = (double)r.v2;
    o.w1 = (double)r.inv_sigma2_1; o.w2 = (double)r.inv_sigma2_2;
    bool f = isfinite(o.w1) && isfinite(o.w2);
#pragma unroll
    for (int i = 0; i < 3; i++) f = f && isfinite(o.X1[i]) && isfinite(o.X2[i]);
#pragma unroll
    for (int i = 0; i < 2; i++) f = f && isfinite(o.uv1[i]) && isfinite(o.uv2[i]);
    return f && o.X1[2] > 0.0 && o.X2[2] > 0.0;
}

/* Q1 = s R X2 + t, Q2 = R' (X1 - t) / s */
__device__ __forceinline__ void so_map(const SoState& T, const SoRow& r, double (&Q1)[3], double (&Q2)[3]) {
    const double d[3] = {r.X1[0] - T.t[0], r.X1[1] - T.t[1], r.X1[2] - T.t[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Q1[i] = T.s * (T.R[3 * i] * r.X2[0] + T.R[3 * i + 1] * r.X2[1] + T.R[3 * i + 2] * r.X2[2]) + T.t[i];
        Q2[i] = (T.R[i] * d[0] + T.R[3 + i] * d[1] + T.R[6 + i] * d[2]) / T.s;
    }
}

/* e = uv - proj(Q) and the edge's plain chi2 */
__device__ __forceinline__ double so_edge(const double (&Q)[3], const double (&uv)[2], double w, double fx, double fy, double cx, double cy,
                                          double (&e)[2]) {
    e[0] = uv[0] - (fx * Q[0] / Q[2] + cx);
    e[1] = uv[1] - (fy * Q[1] / Q[2] + cy);
    return w * (e[0] * e[0] + e[1] * e[1]);
}

/* g2o's RobustKernelHuber with delta = sqrt(th2) on the plain chi2 c: rho; drho = rho' */
__device__ __forceinline__ double so_huber(double c, double th2, double delta, double& drho) {
    const double sq = sqrt(c);
    if (sq > delta) { drho = delta / sq; return 2.0 * sq * delta - th2; }
    drho = 1.0;
    return c;
}

/* index of (i, j), i <= j, in the packed upper triangle of a 7 x 7 */
__device__ __forceinline__ constexpr int so_tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }

/* acc += the edge's J' (w rho') J (upper triangle, 0 .. 27) and -J' (w rho') e (28 .. 34). D: dQ / ddelta, 3 x 7; J = -P(Q) D */
__device__ __forceinline__ void so_accumulate(const double (&Q)[3], const double (&D)[3][7], const double (&e)[2], double a, double fx, double fy,
                                              double (&acc)[SO_SUMS]) {
    const double iz = 1.0 / Q[2];
    const double p00 = fx * iz, p02 = -fx * Q[0] * iz * iz, p11 = fy * iz, p12 = -fy * Q[1] * iz * iz;
    double Ju[7], Jv[7];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        Ju[j] = -(p00 * D[0][j] + p02 * D[2][j]);
        Jv[j] = -(p11 * D[1][j] + p12 * D[2][j]);
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
#pragma unroll
        for (int j = i; j < 7; j++) acc[so_tri(i, j)] += a * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
        acc[28 + i] -= a * (Ju[i] * e[0] + Jv[i] * e[1]);
    }
}

/* [-[X]x | I | X] */
__device__ __forceinline__ void so_dpoint(const double (&X)[3], double (&D)[3][7]) {
    D[0][0] = 0.0;   D[0][1] = X[2];  D[0][2] = -X[1];
    D[1][0] = -X[2]; D[1][1] = 0.0;   D[1][2] = X[0];
    D[2][0] = X[1];  D[2][1] = -X[0]; D[2][2] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) D[i][3 + j] = i == j ? 1.0 : 0.0;
        D[i][6] = X[i];
    }
}

/* every thread's partial sums meet in the butterfly t ^ 1, 2, ..., 128 (k_sim3's s3_block_sum: the wave's six steps by shuffles,
 * the four wave sums through LDS as (w0 + w1) + (w2 + w3)). Called by the whole block; every thread gets the same bits. */
template <int K>
__device__ __forceinline__ void so_block_sum(double (&acc)[K], double (*red)[SO_SUMS]) {
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

__device__ __forceinline__ int so_block_count(int v, int* cnt) {
#pragma unroll
    for (int d = 1; d < TB_WAVE; d <<= 1) v += __shfl_xor(v, d, TB_WAVE);
    __syncthreads();
    if (tb_lane() == 0) cnt[threadIdx.x >> 6] = v;
    __syncthreads();
    return cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

/* the robust chi2 of the active rows under S: +inf where an active row's mapped depth is not above 0. The whole block calls it;
 * every thread gets the same bits. */
__device__ __forceinline__ double so_chi2(const PoSim3& S, const tb_sim3_obs_row* __restrict__ R, const uint8_t* act, int n, double fx, double fy,
                                          double cx, double cy, double th2, double delta, SoShared& sh) {
    SoState T;
    so_state(S, T);
    double c[1] = {0.0};
    int behind = 0;
    for (int i = threadIdx.x; i < n; i += SO_T) {
        if (!act[i]) continue;
        SoRow r;
        so_row(R[i], r);
        double Q1[3], Q2[3], e[2], dr;
        so_map(T, r, Q1, Q2);
        if (!(Q1[2] > 0.0) || !(Q2[2] > 0.0)) { behind = 1; continue; }
        const double r1 = so_huber(so_edge(Q1, r.uv1, r.w1, fx, fy, cx, cy, e), th2, delta, dr);
        const double r2 = so_huber(so_edge(Q2, r.uv2, r.w2, fx, fy, cx, cy, e), th2, delta, dr);
        c[0] += r1 + r2;
    }
    so_block_sum<1>(c, sh.red);
    return __syncthreads_or(behind) ? (double)INFINITY : c[0];
}

/* un-pivoted Cholesky solve of the 7 x 7 system (H + lambda I) x = b, H row-major; false if not positive definite */
__device__ inline bool so_chol7(const double (&H)[49], double lambda, const double (&b)[7], double (&x)[7]) {
    double A[49];
#pragma unroll
    for (int i = 0; i < 49; i++) A[i] = H[i] + ((i % 8 == 0) ? lambda : 0.0);
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = A[j * 7 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= A[j * 7 + k] * A[j * 7 + k];
        if (!(d > 0) || !isfinite(d)) return false;
        d = sqrt(d);
        A[j * 7 + j] = d;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[i * 7 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[i * 7 + k] * A[j * 7 + k];
            A[i * 7 + j] = s / d;
        }
    }
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= A[i * 7 + k] * y[k];
        y[i] = s / A[i * 7 + i];
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) s -= A[k * 7 + i] * x[k];
        x[i] = s / A[i * 7 + i];
    }
    return true;
}

/* finite entries, a quaternion of positive finite norm, a scale above 0 */
__device__ __forceinline__ bool so_srt_ok(const double (&v)[8]) {
    bool f = true;
#pragma unroll
    for (int i = 0; i < 8; i++) f = f && isfinite(v[i]);
    const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    return f && n2 > 0 && isfinite(n2) && v[7] > 0;
}

/* one problem's outputs but the mask: the transform S (srt_in's bytes `in`, read again, when keep; the identity matrix when
 * identity), the count, the statistics */
__device__ __forceinline__ void so_finish(const PoSim3& S, const double* in, bool keep, bool identity, int fixed_scale, double* o, float* S12,
                                          int32_t* inliers, double* stats, int ninl, double it, double chi0, double chi1, double trials,
                                          double nbad, double dropped, double lambda, double flag) {
    if (o) {
        if (keep) {
            if (o != in) {
#pragma unroll 1
                for (int i = 0; i < 8; i++) o[i] = in[i];
            }
        } else {
            o[0] = S.T.qw; o[1] = S.T.qx; o[2] = S.T.qy; o[3] = S.T.qz;
            o[4] = S.T.tx; o[5] = S.T.ty; o[6] = S.T.tz;
            o[7] = fixed_scale ? in[7] : S.s;
        }
    }
    if (S12) {
        SoState T;
        so_state(S, T);
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) S12[4 * i + j] = identity ? (i == j ? 1.f : 0.f) : (float)(T.s * T.R[3 * i + j]);
            S12[4 * i + 3] = identity ? 0.f : (float)T.t[i];
            S12[12 + i] = 0.f;
        }
        S12[15] = 1.f;
    }
    if (inliers) *inliers = ninl;
    if (stats) {
        stats[0] = it; stats[1] = chi0; stats[2] = chi1; stats[3] = trials;
        stats[4] = nbad; stats[5] = dropped; stats[6] = lambda; stats[7] = flag;
    }
}

__global__ void __launch_bounds__(SO_T)
k_sim3_opt(double fx, double fy, double cx, double cy, const tb_sim3_obs_row* __restrict__ rowsAll, const int32_t* __restrict__ counts, int pitch,
           const uint8_t* activeAll, const double* srtIn, double th2, int iters_first, int iters_bad, int iters_clean, int min_keep,
           int fixed_scale, double* srtOut, float* __restrict__ S12All, int32_t* __restrict__ inliers, uint8_t* maskAll,
           double* __restrict__ statsAll) {
    __shared__ SoShared sh;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[p], 0), pitch);
    const tb_sim3_obs_row* R = rowsAll + (size_t)p * pitch;
    const uint8_t* ain = activeAll ? activeAll + (size_t)p * pitch : nullptr;
    uint8_t* act = maskAll + (size_t)p * pitch;   /* the active flags during the call, the inlier flags after it */
    float* S12 = S12All ? S12All + 16 * (size_t)p : nullptr;
    double* stats = statsAll ? statsAll + 8 * (size_t)p : nullptr;
    const double delta = sqrt(th2);
    const int D = fixed_scale ? 6 : 7;

    double seed[8];
#pragma unroll
    for (int i = 0; i < 8; i++) seed[i] = srtIn[8 * (size_t)p + i];

#define SO_FINISH(S, keep, identity, ninl, it, c0, c1, tr, nb, dr, lam, flag)                                                         \
    do {                                                                                                                             \
        if (tid == 0)                                                                                                                \
            so_finish(S, srtIn + 8 * (size_t)p, keep, identity, fixed_scale, srtOut ? srtOut + 8 * (size_t)p : nullptr, S12,             \
                      inliers ? inliers + p : nullptr, stats, ninl, it, c0, c1, tr, nb, dr, lam, flag);                              \
    } while (0)
    auto clear_mask = [&]() {
        for (int i = tid; i < pitch; i += SO_T) act[i] = 0;
    };

    PoSim3 cur;
    cur.T.qw = 1.0; cur.T.qx = cur.T.qy = cur.T.qz = 0.0;
    cur.T.tx = cur.T.ty = cur.T.tz = 0.0;
    cur.s = 1.0;
    if (!so_srt_ok(seed)) { /* block-uniform: malformed */
        clear_mask();
        SO_FINISH(cur, true, true, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0);
        return;
    }
    cur.T.qw = seed[0]; cur.T.qx = seed[1]; cur.T.qy = seed[2]; cur.T.qz = seed[3];
    cur.T.tx = seed[4]; cur.T.ty = seed[5]; cur.T.tz = seed[6];
    cur.s = seed[7];
    po_normalize(cur.T);
    const PoSim3 S0 = cur;

    /* step 0: the rows that start active, and the dropped ones */
    int nact, dropped;
    {
        SoState T;
        so_state(cur, T);
        int a = 0, dr = 0;
        for (int i = tid; i < pitch; i += SO_T) {
            uint8_t on = 0;
            if (i < n && (!ain || ain[i])) {
                SoRow r;
                bool ok = so_row(R[i], r);
                double Q1[3], Q2[3];
                so_map(T, r, Q1, Q2);
                ok = ok && Q1[2] > 0.0 && Q2[2] > 0.0;
                on = ok ? 1 : 0;
                a += ok ? 1 : 0;
                dr += ok ? 0 : 1;
            }
            act[i] = on;
        }
        nact = so_block_count(a, sh.cnt);
        dropped = so_block_count(dr, sh.cnt);
    }
    double chi = so_chi2(cur, R, act, n, fx, fy, cx, cy, th2, delta, sh);
    const double chi0 = chi;
    if (nact < min_keep) { /* block-uniform */
        clear_mask();
        SO_FINISH(S0, true, false, 0, 0.0, chi0, chi0, 0.0, 0.0, (double)dropped, 0.0, 1.0);
        return;
    }

    double lambda = 0.0;
    int done = 0, trials = 0, accepted_any = 0, nbad = 0;
    for (int rnd = 0; rnd < 2; rnd++) {
        const int iters = rnd == 0 ? iters_first : (nbad > 0 ? iters_bad : iters_clean);
        if (rnd == 1) chi = so_chi2(cur, R, act, n, fx, fy, cx, cy, th2, delta, sh);   /* the rows left */
        double nu = 2.0;
        bool ok = true;
        lambda = 0.0;
        for (int iter = 0; iter < iters && ok; iter++) {
            /* linearise at cur */
            double acc[SO_SUMS];
#pragma unroll
            for (int k = 0; k < SO_SUMS; k++) acc[k] = 0.0;
            {
                SoState T;
                so_state(cur, T);
                for (int i = tid; i < n; i += SO_T) {
                    if (!act[i]) continue;
                    SoRow r;
                    so_row(R[i], r);
                    double Q1[3], Q2[3], e[2], dr, Dq[3][7], D2[3][7];
                    so_map(T, r, Q1, Q2);
                    double c = so_edge(Q1, r.uv1, r.w1, fx, fy, cx, cy, e);
                    so_huber(c, th2, delta, dr);
                    so_dpoint(Q1, Dq);
                    so_accumulate(Q1, Dq, e, r.w1 * dr, fx, fy, acc);
                    c = so_edge(Q2, r.uv2, r.w2, fx, fy, cx, cy, e);
                    so_huber(c, th2, delta, dr);
                    so_dpoint(r.X1, Dq);
                    const double ns = -1.0 / T.s;
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int j = 0; j < 7; j++) D2[a][j] = ns * (T.R[a] * Dq[0][j] + T.R[3 + a] * Dq[1][j] + T.R[6 + a] * Dq[2][j]);
                    so_accumulate(Q2, D2, e, r.w2 * dr, fx, fy, acc);
                }
            }
            so_block_sum<SO_SUMS>(acc, sh.red);
            if (iter == 0) {
                double md = 0.0;
#pragma unroll
                for (int i = 0; i < 7; i++)
                    if (i < D) md = fmax(md, fabs(acc[so_tri(i, i)]));
                lambda = 1e-5 * md;
                nu = 2.0;
            }
            double rho = 0.0;
            int q = 0;
            do {
                if (tid == 0) { /* the solve and the trial's element, on one lane */
                    double H[49], g[7], x[7];
#pragma unroll
                    for (int i = 0; i < 7; i++) {
#pragma unroll
                        for (int j = i; j < 7; j++) {
                            const bool held = fixed_scale && j == 6;
                            const double v = held ? (i == 6 ? 1.0 : 0.0) : acc[so_tri(i, j)];
                            H[i * 7 + j] = v;
                            H[j * 7 + i] = v;
                        }
                        g[i] = (fixed_scale && i == 6) ? 0.0 : acc[28 + i];
                    }
                    const bool solved = so_chol7(H, lambda, g, x);
                    if (!solved) {
#pragma unroll
                        for (int i = 0; i < 7; i++) x[i] = 0.0;
                    }
                    double sc = 0.0;
#pragma unroll
                    for (int i = 0; i < 7; i++)
                        if (i < D) sc += x[i] * (lambda * x[i] + g[i]);
                    if (fixed_scale) x[6] = 0.0;   /* e^0 = 1: s keeps its bits */
                    const PoSim3 at = cur;   /* a copy: the call takes an address */
                    const PoSim3 tr = s3_mul(s3_exp(x), at);
                    sh.trial[0] = tr.T.qx; sh.trial[1] = tr.T.qy; sh.trial[2] = tr.T.qz; sh.trial[3] = tr.T.qw;
                    sh.trial[4] = tr.T.tx; sh.trial[5] = tr.T.ty; sh.trial[6] = tr.T.tz; sh.trial[7] = tr.s;
                    sh.sc = sc;
                    sh.solved = solved ? 1 : 0;
                }
                __syncthreads();
                PoSim3 trial;
                trial.T.qx = sh.trial[0]; trial.T.qy = sh.trial[1]; trial.T.qz = sh.trial[2]; trial.T.qw = sh.trial[3];
                trial.T.tx = sh.trial[4]; trial.T.ty = sh.trial[5]; trial.T.tz = sh.trial[6]; trial.s = sh.trial[7];
                const double sc = sh.sc;
                const bool solved = sh.solved != 0;
                double tchi = so_chi2(trial, R, act, n, fx, fy, cx, cy, th2, delta, sh);   /* its barriers also free sh.trial */
                if (!solved) tchi = SO_DBL_MAX;
                rho = (chi - tchi) / (sc + 1e-3);
                if (rho > 0 && isfinite(tchi)) {
                    double alpha = 1.0 - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                    alpha = fmin(alpha, 2.0 / 3.0);
                    lambda *= fmax(1.0 / 3.0, alpha);
                    nu = 2.0;
                    chi = tchi;
                    cur = trial;
                    accepted_any = 1;
                } else {
                    lambda *= nu;
                    nu *= 2;
                }
                q++;
                trials++;
            } while (rho < 0 && q < 10);
            done++;
            if (q == 10 || rho == 0) ok = false;
        }
        if (rnd == 0) { /* step 2: the bad rows leave, both edges together */
            SoState T;
            so_state(cur, T);
            int nb = 0;
            for (int i = tid; i < n; i += SO_T) {
                if (!act[i]) continue;
                SoRow r;
                so_row(R[i], r);
                double Q1[3], Q2[3], e[2];
                so_map(T, r, Q1, Q2);
                const double c1 = so_edge(Q1, r.uv1, r.w1, fx, fy, cx, cy, e), c2 = so_edge(Q2, r.uv2, r.w2, fx, fy, cx, cy, e);
                if (c1 > th2 || c2 > th2) { act[i] = 0; nb++; }
            }
            nbad = so_block_count(nb, sh.cnt);
            nact -= nbad;
            if (nact < min_keep) { /* block-uniform: step 3 */
                clear_mask();
                SO_FINISH(S0, true, false, 0, (double)done, chi0, chi, (double)trials, (double)nbad, (double)dropped, lambda, 1.0);
                return;
            }
        }
    }
    /* step 5: the mask and the count under the final transform */
    int ninl = 0;
    {
        SoState T;
        so_state(cur, T);
        for (int i = tid; i < pitch; i += SO_T) {
            bool in = false;
            if (i < n && act[i]) {
                SoRow r;
                so_row(R[i], r);
                double Q1[3], Q2[3], e[2];
                so_map(T, r, Q1, Q2);
                const double c1 = so_edge(Q1, r.uv1, r.w1, fx, fy, cx, cy, e), c2 = so_edge(Q2, r.uv2, r.w2, fx, fy, cx, cy, e);
                in = c1 <= th2 && c2 <= th2;
            }
            act[i] = in ? 1 : 0;
            ninl += in ? 1 : 0;
        }
        ninl = so_block_count(ninl, sh.cnt);
    }
    SO_FINISH(cur, !accepted_any, false, ninl, (double)done, chi0, chi, (double)trials, (double)nbad, (double)dropped, lambda, 0.0);
}
#undef SO_FINISH

int tbk_sim3_opt_batch(tb_ctx* ctx, int nproblems, const double K[4], const tb_sim3_obs_row* d_rows, const int32_t* d_counts, int pitch,
                       const uint8_t* d_active, const double* d_srt_in, const tb_sim3_opt_params* prm, double* d_srt_out, float* d_S12,
                       int32_t* d_inliers, uint8_t* d_mask, double* d_stats) {
    if (nproblems <= 0) return TB_OK;
    return tb_launch(ctx, "k_sim3_opt", k_sim3_opt, dim3(nproblems), dim3(SO_T), 0, K[0], K[1], K[2], K[3], d_rows, d_counts, pitch, d_active,
                     d_srt_in, prm->th2, prm->iters_first, prm->iters_bad, prm->iters_clean, prm->min_keep, prm->fixed_scale, d_srt_out, d_S12,
                     d_inliers, d_mask, d_stats);
}
