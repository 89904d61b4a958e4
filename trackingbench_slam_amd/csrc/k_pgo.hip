/* Batched SE(3) pose-graph optimisation (tb_pose_graph_batch_dev) -- extension, no reference counterpart: the solver between
 * PoseOptimization (one pose, k_pose.hip) and the local BA (poses and points, k_ba.hip).
 *
 * One 256-thread workgroup per graph runs the whole Levenberg-Marquardt loop, so the call makes no host round trip. A graph has
 * up to 64 poses Tcw (the first nfixed held) and up to 256 edges (a, b, Z, w_rot, w_trans), Z ~ T_b T_a^-1. Residual r =
 * Log(Z^-1 T_b T_a^-1) ordered (omega, upsilon), update T <- exp(delta) T (po_exp_mul), exact Jacobians J_b = Jl^-1(r) Ad(Z^-1),
 * J_a = -Jl^-1(r) Ad(E), information diag(w_rot I3, w_trans I3), no robust kernel; g2o's LM rule as the local BA restates it
 * (lambda0 = 1e-5 max diag H, accept on rho > 0 and a finite chi2, at most 10 trials per iteration). tests/pose_graph_reference.py
 * is the same in numpy.
 *
 * Linearisation: one thread per edge writes r, J_a, J_b to the graph's scratch. Assembly: one thread per (free node, row,
 * column) walks the edges in list order and sums the node's diagonal block, its right-hand side and its blocks with lower-numbered
 * free nodes -- every entry of H has one owner and one order, so there is no atomic and a graph's bits do not depend on the batch.
 * Solve: H + lambda I (up to 378 x 378, packed lower triangle, 560 KB) stays in the scratch; the right-hand side rides along as row N
 * of the matrix, so the factorisation leaves L^-1 g there. A right-looking Cholesky factorises it panel by panel: PG_PANEL columns
 * at a time come into LDS (N + 1 rows, 36 KB), thread 0 factorises the diagonal block, every thread solves its rows against it,
 * and the trailing update L_ij -= sum_c P_ic P_jc runs on the vector pipe in 16 x 16 tiles of the lower triangle. The back
 * substitution walks the panels in reverse with one fixed-shape block sum each. Every sum over edges or unknowns is such a
 * block sum, so a run repeats bit for bit.
 *
 * Bound: latency (a dependent chain of ~N / PG_PANEL panel steps per trial, each a few L2 round trips); loop closures are rare
 * and the graphs small, so nothing here is tuned for throughput.
 */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_se3.h"

#define PG_T 256
#define PG_MAX_NODES 64
#define PG_MAX_EDGES 256
#define PG_PANEL 12  /* columns of one panel: two nodes */
#define PG_TILE 16   /* the trailing update's tile */
#define PG_MAX_N (6 * (PG_MAX_NODES - 1))

static_assert(sizeof(tb_pg_edge) == 80, "tb_pg_edge layout");

struct PgShared {
    PoSE3 cur[PG_MAX_NODES], trial[PG_MAX_NODES];
    int ea[PG_MAX_EDGES], eb[PG_MAX_EDGES];
    double wr[PG_MAX_EDGES], wt[PG_MAX_EDGES];
    double g[PG_MAX_N], x[PG_MAX_N];
    double pan[(PG_MAX_N + 1) * PG_PANEL];
    double red[4 * PG_PANEL];
    int ok;
};

__device__ __forceinline__ size_t pg_tri(int i) { return (size_t)i * (i + 1) / 2; } /* first entry of packed row i */

/* Zi = Z^-1 and E = Z^-1 T_b T_a^-1 of one edge */
__device__ inline void pg_edge_E(const tb_pg_edge& ed, const PoSE3* T, PoSE3& Zi, PoSE3& E) {
    PoSE3 Z;
    Z.qx = ed.q[0]; Z.qy = ed.q[1]; Z.qz = ed.q[2]; Z.qw = ed.q[3];
    Z.tx = ed.t[0]; Z.ty = ed.t[1]; Z.tz = ed.t[2];
    po_normalize(Z);
    Zi = po_inverse(Z);
    E = po_mul(Zi, po_mul(T[ed.b], po_inverse(T[ed.a])));
}

/* chi2 of the poses T: the block's sum over its edges; the same value in every thread */
__device__ inline double pg_chi2(const tb_pg_edge* edges, int E, const PoSE3* T, double* red) {
    double c[1] = {0.0};
    for (int e = threadIdx.x; e < E; e += PG_T) {
        const tb_pg_edge ed = edges[e];
        PoSE3 Zi, Ee;
        pg_edge_E(ed, T, Zi, Ee);
        double r[6];
        po_log(Ee, r);
        c[0] += ed.w_rot * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + ed.w_trans * (r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
    }
    po_block_sum<1>(c, red);
    return c[0];
}

__global__ void __launch_bounds__(PG_T)
k_pgo(int nnodes, int nfixed, float* __restrict__ posesAll, const tb_pg_edge* __restrict__ edgesAll, const int32_t* __restrict__ counts,
      int edge_pitch, int iters, double* __restrict__ statsAll, double* __restrict__ work, size_t work_per_graph) {
    __shared__ PgShared S;
    const int gi = blockIdx.x, tid = threadIdx.x;
    const int nfree = nnodes - nfixed, N = 6 * nfree, M = N + 1;
    float* poses = posesAll + (size_t)gi * nnodes * 16;
    const tb_pg_edge* edges = edgesAll + (size_t)gi * edge_pitch;
    double* stats = statsAll ? statsAll + 8 * (size_t)gi : nullptr;
    double* H = work + (size_t)gi * work_per_graph;   /* packed lower triangle, N rows */
    double* L = H + pg_tri(N);                        /* the same with lambda, and the right-hand side as row N */
    double* Jc = L + pg_tri(M);                       /* [edge_pitch][2][36] J_a, J_b */
    double* rc = Jc + (size_t)edge_pitch * 72;        /* [edge_pitch][6] */
    const int E = counts[gi];

    /* the check: a graph that fails it keeps every byte */
    int bad = (E < 0 || E > edge_pitch) ? 1 : 0;
    if (!bad)
        for (int e = tid; e < E; e += PG_T) {
            const tb_pg_edge ed = edges[e];
            bool f = isfinite(ed.w_rot) && isfinite(ed.w_trans) && ed.w_rot >= 0 && ed.w_trans >= 0;
            for (int i = 0; i < 4; i++) f = f && isfinite(ed.q[i]);
            for (int i = 0; i < 3; i++) f = f && isfinite(ed.t[i]);
            const double n2 = ed.q[0] * ed.q[0] + ed.q[1] * ed.q[1] + ed.q[2] * ed.q[2] + ed.q[3] * ed.q[3];
            f = f && n2 > 0 && isfinite(n2);
            if (!f || ed.a < 0 || ed.a >= nnodes || ed.b < 0 || ed.b >= nnodes || ed.a == ed.b) bad = 1;
        }
    bad = __syncthreads_or(bad);
    if (bad || E == 0) {
        if (stats && tid < 8) stats[tid] = (bad && tid == 7) ? -1.0 : 0.0;
        return;
    }
    for (int e = tid; e < E; e += PG_T) {
        S.ea[e] = edges[e].a; S.eb[e] = edges[e].b;
        S.wr[e] = edges[e].w_rot; S.wt[e] = edges[e].w_trans;
    }
    if (tid < nnodes) {
        const float* Tin = poses + 16 * tid;
        double R[9], t[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) R[i * 3 + j] = (double)Tin[i * 4 + j];
            t[i] = (double)Tin[i * 4 + 3];
        }
        S.cur[tid] = po_from_Rt(R, t);
        S.trial[tid] = S.cur[tid];
    }
    __syncthreads();
    double cur = pg_chi2(edges, E, S.cur, S.red);
    const double chi0 = cur;
    double lambda = 0.0, nu = 2.0;
    int done = 0, trials = 0, accepted_any = 0;
    bool ok = true;

    for (int iter = 0; iter < iters && ok; iter++) {
        /* linearise */
        for (int e = tid; e < E; e += PG_T) {
            const tb_pg_edge ed = edges[e];
            PoSE3 Zi, Ee;
            pg_edge_E(ed, S.cur, Zi, Ee);
            double r[6], Ji[36], A[36];
            po_log(Ee, r);
            po_jl_inv(r, Ji);
            for (int i = 0; i < 6; i++) rc[(size_t)e * 6 + i] = r[i];
            double* Ja = Jc + (size_t)e * 72;
            po_adjoint(Ee, A);
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    double s = 0.0;
                    for (int k = 0; k < 6; k++) s += Ji[i * 6 + k] * A[k * 6 + j];
                    Ja[i * 6 + j] = -s;
                }
            po_adjoint(Zi, A);
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    double s = 0.0;
                    for (int k = 0; k < 6; k++) s += Ji[i * 6 + k] * A[k * 6 + j];
                    Ja[36 + i * 6 + j] = s;
                }
        }
        for (size_t i = tid; i < pg_tri(N); i += PG_T) H[i] = 0.0;
        __syncthreads();
        /* assemble: item = (free node, row, column); edges in list order */
        for (int item = tid; item < 36 * nfree; item += PG_T) {
            const int nf = item / 36, r = (item % 36) / 6, c = item % 6, node = nf + nfixed;
            const int row = 6 * nf + r;
            double diag = 0.0, gs = 0.0;
            for (int e = 0; e < E; e++) {
                const int a = S.ea[e], b = S.eb[e];
                if (a != node && b != node) continue;
                const double* Ji = Jc + (size_t)e * 72 + (a == node ? 0 : 36);
                const double* Jo = Jc + (size_t)e * 72 + (a == node ? 36 : 0);
                const int o = a == node ? b : a;
                const double wr = S.wr[e], wt = S.wt[e];
                double d = 0.0;
                for (int k = 0; k < 6; k++) d += Ji[k * 6 + r] * ((k < 3 ? wr : wt) * Ji[k * 6 + c]);
                diag += d;
                if (c == 0) {
                    double s = 0.0;
                    for (int k = 0; k < 6; k++) s += Ji[k * 6 + r] * ((k < 3 ? wr : wt) * rc[(size_t)e * 6 + k]);
                    gs -= s;
                }
                if (o >= nfixed && o < node) {
                    double s = 0.0;
                    for (int k = 0; k < 6; k++) s += Ji[k * 6 + r] * ((k < 3 ? wr : wt) * Jo[k * 6 + c]);
                    H[pg_tri(row) + 6 * (o - nfixed) + c] += s;
                }
            }
            if (c <= r) H[pg_tri(row) + 6 * nf + c] = diag;
            if (c == r) S.x[row] = diag;
            if (c == 0) S.g[row] = gs;
        }
        __syncthreads();
        if (iter == 0) {
            double md = 0.0;
            for (int i = 0; i < N; i++) md = fmax(md, fabs(S.x[i]));
            lambda = 1e-5 * md;
            nu = 2.0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            /* L = H + lambda I, the right-hand side as row N */
            for (size_t i = tid; i < pg_tri(N); i += PG_T) L[i] = H[i];
            __syncthreads();   /* S.x: the diagonal's readers are done; L: the diagonal's writers come after the copy */
            for (int i = tid; i < N; i += PG_T) {
                L[pg_tri(i) + i] += lambda;
                L[pg_tri(N) + i] = S.g[i];
            }
            if (tid == 0) S.ok = 1;
            __syncthreads();
            /* right-looking Cholesky, PG_PANEL columns at a time */
            bool solved = true;
            for (int k0 = 0; k0 < N; k0 += PG_PANEL) {
                const int pw = min(PG_PANEL, N - k0), below = k0 + pw;
                for (int i = tid; i < (M - k0) * PG_PANEL; i += PG_T) {
                    const int row = k0 + i / PG_PANEL, c = i % PG_PANEL;
                    S.pan[i] = (c < pw && k0 + c <= row) ? L[pg_tri(row) + k0 + c] : 0.0;
                }
                __syncthreads();
                if (tid == 0) {
                    for (int j = 0; j < pw; j++) {
                        double d = S.pan[j * PG_PANEL + j];
                        for (int k = 0; k < j; k++) d -= S.pan[j * PG_PANEL + k] * S.pan[j * PG_PANEL + k];
                        if (!(d > 0) || !isfinite(d)) { S.ok = 0; break; }
                        d = sqrt(d);
                        S.pan[j * PG_PANEL + j] = d;
                        for (int i = j + 1; i < pw; i++) {
                            double s = S.pan[i * PG_PANEL + j];
                            for (int k = 0; k < j; k++) s -= S.pan[i * PG_PANEL + k] * S.pan[j * PG_PANEL + k];
                            S.pan[i * PG_PANEL + j] = s / d;
                        }
                    }
                }
                __syncthreads();
                if (!S.ok) { solved = false; break; }
                for (int row = below + tid; row < M; row += PG_T) {
                    double* p = S.pan + (row - k0) * PG_PANEL;
                    for (int c = 0; c < pw; c++) {
                        double s = p[c];
                        for (int k = 0; k < c; k++) s -= p[k] * S.pan[c * PG_PANEL + k];
                        p[c] = s / S.pan[c * PG_PANEL + c];
                    }
                }
                __syncthreads();
                for (int i = tid; i < (M - k0) * PG_PANEL; i += PG_T) {
                    const int row = k0 + i / PG_PANEL, c = i % PG_PANEL;
                    if (c < pw && k0 + c <= row) L[pg_tri(row) + k0 + c] = S.pan[i];
                }
                /* trailing update in PG_TILE x PG_TILE tiles of the lower triangle (rows below..M-1, columns below..N-1) */
                const int ty = tid / PG_TILE, tx = tid % PG_TILE;
                const int nt = (M - below + PG_TILE - 1) / PG_TILE;
                for (int ti = 0; ti < nt; ti++)
                    for (int tj = 0; tj <= ti; tj++) {
                        const int row = below + ti * PG_TILE + ty, col = below + tj * PG_TILE + tx;
                        if (row < M && col <= row && col < N) {
                            const double* pi = S.pan + (row - k0) * PG_PANEL;
                            const double* pj = S.pan + (col - k0) * PG_PANEL;
                            double s = 0.0;
                            for (int c = 0; c < PG_PANEL; c++) s += pi[c] * pj[c];
                            L[pg_tri(row) + col] -= s;
                        }
                    }
                __syncthreads();
            }
            /* back substitution L' x = y, y = row N, the panels in reverse */
            if (solved) {
                const int np = (N + PG_PANEL - 1) / PG_PANEL;
                for (int p = np - 1; p >= 0; p--) {
                    const int k0 = p * PG_PANEL, pw = min(PG_PANEL, N - k0), below = k0 + pw;
                    double acc[PG_PANEL];
                    for (int c = 0; c < PG_PANEL; c++) acc[c] = 0.0;
                    for (int row = below + tid; row < N; row += PG_T) {
                        const double xr = S.x[row];
                        for (int c = 0; c < PG_PANEL; c++)
                            if (c < pw) acc[c] += L[pg_tri(row) + k0 + c] * xr;
                    }
                    po_block_sum<PG_PANEL>(acc, S.red);
                    if (tid == 0)
                        for (int c = pw - 1; c >= 0; c--) {
                            double s = L[pg_tri(N) + k0 + c] - acc[c];
                            for (int k = c + 1; k < pw; k++) s -= L[pg_tri(k0 + k) + k0 + c] * S.x[k0 + k];
                            S.x[k0 + c] = s / L[pg_tri(k0 + c) + k0 + c];
                        }
                    __syncthreads();
                }
            } else {
                for (int i = tid; i < N; i += PG_T) S.x[i] = 0.0;
                __syncthreads();
            }
            /* the trial */
            if (tid >= nfixed && tid < nnodes) S.trial[tid] = po_exp_mul(S.x + 6 * (tid - nfixed), S.cur[tid]);
            __syncthreads();
            double trial = pg_chi2(edges, E, S.trial, S.red);
            if (!solved) trial = 1.7976931348623157e308;
            double sc[1] = {0.0};
            for (int i = tid; i < N; i += PG_T) sc[0] += S.x[i] * (lambda * S.x[i] + S.g[i]);
            po_block_sum<1>(sc, S.red);
            rho = (cur - trial) / (sc[0] + 1e-3);
            if (rho > 0 && isfinite(trial)) {
                double alpha = 1.0 - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                alpha = fmin(alpha, 2.0 / 3.0);
                lambda *= fmax(1.0 / 3.0, alpha);
                nu = 2.0;
                cur = trial;
                accepted_any = 1;
                if (tid < nnodes) S.cur[tid] = S.trial[tid];
            } else {
                lambda *= nu;
                nu *= 2;
            }
            __syncthreads();
            qmax++;
            trials++;
        } while (rho < 0 && qmax < 10);
        done++;
        if (qmax == 10 || rho == 0) ok = false;
    }
    /* fixed nodes and a graph that accepted no step keep their bytes */
    if (accepted_any && tid >= nfixed && tid < nnodes) {
        double R[9];
        po_to_R(S.cur[tid], R);
        float* Tout = poses + 16 * tid;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Tout[i * 4 + j] = (float)R[i * 3 + j];
        }
        Tout[3] = (float)S.cur[tid].tx; Tout[7] = (float)S.cur[tid].ty; Tout[11] = (float)S.cur[tid].tz;
        Tout[12] = Tout[13] = Tout[14] = 0.f;
        Tout[15] = 1.f;
    }
    if (stats && tid == 0) {
        stats[0] = done; stats[1] = chi0; stats[2] = cur; stats[3] = lambda; stats[4] = trials;
        stats[5] = stats[6] = stats[7] = 0.0;
    }
}

/* doubles of scratch one graph takes: H, L with its extra row, the edges' Jacobians and residuals */
static size_t pg_work_doubles(int nnodes, int nfixed, int edge_pitch) {
    const size_t N = 6 * (size_t)(nnodes - nfixed);
    return N * (N + 1) / 2 + (N + 1) * (N + 2) / 2 + (size_t)edge_pitch * 78;
}

size_t tbk_pose_graph_work_bytes(int ngraphs, int nnodes, int nfixed, int edge_pitch) {
    return (size_t)ngraphs * pg_work_doubles(nnodes, nfixed, edge_pitch) * sizeof(double);
}

int tbk_pose_graph_batch(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, float* d_poses, const tb_pg_edge* d_edges,
                         const int32_t* d_counts, int edge_pitch, int iters, double* d_stats, void* d_work) {
    return tb_launch(ctx, "k_pgo", k_pgo, dim3(ngraphs), dim3(PG_T), 0, nnodes, nfixed, d_poses, d_edges, d_counts, edge_pitch, iters,
                     d_stats, (double*)d_work, pg_work_doubles(nnodes, nfixed, edge_pitch));
}

/* ---- loop correction in the VO loop (tb_vo_loop_enable, tb_vo.cpp): the graph of a sequence's stored keyframes and its current
 * frame, and the adoption of the solver's poses. The ring is counted for the whole batch (lock-step), so the host knows which
 * slots are live and their order: node i < nlive is ring slot (oldest + i) % cap, node nlive the current frame, the other
 * nodes the identity, which no edge names. */
__device__ inline PoSE3 pg_pose_from_f32(const float* T) {
    double R[9], t[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i * 3 + j] = (double)T[i * 4 + j];
        t[i] = (double)T[i * 4 + 3];
    }
    return po_from_Rt(R, t);
}
__device__ inline void pg_edge_write(tb_pg_edge* e, int a, int b, const PoSE3& Ta, const PoSE3& Tb, double w_rot, double w_trans) {
    const PoSE3 Z = po_mul(Tb, po_inverse(Ta));
    e->a = a; e->b = b;
    e->q[0] = Z.qx; e->q[1] = Z.qy; e->q[2] = Z.qz; e->q[3] = Z.qw;
    e->t[0] = Z.tx; e->t[1] = Z.ty; e->t[2] = Z.tz;
    e->w_rot = w_rot; e->w_trans = w_trans;
}

/* one 64-thread workgroup per sequence, thread i = node i (nn = cap + 1 <= 64 nodes, edge pitch nn) */
__global__ void __launch_bounds__(64)
k_vo_loop_graph(int cap, int nlive, int oldest, int frame, int topk, double w_rot, double w_trans, const float* __restrict__ s_Tcw,
                const int32_t* __restrict__ s_kf_ids, const float* __restrict__ cur_Tcw, const int32_t* __restrict__ best_rank,
                const int32_t* __restrict__ best_kf, const float* __restrict__ best_Tcw, float* __restrict__ before,
                float* __restrict__ after, int32_t* __restrict__ node_kf, int32_t* __restrict__ nnodes, tb_pg_edge* __restrict__ edges,
                int32_t* __restrict__ ecount) {
    const int s = blockIdx.x, i = threadIdx.x, nn = cap + 1;
    if (i >= nn) return;
    const float* Tkf = s_Tcw + (size_t)s * cap * 16;
    const int32_t* ids = s_kf_ids + (size_t)s * cap;
    auto node_pose = [&](int n) { return n < nlive ? Tkf + (size_t)((oldest + n) % cap) * 16 : cur_Tcw + (size_t)s * 16; };
    float* pb = before + ((size_t)s * nn + i) * 16;
    float* pa = after + ((size_t)s * nn + i) * 16;
    if (i <= nlive) {
        const float* T = node_pose(i);
        for (int k = 0; k < 16; k++) pb[k] = pa[k] = T[k];
        node_kf[(size_t)s * nn + i] = i < nlive ? ids[(oldest + i) % cap] : frame;
    } else {
        for (int k = 0; k < 16; k++) pb[k] = pa[k] = (k % 5 == 0) ? 1.f : 0.f;
        node_kf[(size_t)s * nn + i] = -1;
    }
    const bool loop = best_rank[s] >= 0 && best_rank[s] < topk && nlive >= 2;
    if (i == 0) {
        nnodes[s] = nlive + 1;
        ecount[s] = loop ? nlive + 1 : 0;
    }
    if (!loop) return;
    tb_pg_edge* e = edges + (size_t)s * nn + i;
    if (i < nlive) {   /* odometry: node i -> node i + 1 */
        pg_edge_write(e, i, i + 1, pg_pose_from_f32(node_pose(i)), pg_pose_from_f32(node_pose(i + 1)), w_rot, w_trans);
    } else if (i == nlive) {   /* the loop edge: the winning keyframe's node -> the current node; a keyframe the ring no longer
                                * holds leaves a = -1, which the solver flags */
        int j = -1;
        for (int n = 0; n < nlive; n++)
            if (ids[(oldest + n) % cap] == best_kf[s]) j = n;
        pg_edge_write(e, j, nlive, pg_pose_from_f32(node_pose(j < 0 ? 0 : j)), pg_pose_from_f32(best_Tcw + (size_t)s * 16), w_rot, w_trans);
    }
}

/* X' = T_new^-1 (T_old X) in FP64 for the valid points of one list, stored as float32 */
__device__ inline void pg_move_points(const float* Told, const float* Tnew, float* mp, const uint8_t* valid, int n) {
    double Ro[9], to[3], Rn[9], tn[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) { Ro[i * 3 + j] = (double)Told[i * 4 + j]; Rn[i * 3 + j] = (double)Tnew[i * 4 + j]; }
        to[i] = (double)Told[i * 4 + 3]; tn[i] = (double)Tnew[i * 4 + 3];
    }
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        if (!valid[p]) continue;
        const double X[3] = {(double)mp[3 * p], (double)mp[3 * p + 1], (double)mp[3 * p + 2]};
        double Y[3];
        for (int i = 0; i < 3; i++) Y[i] = (Ro[i * 3] * X[0] + Ro[i * 3 + 1] * X[1] + Ro[i * 3 + 2] * X[2]) + to[i] - tn[i];
        for (int i = 0; i < 3; i++) mp[3 * p + i] = (float)(Rn[i] * Y[0] + Rn[3 + i] * Y[1] + Rn[6 + i] * Y[2]);
    }
}

/* workgroup (s, j): j < nlive the stored keyframe of node j, j == nlive the keyframe snapshot, j == nlive + 1 the frame's carried
 * points and its pose. A sequence adopts where a loop edge was built and the solver did not flag the graph. */
__global__ void __launch_bounds__(256)
k_vo_loop_adopt(int cap, int nlive, int oldest, int topk, int pitch, const float* __restrict__ before, const float* __restrict__ after,
                const int32_t* __restrict__ ecount, const double* __restrict__ stats, const int32_t* __restrict__ best_rank,
                const int32_t* __restrict__ best_kf, const int32_t* __restrict__ cand_inliers, float* __restrict__ s_Tcw,
                float* __restrict__ s_mp, const uint8_t* __restrict__ s_valid, const int32_t* __restrict__ s_counts,
                float* __restrict__ kf_mp, const uint8_t* __restrict__ kf_valid, const int32_t* __restrict__ kf_cnt,
                float* __restrict__ mp, const uint8_t* __restrict__ valid, const int32_t* __restrict__ key_counts, float* __restrict__ Tcw,
                uint8_t* __restrict__ closed, int32_t* __restrict__ loop_kf, int32_t* __restrict__ loop_inliers) {
    const int s = blockIdx.x, j = blockIdx.y, nn = cap + 1;
    const bool adopt = ecount[s] > 0 && stats[8 * (size_t)s + 7] == 0.0;
    if (j == 0 && threadIdx.x == 0) {
        closed[s] = adopt ? 1 : 0;
        loop_kf[s] = adopt ? best_kf[s] : -1;
        loop_inliers[s] = adopt ? cand_inliers[(size_t)s * topk + best_rank[s]] : 0;
    }
    if (!adopt) return;
    const float* B = before + (size_t)s * nn * 16;
    const float* A = after + (size_t)s * nn * 16;
    if (j < nlive) {
        const size_t slot = (size_t)s * cap + (oldest + j) % cap;
        pg_move_points(B + 16 * j, A + 16 * j, s_mp + slot * pitch * 3, s_valid + slot * pitch, min(s_counts[slot], pitch));
        if (threadIdx.x < 16) s_Tcw[slot * 16 + threadIdx.x] = A[16 * j + threadIdx.x];
    } else if (j == nlive) {   /* copies of the newest keyframe's points move by its correction */
        pg_move_points(B + 16 * (nlive - 1), A + 16 * (nlive - 1), kf_mp + (size_t)s * pitch * 3, kf_valid + (size_t)s * pitch,
                       min(kf_cnt[s], pitch));
    } else {
        pg_move_points(B + 16 * (nlive - 1), A + 16 * (nlive - 1), mp + (size_t)s * pitch * 3, valid + (size_t)s * pitch,
                       min(key_counts[s], pitch));
        if (threadIdx.x < 16) Tcw[(size_t)s * 16 + threadIdx.x] = A[16 * nlive + threadIdx.x];
    }
}

int tbk_vo_loop_graph(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int frame, int topk, double w_rot, double w_trans,
                      const float* s_Tcw, const int32_t* s_kf_ids, const float* cur_Tcw, const int32_t* best_rank, const int32_t* best_kf,
                      const float* best_Tcw, float* before, float* after, int32_t* node_kf, int32_t* nnodes, tb_pg_edge* edges,
                      int32_t* ecount) {
    return tb_launch(ctx, "k_vo_loop_graph", k_vo_loop_graph, dim3(nseq), dim3(64), 0, cap, nlive, oldest, frame, topk, w_rot, w_trans, s_Tcw,
                     s_kf_ids, cur_Tcw, best_rank, best_kf, best_Tcw, before, after, node_kf, nnodes, edges, ecount);
}

int tbk_vo_loop_adopt(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int topk, int pitch, const float* before, const float* after,
                      const int32_t* ecount, const double* stats, const int32_t* best_rank, const int32_t* best_kf,
                      const int32_t* cand_inliers, float* s_Tcw, float* s_mp, const uint8_t* s_valid, const int32_t* s_counts, float* kf_mp,
                      const uint8_t* kf_valid, const int32_t* kf_cnt, float* mp, const uint8_t* valid, const int32_t* key_counts, float* Tcw,
                      uint8_t* closed, int32_t* loop_kf, int32_t* loop_inliers) {
    return tb_launch(ctx, "k_vo_loop_adopt", k_vo_loop_adopt, dim3(nseq, nlive + 2), dim3(256), 0, cap, nlive, oldest, topk, pitch, before,
                     after, ecount, stats, best_rank, best_kf, cand_inliers, s_Tcw, s_mp, s_valid, s_counts, kf_mp, kf_valid, kf_cnt, mp, valid,
                     key_counts, Tcw, closed, loop_kf, loop_inliers);
}
