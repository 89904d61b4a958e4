/* Batched Sim(3) pose-graph optimisation (tb_pose_graph_sim3_batch_dev) -- extension, no reference counterpart: k_pgo.hip's solver
 * on the group that can change scale, the consumer of the Sim(3) edge that the Horn-RANSAC (k_sim3.hip) measures.
 *
 * One 256-thread workgroup per graph runs the whole Levenberg-Marquardt loop, so the call makes no host round trip. A graph has
 * up to 64 nodes S = (s, R, t) in k_sim3's FP64 srt layout (quaternion w x y z, t, s; the first nfixed held) and up to 256 edges
 * (a, b, Z, w_rot, w_trans, w_scale), Z ~ S_b S_a^-1. Residual r = Log(Z^-1 S_b S_a^-1) ordered (omega, upsilon, sigma), update
 * S <- Exp(delta) S, Jacobians J_b = Jl^-1(r) Ad(Z^-1), J_a = -Jl^-1(r) Ad(E) with Jl^-1 the fixed-length Bernoulli series of
 * tb_sim3.h, information diag(w_rot I3, w_trans I3, w_scale), no robust kernel, k_pgo's LM rule. With fixed_scale a free node has
 * the 6 unknowns (omega, upsilon) and its s keeps its bytes; the residual keeps its seventh component.
 * tests/pose_graph_sim3_reference.py is the same in numpy.
 *
 * The stages are k_pgo's, D = 7 (or 6) wide: one thread per edge linearises into the graph's scratch; one owner thread per (free
 * node, row, column) assembles in edge-list order, so there is no atomic; H + lambda I (up to 441 x 441, packed lower triangle) is
 * factorised by a right-looking panel Cholesky with the right-hand side riding as row N, the trailing update in 16 x 16 tiles on
 * the vector pipe; the back substitution walks the panels in reverse with one fixed-shape block sum each. Every sum has a fixed
 * shape, so a graph gives the same bits alone, in any batch and from run to run.
 *
 * The panel is PG3_PANEL = 7 columns, one node: 442 rows x 7 is 24.2 KB and the whole of the kernel's LDS 47.5 KB, static and
 * below the 64 KB a kernel gets without asking. A two-node panel (49.5 KB, 73 KB in all) would halve the dependent panel steps
 * but needs the raised dynamic limit, which costs occupancy beside other kernels for a solver that runs once per loop closure.
 *
 * Bound: latency, as k_pgo (a dependent chain of N / PG3_PANEL panel steps per trial); nothing here is tuned.
 */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_sim3.h"

#define PG3_T 256
#define PG3_MAX_NODES 64
#define PG3_MAX_EDGES 256
#define PG3_PANEL 7   /* columns of one panel: one node */
#define PG3_TILE 16   /* the trailing update's tile */
#define PG3_MAX_N (7 * (PG3_MAX_NODES - 1))

static_assert(sizeof(tb_pg_sim3_edge) == 96, "tb_pg_sim3_edge layout");

struct Pg3Shared {
    PoSim3 cur[PG3_MAX_NODES], trial[PG3_MAX_NODES];
    int ea[PG3_MAX_EDGES], eb[PG3_MAX_EDGES];
    double wr[PG3_MAX_EDGES], wt[PG3_MAX_EDGES], ws[PG3_MAX_EDGES];
    double g[PG3_MAX_N], x[PG3_MAX_N];
    double pan[(PG3_MAX_N + 1) * PG3_PANEL];
    double red[4 * PG3_PANEL];
    int ok;
};

__device__ __forceinline__ size_t pg3_tri(int i) { return (size_t)i * (i + 1) / 2; } /* first entry of packed row i */

/* an srt record (w x y z, t, s) as an element, its quaternion normalised */
__device__ inline PoSim3 pg3_from_srt(const double* v) {
    PoSim3 S;
    S.T.qw = v[0]; S.T.qx = v[1]; S.T.qy = v[2]; S.T.qz = v[3];
    S.T.tx = v[4]; S.T.ty = v[5]; S.T.tz = v[6];
    S.s = v[7];
    po_normalize(S.T);
    return S;
}
/* finite entries, a quaternion of positive finite norm, a scale above 0 */
__device__ inline bool pg3_srt_ok(const double* v) {
    bool f = true;
    for (int i = 0; i < 8; i++) f = f && isfinite(v[i]);
    const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    return f && n2 > 0 && isfinite(n2) && v[7] > 0;
}

/* Zi = Z^-1 and E = Z^-1 S_b S_a^-1 of one edge */
__device__ inline void pg3_edge_E(const tb_pg_sim3_edge& ed, const PoSim3* S, PoSim3& Zi, PoSim3& E) {
    Zi = s3_inverse(pg3_from_srt(ed.srt));
    E = s3_mul(Zi, s3_mul(S[ed.b], s3_inverse(S[ed.a])));
}

/* chi2 of the nodes S: the block's sum over its edges; the same value in every thread */
__device__ inline double pg3_chi2(const tb_pg_sim3_edge* edges, int E, const PoSim3* S, double* red) {
    double c[1] = {0.0};
    for (int e = threadIdx.x; e < E; e += PG3_T) {
        const tb_pg_sim3_edge ed = edges[e];
        PoSim3 Zi, Ee;
        pg3_edge_E(ed, S, Zi, Ee);
        double r[7];
        s3_log(Ee, r);
        c[0] += (ed.w_rot * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + ed.w_trans * (r[3] * r[3] + r[4] * r[4] + r[5] * r[5])) +
                ed.w_scale * (r[6] * r[6]);
    }
    po_block_sum<1>(c, red);
    return c[0];
}

__global__ void __launch_bounds__(PG3_T)
k_pgo_sim3(int nnodes, int nfixed, int fixed_scale, double* __restrict__ nodesAll, const tb_pg_sim3_edge* __restrict__ edgesAll,
           const int32_t* __restrict__ counts, int edge_pitch, int iters, double* __restrict__ statsAll, double* __restrict__ work,
           size_t work_per_graph) {
    __shared__ Pg3Shared S;
    const int gi = blockIdx.x, tid = threadIdx.x;
    const int D = fixed_scale ? 6 : 7;
    const int nfree = nnodes - nfixed, N = D * nfree, M = N + 1;
    double* nodes = nodesAll + (size_t)gi * nnodes * 8;
    const tb_pg_sim3_edge* edges = edgesAll + (size_t)gi * edge_pitch;
    double* stats = statsAll ? statsAll + 8 * (size_t)gi : nullptr;
    double* H = work + (size_t)gi * work_per_graph;   /* packed lower triangle, N rows */
    double* L = H + pg3_tri(N);                       /* the same with lambda, and the right-hand side as row N */
    double* Jc = L + pg3_tri(M);                      /* [edge_pitch][2][49] J_a, J_b */
    double* rc = Jc + (size_t)edge_pitch * 98;        /* [edge_pitch][7] */
    const int E = counts[gi];

    /* the check: a graph that fails it keeps every byte */
    int bad = (E < 0 || E > edge_pitch) ? 1 : 0;
    if (tid < nnodes && !pg3_srt_ok(nodes + 8 * tid)) bad = 1;
    if (!bad)
        for (int e = tid; e < E; e += PG3_T) {
            const tb_pg_sim3_edge ed = edges[e];
            const bool f = isfinite(ed.w_rot) && isfinite(ed.w_trans) && isfinite(ed.w_scale) && ed.w_rot >= 0 && ed.w_trans >= 0 &&
                           ed.w_scale >= 0 && pg3_srt_ok(ed.srt);
            if (!f || ed.a < 0 || ed.a >= nnodes || ed.b < 0 || ed.b >= nnodes || ed.a == ed.b) bad = 1;
        }
    bad = __syncthreads_or(bad);
    if (bad || E == 0) {
        if (stats && tid < 8) stats[tid] = (bad && tid == 7) ? -1.0 : 0.0;
        return;
    }
    for (int e = tid; e < E; e += PG3_T) {
        S.ea[e] = edges[e].a; S.eb[e] = edges[e].b;
        S.wr[e] = edges[e].w_rot; S.wt[e] = edges[e].w_trans; S.ws[e] = edges[e].w_scale;
    }
    if (tid < nnodes) {
        S.cur[tid] = pg3_from_srt(nodes + 8 * tid);
        S.trial[tid] = S.cur[tid];
    }
    __syncthreads();
    double cur = pg3_chi2(edges, E, S.cur, S.red);
    const double chi0 = cur;
    double lambda = 0.0, nu = 2.0;
    int done = 0, trials = 0, accepted_any = 0;
    bool ok = true;

    for (int iter = 0; iter < iters && ok; iter++) {
        /* linearise */
        for (int e = tid; e < E; e += PG3_T) {
            const tb_pg_sim3_edge ed = edges[e];
            PoSim3 Zi, Ee;
            pg3_edge_E(ed, S.cur, Zi, Ee);
            double r[7], Ji[49], A[49];
            s3_log(Ee, r);
            s3_jl_inv(r, Ji);
            for (int i = 0; i < 7; i++) rc[(size_t)e * 7 + i] = r[i];
            double* Ja = Jc + (size_t)e * 98;
            s3_adjoint(Ee, A);
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) {
                    double s = 0.0;
                    for (int k = 0; k < 7; k++) s += Ji[i * 7 + k] * A[k * 7 + j];
                    Ja[i * 7 + j] = -s;
                }
            s3_adjoint(Zi, A);
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) {
                    double s = 0.0;
                    for (int k = 0; k < 7; k++) s += Ji[i * 7 + k] * A[k * 7 + j];
                    Ja[49 + i * 7 + j] = s;
                }
        }
        for (size_t i = tid; i < pg3_tri(N); i += PG3_T) H[i] = 0.0;
        __syncthreads();
        /* assemble: item = (free node, row, column) of the D x D blocks; edges in list order */
        for (int item = tid; item < D * D * nfree; item += PG3_T) {
            const int nf = item / (D * D), r = (item % (D * D)) / D, c = item % D, node = nf + nfixed;
            const int row = D * nf + r;
            double diag = 0.0, gs = 0.0;
            for (int e = 0; e < E; e++) {
                const int a = S.ea[e], b = S.eb[e];
                if (a != node && b != node) continue;
                const double* Ji = Jc + (size_t)e * 98 + (a == node ? 0 : 49);
                const double* Jo = Jc + (size_t)e * 98 + (a == node ? 49 : 0);
                const int o = a == node ? b : a;
                const double wr = S.wr[e], wt = S.wt[e], ws = S.ws[e];
                double d = 0.0;
                for (int k = 0; k < 7; k++) d += Ji[k * 7 + r] * ((k < 3 ? wr : k < 6 ? wt : ws) * Ji[k * 7 + c]);
                diag += d;
                if (c == 0) {
                    double s = 0.0;
                    for (int k = 0; k < 7; k++) s += Ji[k * 7 + r] * ((k < 3 ? wr : k < 6 ? wt : ws) * rc[(size_t)e * 7 + k]);
                    gs -= s;
                }
                if (o >= nfixed && o < node) {
                    double s = 0.0;
                    for (int k = 0; k < 7; k++) s += Ji[k * 7 + r] * ((k < 3 ? wr : k < 6 ? wt : ws) * Jo[k * 7 + c]);
                    H[pg3_tri(row) + D * (o - nfixed) + c] += s;
                }
            }
            if (c <= r) H[pg3_tri(row) + D * nf + c] = diag;
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
            for (size_t i = tid; i < pg3_tri(N); i += PG3_T) L[i] = H[i];
            __syncthreads();   /* S.x: the diagonal's readers are done; L: the diagonal's writers come after the copy */
            for (int i = tid; i < N; i += PG3_T) {
                L[pg3_tri(i) + i] += lambda;
                L[pg3_tri(N) + i] = S.g[i];
            }
            if (tid == 0) S.ok = 1;
            __syncthreads();
            /* right-looking Cholesky, PG3_PANEL columns at a time */
            bool solved = true;
            for (int k0 = 0; k0 < N; k0 += PG3_PANEL) {
                const int pw = min(PG3_PANEL, N - k0), below = k0 + pw;
                for (int i = tid; i < (M - k0) * PG3_PANEL; i += PG3_T) {
                    const int row = k0 + i / PG3_PANEL, c = i % PG3_PANEL;
                    S.pan[i] = (c < pw && k0 + c <= row) ? L[pg3_tri(row) + k0 + c] : 0.0;
                }
                __syncthreads();
                if (tid == 0) {
                    for (int j = 0; j < pw; j++) {
                        double d = S.pan[j * PG3_PANEL + j];
                        for (int k = 0; k < j; k++) d -= S.pan[j * PG3_PANEL + k] * S.pan[j * PG3_PANEL + k];
                        if (!(d > 0) || !isfinite(d)) { S.ok = 0; break; }
                        d = sqrt(d);
                        S.pan[j * PG3_PANEL + j] = d;
                        for (int i = j + 1; i < pw; i++) {
                            double s = S.pan[i * PG3_PANEL + j];
                            for (int k = 0; k < j; k++) s -= S.pan[i * PG3_PANEL + k] * S.pan[j * PG3_PANEL + k];
                            S.pan[i * PG3_PANEL + j] = s / d;
                        }
                    }
                }
                __syncthreads();
                if (!S.ok) { solved = false; break; }
                for (int row = below + tid; row < M; row += PG3_T) {
                    double* p = S.pan + (row - k0) * PG3_PANEL;
                    for (int c = 0; c < pw; c++) {
                        double s = p[c];
                        for (int k = 0; k < c; k++) s -= p[k] * S.pan[c * PG3_PANEL + k];
                        p[c] = s / S.pan[c * PG3_PANEL + c];
                    }
                }
                __syncthreads();
                for (int i = tid; i < (M - k0) * PG3_PANEL; i += PG3_T) {
                    const int row = k0 + i / PG3_PANEL, c = i % PG3_PANEL;
                    if (c < pw && k0 + c <= row) L[pg3_tri(row) + k0 + c] = S.pan[i];
                }
                /* trailing update in PG3_TILE x PG3_TILE tiles of the lower triangle (rows below..M-1, columns below..N-1) */
                const int ty = tid / PG3_TILE, tx = tid % PG3_TILE;
                const int nt = (M - below + PG3_TILE - 1) / PG3_TILE;
                for (int ti = 0; ti < nt; ti++)
                    for (int tj = 0; tj <= ti; tj++) {
                        const int row = below + ti * PG3_TILE + ty, col = below + tj * PG3_TILE + tx;
                        if (row < M && col <= row && col < N) {
                            const double* pi = S.pan + (row - k0) * PG3_PANEL;
                            const double* pj = S.pan + (col - k0) * PG3_PANEL;
                            double s = 0.0;
                            for (int c = 0; c < PG3_PANEL; c++) s += pi[c] * pj[c];
                            L[pg3_tri(row) + col] -= s;
                        }
                    }
                __syncthreads();
            }
            /* back substitution L' x = y, y = row N, the panels in reverse */
            if (solved) {
                const int np = (N + PG3_PANEL - 1) / PG3_PANEL;
                for (int p = np - 1; p >= 0; p--) {
                    const int k0 = p * PG3_PANEL, pw = min(PG3_PANEL, N - k0), below = k0 + pw;
                    double acc[PG3_PANEL];
                    for (int c = 0; c < PG3_PANEL; c++) acc[c] = 0.0;
                    for (int row = below + tid; row < N; row += PG3_T) {
                        const double xr = S.x[row];
                        for (int c = 0; c < PG3_PANEL; c++)
                            if (c < pw) acc[c] += L[pg3_tri(row) + k0 + c] * xr;
                    }
                    po_block_sum<PG3_PANEL>(acc, S.red);
                    if (tid == 0)
                        for (int c = pw - 1; c >= 0; c--) {
                            double s = L[pg3_tri(N) + k0 + c] - acc[c];
                            for (int k = c + 1; k < pw; k++) s -= L[pg3_tri(k0 + k) + k0 + c] * S.x[k0 + k];
                            S.x[k0 + c] = s / L[pg3_tri(k0 + c) + k0 + c];
                        }
                    __syncthreads();
                }
            } else {
                for (int i = tid; i < N; i += PG3_T) S.x[i] = 0.0;
                __syncthreads();
            }
            /* the trial: S <- Exp(delta) S; with the scale fixed sigma = 0, e^0 = 1 and s keeps its bits */
            if (tid >= nfixed && tid < nnodes) {
                double u[7];
                for (int i = 0; i < 7; i++) u[i] = i < D ? S.x[D * (tid - nfixed) + i] : 0.0;
                S.trial[tid] = s3_mul(s3_exp(u), S.cur[tid]);
            }
            __syncthreads();
            double trial = pg3_chi2(edges, E, S.trial, S.red);
            if (!solved) trial = 1.7976931348623157e308;
            double sc[1] = {0.0};
            for (int i = tid; i < N; i += PG3_T) sc[0] += S.x[i] * (lambda * S.x[i] + S.g[i]);
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
    /* fixed nodes and a graph that accepted no step keep their bytes; so does a held scale */
    if (accepted_any && tid >= nfixed && tid < nnodes) {
        double* v = nodes + 8 * tid;
        const PoSim3 o = S.cur[tid];
        v[0] = o.T.qw; v[1] = o.T.qx; v[2] = o.T.qy; v[3] = o.T.qz;
        v[4] = o.T.tx; v[5] = o.T.ty; v[6] = o.T.tz;
        if (!fixed_scale) v[7] = o.s;
    }
    if (stats && tid == 0) {
        stats[0] = done; stats[1] = chi0; stats[2] = cur; stats[3] = lambda; stats[4] = trials;
        stats[5] = stats[6] = stats[7] = 0.0;
    }
}

/* ---- the graph of a keyframe store's live keyframes and a query frame (tb_kf_store_sim3_graph_dev, tb_vo_loop_sim3_dev), by
 * k_vo_loop_graph's rules: the ring is counted for the whole batch, so the host knows which slots are live and their order; node
 * i < nlive is ring slot (oldest + i) % cap, node nlive the query frame, the other nodes the identity, which no edge names. Every
 * node is the quaternion form of a float32 Tcw with s = 1; the loop edge is the kept best_srt, copied byte for byte. Every output
 * of every slot is written by every call. */
__device__ inline PoSE3 pg3_pose_from_f32(const float* T) {
    double R[9], t[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i * 3 + j] = (double)T[i * 4 + j];
        t[i] = (double)T[i * 4 + 3];
    }
    return po_from_Rt(R, t);
}
__device__ inline void pg3_srt_write(double* v, const PoSE3& T) {
    v[0] = T.qw; v[1] = T.qx; v[2] = T.qy; v[3] = T.qz;
    v[4] = T.tx; v[5] = T.ty; v[6] = T.tz;
    v[7] = 1.0;
}

/* one 64-thread workgroup per sequence, thread i = node i and edge slot i (nn = cap + 1 <= 64) */
__global__ void __launch_bounds__(64)
k_sim3_graph(int cap, int nlive, int oldest, int frame_id, double w_rot, double w_trans, double w_scale, const float* __restrict__ s_Tcw,
             const int32_t* __restrict__ s_kf_ids, const float* __restrict__ q_Tcw, const int32_t* __restrict__ best_kf,
             const double* __restrict__ best_srt, double* __restrict__ before, double* __restrict__ after, int32_t* __restrict__ node_kf,
             int32_t* __restrict__ nnodes, tb_pg_sim3_edge* __restrict__ edges, int32_t* __restrict__ ecount) {
    const int s = blockIdx.x, i = threadIdx.x, nn = cap + 1;
    if (i >= nn) return;
    const float* Tkf = s_Tcw + (size_t)s * cap * 16;
    const int32_t* ids = s_kf_ids + (size_t)s * cap;
    auto node_pose = [&](int n) { return n < nlive ? Tkf + (size_t)((oldest + n) % cap) * 16 : q_Tcw + (size_t)s * 16; };
    double* pb = before + ((size_t)s * nn + i) * 8;
    double* pa = after + ((size_t)s * nn + i) * 8;
    if (i <= nlive) {
        const PoSE3 T = pg3_pose_from_f32(node_pose(i));
        pg3_srt_write(pb, T);
        pg3_srt_write(pa, T);
        node_kf[(size_t)s * nn + i] = i < nlive ? ids[(oldest + i) % cap] : frame_id;
    } else {
        for (int k = 0; k < 8; k++) pb[k] = pa[k] = (k == 0 || k == 7) ? 1.0 : 0.0;
        node_kf[(size_t)s * nn + i] = -1;
    }
    const bool loop = best_kf[s] >= 0 && nlive >= 2;
    if (i == 0) {
        nnodes[s] = nlive + 1;
        ecount[s] = loop ? nlive + 1 : 0;
    }
    tb_pg_sim3_edge e;
    e.a = e.b = 0;
    for (int k = 0; k < 8; k++) e.srt[k] = 0.0;
    e.w_rot = e.w_trans = e.w_scale = 0.0;
    if (loop && i < nlive) {   /* odometry: node i -> node i + 1, Z = S_next S_prev^-1 at s = 1 */
        e.a = i; e.b = i + 1;
        pg3_srt_write(e.srt, po_mul(pg3_pose_from_f32(node_pose(i + 1)), po_inverse(pg3_pose_from_f32(node_pose(i)))));
        e.w_rot = w_rot; e.w_trans = w_trans; e.w_scale = w_scale;
    } else if (loop && i == nlive) {   /* the loop edge: the winning keyframe's node -> the frame's node; a keyframe the ring no
                                        * longer holds leaves a = -1, which the solver flags */
        int j = -1;
        for (int n = 0; n < nlive; n++)
            if (ids[(oldest + n) % cap] == best_kf[s]) j = n;
        e.a = j; e.b = nlive;
        for (int k = 0; k < 8; k++) e.srt[k] = best_srt[8 * (size_t)s + k];
        e.w_rot = w_rot; e.w_trans = w_trans; e.w_scale = w_scale;
    }
    edges[(size_t)s * nn + i] = e;
}

int tbk_sim3_graph(tb_ctx* ctx, int nseq, int cap, int nlive, int oldest, int frame_id, double w_rot, double w_trans, double w_scale,
                   const float* s_Tcw, const int32_t* s_kf_ids, const float* q_Tcw, const int32_t* best_kf, const double* best_srt,
                   double* before, double* after, int32_t* node_kf, int32_t* nnodes, tb_pg_sim3_edge* edges, int32_t* ecount) {
    return tb_launch(ctx, "k_sim3_graph", k_sim3_graph, dim3(nseq), dim3(64), 0, cap, nlive, oldest, frame_id, w_rot, w_trans, w_scale, s_Tcw,
                     s_kf_ids, q_Tcw, best_kf, best_srt, before, after, node_kf, nnodes, edges, ecount);
}

/* doubles of scratch one graph takes: H, L with its extra row (both at 7 unknowns a node, whatever fixed_scale says, so that one plan
 * serves both), the edges' Jacobians and residuals */
static size_t pg3_work_doubles(int nnodes, int nfixed, int edge_pitch) {
    const size_t N = 7 * (size_t)(nnodes - nfixed);
    return N * (N + 1) / 2 + (N + 1) * (N + 2) / 2 + (size_t)edge_pitch * 105;
}

size_t tbk_pose_graph_sim3_work_bytes(int ngraphs, int nnodes, int nfixed, int edge_pitch) {
    return (size_t)ngraphs * pg3_work_doubles(nnodes, nfixed, edge_pitch) * sizeof(double);
}

int tbk_pose_graph_sim3_batch(tb_ctx* ctx, int ngraphs, int nnodes, int nfixed, int fixed_scale, double* d_nodes,
                              const tb_pg_sim3_edge* d_edges, const int32_t* d_counts, int edge_pitch, int iters, double* d_stats,
                              void* d_work) {
    return tb_launch(ctx, "k_pgo_sim3", k_pgo_sim3, dim3(ngraphs), dim3(PG3_T), 0, nnodes, nfixed, fixed_scale, d_nodes, d_edges, d_counts,
                     edge_pitch, iters, d_stats, (double*)d_work, pg3_work_doubles(nnodes, nfixed, edge_pitch));
}
