/* a17 -- multi-keyframe local bundle adjustment.  NORTH-STAR EXTENSION WITH NO REFERENCE COUNTERPART:
 * the reference's "LocalBA" only holds motion-only pose optimisation; BASELINE.json asks
 * for a 10-keyframe local BA with an MFMA Schur block-GEMM, so this stage is designed here and checked
 * against this repo's own FP64 CPU solver (oracle_local_ba), never against the reference.
 *
 * Problem: nkf SE(3) poses (first nfixed held), npt points, reprojection edges with Huber (delta^2 =
 * 5.991); g2o-style Levenberg-Marquardt (tau = 1e-5, rho-based lambda update, <= 10 trials per
 * iteration) on the Schur-reduced pose system.  A batch of W equally sized windows runs together.
 *
 * MI355X mapping: an LM trial is a "round" of eight kernels over all windows (no host round trips inside a round;
 * per-window LM state lives in HBM and every kernel skips finished windows). NOTHING PER EDGE IS STORED between the
 * passes: every consumer rebuilds the linearisation of an edge (ba_linearize: ww, residual, Jl, Jp) from its
 * 20-byte observation and the state -- ~150 FP64 operations against what used to be a 144-byte Hpl block per edge
 * and pass through HBM.
 *   A point pass    (thread per point)   chi2, Hll, bl; the point's record once lambda is final  -- after an accepted step
 *   B keyframe pass (block per free KF)  Hpp, bp as fixed-shape tree reductions                  -- "
 *   C reduce        chunk partials -> Hpp, bp, chi2, lambda_0
 *   C2 records      (thread per point)   A = Hll + lambda I = C C^T, U = C^-T (A^-1 = U U^T), bl, X -- when A could not
 *   D Schur         S' = sum_l Z_l Z_l^T, Z_l = Hpl_l U_l, on the FP64 matrix cores (v_mfma_f64_16x16x4): every
 *                   wavefront densifies its own 4-point chunks into a private LDS tile (lane = edge), both MFMA
 *                   operands come from that tile; reduced rhs = sum_l Z_l (U_l^T bl_l) on the vector ALU
 *   E solve         S = Hpp + lambda I - S', Cholesky in the registers of one wavefront, pose update through the exp map
 *   F point update  back-substitution xl = U (U^T (bl - sum_k Hpl^T x_k)), trial chi2
 *   G decide        rho, accept / reject, lambda update, termination
 * Every cross-thread sum has a fixed shape (per-block trees + ordered partial sums), so results are
 * reproducible run to run.  Bound: the FP64 units (matrix + vector work, same datapath on CDNA4) for D, FP64
 * VALU / latency for the rest; bench.py reports both roofs of D.
 */
#include <mutex>
#include <type_traits>
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_se3.h"
#include "tb_math.h"

#define BA_T 256
#ifndef BA_KFCH
#define BA_KFCH 512           /* edges per keyframe-pass chunk: the unit of a workgroup's share and of the oPartKF slots */
#endif
#ifndef BA_KFBLK
#define BA_KFBLK 1            /* workgroups per keyframe in the keyframe pass, each with a contiguous run of the keyframe's chunks: the
                                 whole list (1) 0.316 ms per 171-window call alone and 14.12 ms per 512-frame step, halves (2) 0.390
                                 and 14.51; the chunk-per-workgroup form this replaced 0.432 and 14.89 (profiles/ba_kf_pass_ab.json) */
#endif
#ifndef BA_KFE
#define BA_KFE 2              /* edges per thread and round of the keyframe pass (a thread's edges come in list order either way: the
                                 value changes the schedule, not a bit of the sums). 2: 128 VGPRs; 1: 106 VGPRs, 0.309 against
                                 0.316 ms alone and the same step time (14.19 against 14.17 in the same alternation) */
#endif
#ifndef BA_LIN_FUSE_ALL
#define BA_LIN_FUSE_ALL 0     /* 1: batches of more than 32 windows run the point and keyframe passes in one launch as well.
                                 Measured again with the pass at 9.6 KB of LDS: 0.761 against 0.316 + 0.490 ms alone, but 14.5-15.2
                                 against 14.0-14.1 ms per step: two launches stay */
#endif
#ifndef BA_KF_AHEAD
#define BA_KF_AHEAD 1         /* keyframe pass: the next round's points and the one after's records load while a round computes
                                 (0: load, gather, compute per round: 0.333 against 0.316 ms alone) */
#endif
#ifndef BA_KF_POSE_ONCE
#define BA_KF_POSE_ONCE 1     /* keyframe pass: one wavefront converts the keyframe's pose, the others read R|t from LDS (0: every
                                 thread converts, as before: 0.419 against 0.316 ms alone) */
#endif
#define BA_BIG_MAXF 64        /* free keyframes of a large window (6 bits of the free-edge key) */
#define BA_SMALL_MAXF 10      /* free keyframes of a window on the MFMA path (visibility patterns are 10-bit masks) */
#define BA_SORT_LDS 8192      /* points of a window whose pattern sort runs in LDS (k_ba_groups) */
#ifndef BA_EMAX
#define BA_EMAX 64            /* free-keyframe edges of a Schur group at most: one lane each */
#endif
#ifndef BA_UPD_BATCH
#define BA_UPD_BATCH 4        /* slots per fetch of k_ba_update's second walk */
#endif
#ifndef BA_PCAP
#define BA_PCAP 21            /* points of a Schur group at most (their 12-double records fill 252 of 256 staged doubles) */
#endif

struct BaState {
    double lambda, ni, currentChi, chi0, scale_p, rho;
    int iter, qmax, status, need_lin, cur, ok2, done_iters, err;
    int sing, pad0, hq_fresh, pad2; /* hq_fresh: the point pass of this trial already wrote the point records;
                                       sing: a point block was not positive definite in this trial (solve fails, as in the CPU solver) */
};

struct BaDims {
    int W, nkf, nfixed, nfree, np, npt, obs_pitch, iters;
    int nblkP, kfChunks, G, nChunks; /* G: most Schur workgroups a window has */
    int Gbase, Gextra;               /* small batches (wgReduce): window w has Gbase + (w < Gextra) Schur workgroups */
    int Vbase, Vextra;               /* otherwise window w has Vbase + (w < Vextra) Schur WAVEFRONTS, dealt to the windows one by one
                                        (a workgroup's four may belong to two windows): one resident round over the batch */
    int big, npairs;             /* more than 10 free keyframes: the block-pair Schur / panel solve kernels */
    unsigned long long oBigA;    /* large windows: the reduced system [np + 1][np] (row np = rhs) */
    unsigned long long oPairStart, oPairCnt, oPairItems, maxItems; /* ints: block-pair item lists */
    double fx, fy, cx, cy;
    /* per-window offsets, in doubles, into the double workspace */
    unsigned long long wstride, oT, oP, oHll, oBl, oHq, oHpp, oBp, oXp, oPartKF, oPartP, oPartS;
    /* per-window offsets, in ints, into the int workspace */
    unsigned long long istride, oPtStart, oPtFree, oKfStart, oKfEdges, oFreeKP;
    unsigned long long oKfRec;   /* ints: 16-byte records {pt, u, v, inv_sigma2} of every edge in keyframe order (the keyframe pass) */
    /* ints, windows on the MFMA path (k_ba_groups): visibility mask per point, the two permutation buffers of the pattern
     * sort, rank of every point in pattern order (its record's slot in Hq; identity for large windows), the free-keyframe
     * edge records in pattern order (4 ints each), the group descriptors (int4 each, count at [4 npt]) */
    unsigned long long oPtMask, oPermA, oPermB, oPtRank, oKPs, oGDesc;
    unsigned long long oGCost;   /* ints: cost estimate of the groups before group g (exclusive prefix, total at [ng]) */
    unsigned long long oGCut;    /* ints: first group of Schur wavefront v of the window (4 G + 1 entries) */
    int renum;                   /* k_ba_rank renumbered the window's points in visibility-pattern order: every later kernel works on
                                    the renumbered copy of the observations, ranks are the identity */
    unsigned long long oPerm;    /* ints (renum): old index of the point that is now r */
    int stream;                  /* renum, unless tb_debug_ba_plain_obs: the point passes read the lane-interleaved observation stream
                                    (ba_stream_walk) that k_ba_prepare writes at oFreeKP -- a region only the windows it does not
                                    serve use (k_ba_setup's free-edge records for k_ba_groups and the block-pair kernels) */
    int schurWaveLds;            /* doubles of LDS per Schur wavefront (host: ba_c_wave_lds(nfree)) */
    int wgReduce;                /* Schur workgroups add their four wavefronts' partial systems through LDS (small batches: many
                                    workgroups per window, and k_ba_solve -- one workgroup per window -- adds them all) */
};

/* Schur wavefronts of window w, and the window / wavefront-in-window of the batch's u-th unit (units: wavefronts, or
 * workgroups when wgReduce): windows below `extra` have base + 1 units, the others base */
__host__ __device__ inline int ba_schur_waves(const BaDims& d, int w) {
    return d.wgReduce ? 4 * (d.Gbase + (w < d.Gextra ? 1 : 0)) : d.Vbase + (w < d.Vextra ? 1 : 0);
}
__device__ __forceinline__ void ba_schur_unit(int u, int base, int extra, int& w, int& i) {
    const int head = extra * (base + 1);
    if (u < head) { w = u / (base + 1); i = u - w * (base + 1); }
    else { const int r = u - head; w = extra + r / base; i = r - (w - extra) * base; }
}

typedef double ba_d4 __attribute__((ext_vector_type(4)));
typedef double ba_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double ba_huber_rho0(double c, double delta) {
    const double dsqr = delta * delta;
    return (c <= dsqr) ? c : 2 * sqrt(c) * delta - dsqr;
}
/* Linearisation of one observation at (Tk, X): Huber-weighted information ww, residual (e0, e1), the 2x3 point
 * Jacobian Jl and camera-frame point pc (for ba_jac_pose_iz). ONE definition for every kernel that needs Hpl =
 * ww Jp^T Jl: the blocks are never stored, the point pass, the Schur kernel and the back-substitution each rebuild
 * what they need from the 20-byte observation, and must agree bit for bit. */
struct BaLin { double ww, e0, e1, c2, invz; double pc[3]; double Jl[6]; };
/* The helpers below spell out their fused multiply-adds (the library builds with -ffp-contract=off for the
 * reference-facing float paths; here every product-sum is an explicit fma, ~140 FP64 instructions per edge instead of
 * ~215 separate multiplies and adds -- they run on the same FP64 units as the MFMAs) and use ONE reciprocal per edge:
 * v_rcp_f64 refined by two Newton steps (relative error ~1e-16; the IEEE division sequence is a dozen instructions
 * around the same quarter-rate v_rcp_f64). Every kernel calls the same helpers, so they agree bit for bit. */
__device__ __forceinline__ double ba_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
/* residual and Huber-weighted information of one observation */
__device__ __forceinline__ void ba_residual(const double* Rt, const double* X, float u, float v, float inv_sigma2, double fx,
                                            double fy, double cx, double cy, double delta, BaLin& L) {
#pragma unroll
    for (int i = 0; i < 3; i++) L.pc[i] = fma(Rt[3 * i + 2], X[2], fma(Rt[3 * i + 1], X[1], fma(Rt[3 * i], X[0], Rt[9 + i])));
    L.invz = ba_rcp(L.pc[2]);
    L.e0 = (double)u - fma(L.pc[0] * L.invz, fx, cx);
    L.e1 = (double)v - fma(L.pc[1] * L.invz, fy, cy);
    const double wgt = (double)inv_sigma2;
    L.c2 = fma(L.e0, wgt * L.e0, L.e1 * (wgt * L.e1));
    const double r1 = (L.c2 <= delta * delta) ? 1.0 : delta / sqrt(L.c2);
    L.ww = r1 * wgt;
}
__device__ __forceinline__ void ba_linearize(const double* Rt, const double* X, float u, float v, float inv_sigma2, double fx,
                                             double fy, double cx, double cy, double delta, BaLin& L) {
    ba_residual(Rt, X, u, v, inv_sigma2, fx, fy, cx, cy, delta, L);
    const double ax = -(L.pc[0] * L.invz) * fx, ay = -(L.pc[1] * L.invz) * fy, m = -L.invz;
#pragma unroll
    for (int c = 0; c < 3; c++) { /* Jl = -1/z [fx 0 -x/z fx; 0 fy -y/z fy] R */
        L.Jl[c] = m * fma(ax, Rt[6 + c], fx * Rt[c]);
        L.Jl[3 + c] = m * fma(ay, Rt[6 + c], fy * Rt[3 + c]);
    }
}
/* keyframe pose as the passes use it: rotation matrix (row major) and translation, 12 doubles. Every kernel converts
 * the stored unit quaternion once per workgroup instead of once per edge. */
__device__ __forceinline__ void ba_pose_to_Rt(const double* T7, double* Rt) {
    PoSE3 s;
    s.qx = T7[0]; s.qy = T7[1]; s.qz = T7[2]; s.qw = T7[3]; s.tx = T7[4]; s.ty = T7[5]; s.tz = T7[6];
    po_to_R(s, Rt);
    Rt[9] = s.tx; Rt[10] = s.ty; Rt[11] = s.tz;
}
/* a value every lane of the wavefront holds alike, moved to scalar registers (two v_readfirstlane_b32) */
__device__ __forceinline__ double ba_uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
/* d(projection)/d(pose increment), 2 x 6, rows at J[0..5] and J[6..11] (g2o EdgeSE3ProjectXYZ convention) */
__device__ __forceinline__ void ba_jac_pose_iz(const double* pc, double invz, double fx, double fy, double* J) {
    const double xz = pc[0] * invz, yz = pc[1] * invz, xf = xz * fx, yf = yz * fy; /* x/z, y/z, fx x/z, fy y/z */
    J[0] = xf * yz; J[1] = -fma(xf, xz, fx); J[2] = yz * fx;
    J[3] = -invz * fx; J[4] = 0; J[5] = xf * invz;
    J[6] = fma(yf, yz, fy); J[7] = -(xz * yf); J[8] = -xz * fy;
    J[9] = 0; J[10] = -invz * fy; J[11] = yf * invz;
}

__device__ __forceinline__ bool ba_inv3(const double* H6, double lambda, double* I) {
    /* H6 = xx, xy, xz, yy, yz, zz of the symmetric Hll block */
    const double A0 = H6[0] + lambda, A1 = H6[1], A2 = H6[2], A4 = H6[3] + lambda, A5 = H6[4], A8 = H6[5] + lambda;
    const double A3 = A1, A6 = A2, A7 = A5;
    const double det = A0 * (A4 * A8 - A5 * A7) - A1 * (A3 * A8 - A5 * A6) + A2 * (A3 * A7 - A4 * A6);
    if (!(fabs(det) > 0)) return false;
    const double id = 1.0 / det;
    I[0] = (A4 * A8 - A5 * A7) * id; I[1] = (A2 * A7 - A1 * A8) * id; I[2] = (A1 * A5 - A2 * A4) * id;
    I[3] = (A5 * A6 - A3 * A8) * id; I[4] = (A0 * A8 - A2 * A6) * id; I[5] = (A2 * A3 - A0 * A5) * id;
    I[6] = (A3 * A7 - A4 * A6) * id; I[7] = (A1 * A6 - A0 * A7) * id; I[8] = (A0 * A4 - A1 * A3) * id;
    return true;
}
__device__ __forceinline__ PoSE3 ba_load_se3(const double* p) {
    PoSE3 s;
    s.qx = p[0]; s.qy = p[1]; s.qz = p[2]; s.qw = p[3]; s.tx = p[4]; s.ty = p[5]; s.tz = p[6];
    return s;
}
__device__ __forceinline__ void ba_store_se3(double* p, const PoSE3& s) {
    p[0] = s.qx; p[1] = s.qy; p[2] = s.qz; p[3] = s.qw; p[4] = s.tx; p[5] = s.ty; p[6] = s.tz;
}
__device__ __forceinline__ double ba_block_sum1(double v, double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = po_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double ba_block_max1(double v, double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

/* Ordered compaction of the edges [0, n) that satisfy pred, by one 256-thread workgroup without a barrier per slab:
 * every wavefront owns a contiguous quarter of the range; pass 1 counts (independent loads), one barrier gives each
 * quarter its base rank, pass 2 ranks with ballots, four independent 64-edge groups per trip. visit(e, rank, hit) is
 * called for EVERY edge with the number of hits before it. Returns the total number of hits. tmp: >= 8 ints of LDS. */
template <class Pred, class Pred2, class Visit>
__device__ __forceinline__ int ba_ordered_rank(int n, int* tmp, Pred pred, Pred2 pred2, int* total2, Visit visit) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = (((n + 3) >> 2) + 63) & ~63, lo = min(wave * q, n), hi = min(lo + q, n);
    int cnt = 0, cnt2 = 0; /* pred2: a second class counted over the whole range in the same pass (total2) */
    for (int e0 = lo; e0 < hi; e0 += 256) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = e0 + 64 * i + lane;
            cnt += (e < hi && pred(e)) ? 1 : 0;
            cnt2 += (e < hi && pred2(e)) ? 1 : 0;
        }
    }
    cnt = tb_wave_sum(cnt);
    cnt2 = tb_wave_sum(cnt2);
    if (lane == 0) { tmp[wave] = cnt; tmp[4 + wave] = cnt2; }
    __syncthreads();
    int base = 0;
    for (int v = 0; v < wave; v++) base += tmp[v];
    const int total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    *total2 = tmp[4] + tmp[5] + tmp[6] + tmp[7];
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int e0 = lo; e0 < hi; e0 += 256) {
        bool f[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const int e = e0 + 64 * i + lane; f[i] = e < hi && pred(e); }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = e0 + 64 * i + lane;
            const unsigned long long m = __ballot(f[i]);
            if (e < hi) visit(e, base + __popcll(m & lt), f[i]);
            base += __popcll(m);
        }
    }
    __syncthreads(); /* tmp may be reused */
    return total;
}

/* ---- setup: CSR by point (observations must be grouped by ascending point index) and by keyframe.
 * grid (nkf + 2, W): block k < nkf lists keyframe k's edges in ascending edge order (its base offset is
 * the count of edges with a smaller keyframe index, recounted per block so blocks stay independent);
 * block nkf initialises the LM state, checks the input, builds ptStart and converts poses / points;
 * block nkf + 1 numbers the free-keyframe edges compactly (16-byte edge records, ptFree). */
__global__ void __launch_bounds__(BA_T)
k_ba_setup(BaDims d, const float* __restrict__ poses, const float* __restrict__ pts, const tb_ba_obs* __restrict__ obsOrig,
           const tb_ba_obs* __restrict__ obsAll, const int32_t* __restrict__ obsCounts, double* __restrict__ dw, int* __restrict__ iw,
           BaState* __restrict__ states, int* __restrict__ errflag) {
    __shared__ int tmp[8];
    const int w = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    /* obsOrig: the caller's observations (checked here); obsAll: what the passes read -- the same, or k_ba_rank's renumbered
     * copy, which is exact whenever the check passes and merely in range when it does not (the window is then skipped) */
    const tb_ba_obs* obs = obsOrig + (size_t)w * d.obs_pitch;
    const int nobs = min(obsCounts[w], d.obs_pitch);
    double* D = dw + (size_t)w * d.wstride;
    int* I = iw + (size_t)w * d.istride;
    BaState* st = states + w;
    {   /* input check, a slice of the edges per block (errflag[w] was zeroed before the launch; k_ba_points turns it
         * into the window's status): indices in range, grouped by ascending point, and a point observed at most once
         * per keyframe (the Schur tile holds one 6 x 3 block per (keyframe, point); within a sorted run the first
         * repeat lies at most nkf edges after its earlier occurrence). The look-back loads are issued eight at a time
         * without looking at them in between -- a compare-and-continue loop is one memory latency per step. */
        const int nb = gridDim.x, per = (nobs + nb - 1) / nb;
        bool bad = false;
        for (int e = k * per + tid; e < min((k + 1) * per, nobs); e += BA_T) {
            const tb_ba_obs o = obs[e];
            if (o.kf < 0 || o.kf >= d.nkf || o.pt < 0 || o.pt >= d.npt || (e > 0 && o.pt < obs[e - 1].pt)) bad = true;
            for (int b0 = 1; b0 <= d.nkf && b0 <= e; b0 += 8) {
                int pk[8], pp[8];
#pragma unroll
                for (int i = 0; i < 8; i++) { const int ee = max(e - b0 - i, 0); pk[i] = obs[ee].kf; pp[i] = obs[ee].pt; }
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if (b0 + i <= d.nkf && b0 + i <= e && pp[i] == o.pt && pk[i] == o.kf) bad = true;
                if (pp[7] != o.pt) break; /* left the point's run */
            }
        }
        if (bad) errflag[w] = 1; /* benign race: every writer stores 1 */
    }
    obs = obsAll + (size_t)w * d.obs_pitch;
    if (d.renum && k != d.nkf) return; /* k_ba_prepare built the lists of this window */
    if (k < d.nkf) {
        /* keyframe k's edges in ascending edge order, placed behind the edges of the keyframes before it */
        int base = 0;
        const int mine = ba_ordered_rank(nobs, tmp, [&](int e) { return obs[e].kf == k; },
                                         [&](int e) { const int kf = obs[e].kf; return kf >= 0 && kf < k; }, &base,
                                         [&](int e, int rank, bool hit) {
                                             if (hit) {   /* the edge's index, and its observation as the keyframe pass reads it */
                                                 I[d.oKfEdges + base + rank] = e;
                                                 const tb_ba_obs o = obs[e];
                                                 int4 r;
                                                 r.x = o.pt; r.y = __float_as_int(o.u); r.z = __float_as_int(o.v); r.w = __float_as_int(o.inv_sigma2);
                                                 *reinterpret_cast<int4*>(I + d.oKfRec + 4 * (size_t)(base + rank)) = r;
                                             }
                                         });
        if (tid == 0) {
            I[d.oKfStart + k] = base;
            if (k == d.nkf - 1) I[d.oKfStart + d.nkf] = base + mine;
        }
        return;
    }
    if (k == d.nkf + 1) {
        /* compact numbering of the free-keyframe edges (the only ones that enter the Schur complement): ce = rank among
         * the free edges in edge order, so a point's / a chunk's free edges are contiguous in the record list
         * freeKP[ce] = {pt << 6 | free keyframe index, u, v, inv_sigma2}; ptFree[p] = first compact edge of point p */
        int unused = 0;
        const int nfreeE = ba_ordered_rank(nobs, tmp, [&](int e) { return obs[e].kf >= d.nfixed; }, [](int) { return false; }, &unused,
            [&](int e, int ce, bool hit) {
                /* points whose first edge is this one (observations are grouped by ascending point) */
                const int prev = (e > 0) ? obs[e - 1].pt : -1, cur = obs[e].pt;
                for (int p = max(prev + 1, 0); p <= min(cur, d.npt); p++) I[d.oPtFree + p] = ce;
                if (hit) { /* 16-byte record of the free-keyframe edge: key, pixel, information scale */
                    const tb_ba_obs o = obs[e];
                    int4 r;
                    r.x = (int)(((unsigned)cur << 6) | ((unsigned)(o.kf - d.nfixed) & 63u));
                    r.y = __float_as_int(o.u); r.z = __float_as_int(o.v); r.w = __float_as_int(o.inv_sigma2);
                    *reinterpret_cast<int4*>(I + d.oFreeKP + 4 * (size_t)ce) = r;
                }
            });
        for (int p = max((nobs > 0 ? obs[nobs - 1].pt : -1) + 1, 0) + tid; p <= d.npt; p += BA_T) I[d.oPtFree + p] = nfreeE;
        return;
    }
    if (tid == 0) {
        st->lambda = 0; st->ni = 2; st->currentChi = 0; st->chi0 = 0; st->scale_p = 0; st->rho = 0;
        st->iter = 0; st->qmax = 0; st->status = (d.iters > 0 && nobs > 0) ? 0 : 1; st->need_lin = 1; st->cur = 0; st->ok2 = 1;
        st->done_iters = 0; st->err = 0; st->sing = 0; st->hq_fresh = 0;
    }
    __syncthreads();
    if (!d.renum) {
        for (int e = tid; e < nobs; e += BA_T) { /* ptStart[p] = first edge with pt >= p: the points whose first edge is e */
            const int prev = (e > 0) ? obs[e - 1].pt : -1, cur = obs[e].pt;
            for (int p = max(prev + 1, 0); p <= min(cur, d.npt); p++) I[d.oPtStart + p] = e;
        }
        for (int p = max((nobs > 0 ? obs[nobs - 1].pt : -1) + 1, 0) + tid; p <= d.npt; p += BA_T) I[d.oPtStart + p] = nobs;
        if (d.big) for (int p = tid; p < d.npt; p += BA_T) I[d.oPtRank + p] = p; /* large windows keep the point records in point order */
    }
    for (int kk = tid; kk < d.nkf; kk += BA_T) {
        const float* T = poses + ((size_t)w * d.nkf + kk) * 16;
        double R[9], t[3];
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[i * 3 + j] = (double)T[i * 4 + j]; t[i] = (double)T[i * 4 + 3]; }
        const PoSE3 s = po_from_Rt(R, t);
        ba_store_se3(D + d.oT + (size_t)kk * 7, s);
        ba_store_se3(D + d.oT + (size_t)(d.nkf + kk) * 7, s);
    }
    for (int i = tid; i < d.npt * 3; i += BA_T) {
        const int r = i / 3, c = i - 3 * r;
        const double v = (double)pts[(size_t)w * d.npt * 3 + (d.renum ? 3 * (size_t)I[d.oPerm + r] + c : (size_t)i)];
        D[d.oP + i] = v;
        D[d.oP + (size_t)d.npt * 3 + i] = v;
    }
}

/* Point record of one trial (12 doubles): the damped point block A = Hll + lambda I enters the Schur complement and
 * the back-substitution only through A^-1 = U U^T, U = C^-T upper triangular from the Cholesky factor A = C C^T:
 *   S' = sum_l (Hpl U)(Hpl U)^T,   reduced rhs = sum_l (Hpl U)(U^T bl),   xl = U (U^T r)
 * so the Schur kernel densifies ONE matrix Z = Hpl U instead of Hpl and Hpl A^-1. Layout: u00 u01 u02 u11 u12 u22,
 * bl (3; the Schur kernels form U^T bl from it, the back-substitution reads it), the point X at the linearisation state (3). A block that is not positive definite gives zeros and
 * flags the trial (st->sing), like the failed inverse of the CPU solver. */
__device__ __forceinline__ void ba_write_rec(double* q, const double* Hll, const double* bl, const double* X, double lambda,
                                             BaState* st) {
    const double a00 = Hll[0] + lambda, a10 = Hll[1], a20 = Hll[2], a11 = Hll[3] + lambda, a21 = Hll[4], a22 = Hll[5] + lambda;
    bool ok = a00 > 0;
    const double i00 = 1.0 / sqrt(ok ? a00 : 1.0), c10 = a10 * i00, c20 = a20 * i00;
    const double d1 = a11 - c10 * c10;
    ok = ok && d1 > 0;
    const double i11 = 1.0 / sqrt(ok ? d1 : 1.0), c21 = (a21 - c20 * c10) * i11;
    const double d2 = a22 - c20 * c20 - c21 * c21;
    ok = ok && d2 > 0 && isfinite(d2);
    const double i22 = 1.0 / sqrt(ok ? d2 : 1.0);
    if (!ok) st->sing = 1; /* benign race: every writer stores 1 */
    const double u00 = i00, u11 = i11, u22 = i22, u01 = -c10 * i00 * i11, u12 = -c21 * i11 * i22,
                 u02 = -(c20 * i00 + c21 * u01) * i22;
    /* six 16-byte stores: a record starts at a multiple of 96 bytes behind oHq, and ba_dims' take() keeps every offset and the
     * window stride even, so with the 16-byte-aligned workspace the int4 tables already need every record is 16-byte aligned */
    ba_d2* q2 = reinterpret_cast<ba_d2*>(q);
    q2[0] = ba_d2{ok ? u00 : 0.0, ok ? u01 : 0.0};
    q2[1] = ba_d2{ok ? u02 : 0.0, ok ? u11 : 0.0};
    q2[2] = ba_d2{ok ? u12 : 0.0, ok ? u22 : 0.0};
    q2[3] = ba_d2{bl[0], bl[1]}; /* the gradient itself: the back-substitution needs it, the Schur kernels form U^T bl (ba_rec_utb) */
    q2[4] = ba_d2{bl[2], X[0]};
    q2[5] = ba_d2{X[1], X[2]};
}
/* a point record as six 16-byte loads (alignment: see ba_write_rec) */
__device__ __forceinline__ void ba_load_rec(const double* __restrict__ q, double* __restrict__ r) {
    const ba_d2* q2 = reinterpret_cast<const ba_d2*>(q);
#pragma unroll
    for (int i = 0; i < 6; i++) { const ba_d2 v = q2[i]; r[2 * i] = v.x; r[2 * i + 1] = v.y; }
}

/* The observation stream of renumbered windows: 16-byte entries {kf, u, v, inv_sigma2}, the point implicit, sliced by
 * wavefront of the point passes. The 64 consecutive ranks [64 B, 64 B + 63] -- one wavefront, p = 256 bx + tid -- own the
 * entries ptStart[64 B] .. ptStart[64 B + 64]; inside that range all lanes' slot 0 come first, then all slot 1, ..., a slot
 * holds only the lanes with more observations than that, in lane order, without padding (tbm::ba_stream_slot is the rule, ba_stream_slot_self its form for the calling lane,
 * tb_ba_obs_stream_positions its host form). Slot j of a point is its j-th observation in the caller's order, so a walk
 * visits a point's observations in the order of the array-of-structs copy and every per-point sum keeps its order -- but a
 * wave-level load reads one contiguous run of up to 1 KB where 64 lanes walking their own 20-byte structs (lane stride ~88
 * bytes) touched 45-64 cache lines. No LDS, no barrier: the point passes share their CUs with the extractor's workgroups.
 * f(entry) runs for this lane's slots 0 .. deg - 1; the next slot's load is in flight meanwhile. Every lane of the
 * wavefront must call (deg = 0 for the lanes past the last point). */
struct BaStreamPos { int base, deg; int4 first; }; /* where a lane's walk starts: ba_stream_begin */
template <class F>
__device__ __forceinline__ void ba_stream_walk(const int4* __restrict__ S, const BaStreamPos& sp, F f) {
    const int deg = sp.deg;
    int base = sp.base;
    unsigned long long m = __ballot(0 < deg);
    int4 rn = sp.first;
    for (int j = 0; m != 0; j++) { /* wave-uniform trip count: the block's largest degree */
        const int4 r = rn;
        const unsigned long long mn = __ballot(j + 1 < deg);
        const int idx = tbm::ba_stream_slot_self(mn, &base);
        if (j + 1 < deg) rn = S[idx];
        if (j < deg) f(r);
        m = mn;
    }
}
/* the same walk for a light f: N slots' loads in flight together, then their N calls (one memory latency per N slots where the
 * walk above has one per slot unless f covers it) */
template <int N, class F>
__device__ __forceinline__ void ba_stream_walk_batched(const int4* __restrict__ S, const BaStreamPos& sp, F f) {
    const int deg = sp.deg;
    int base = sp.base - __popcll(__ballot(0 < deg)); /* sp.base is slot 1's: back to slot 0 */
    for (int j0 = 0; __ballot(j0 < deg) != 0; j0 += N) {
        int4 r[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            const unsigned long long m = __ballot(j0 + i < deg);
            const int idx = tbm::ba_stream_slot_self(m, &base);
            r[i] = make_int4(0, 0, 0, 0);
            if (j0 + i < deg) r[i] = S[idx];
        }
#pragma unroll
        for (int i = 0; i < N; i++)
            if (j0 + i < deg) f(r[i]);
    }
}
/* Start of the walk of point p (any p >= 0; every lane of the wavefront calls): this lane's degree, its slot-0 entry -- the load
 * is issued here, so a pass calls this before it waits for its state and poses -- and the first entry of slot 1. The tables are
 * complete and in range for every window, also one that k_ba_setup rejects. */
__device__ __forceinline__ BaStreamPos ba_stream_begin(const BaDims& d, const int* __restrict__ I, int p) {
    BaStreamPos sp;
    sp.base = I[d.oPtStart + min(p & ~63, d.npt)];
    sp.deg = (p < d.npt) ? I[d.oPtStart + p + 1] - I[d.oPtStart + p] : 0;
    sp.first = make_int4(0, 0, 0, 0);
    const int idx = tbm::ba_stream_slot_self(__ballot(0 < sp.deg), &sp.base);
    if (0 < sp.deg) sp.first = reinterpret_cast<const int4*>(I + d.oFreeKP)[idx];
    return sp;
}

/* U^T bl of a point record (zero for a block that was not positive definite: U is zero then) */
__device__ __forceinline__ void ba_rec_utb(const double* q, double* t) {
    t[0] = q[0] * q[6];
    t[1] = q[1] * q[6] + q[3] * q[7];
    t[2] = q[2] * q[6] + q[4] * q[7] + q[5] * q[8];
}

/* ---- A: point pass (STREAM: the window's observations come from the stream, d.stream; a template parameter so that each
 * form keeps its own register count) */
template <bool STREAM>
__device__ __forceinline__ void ba_points_pass(const BaDims& d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw,
                                               BaState* __restrict__ states, const int* __restrict__ errflag, int bx, int w) {
    __shared__ double red[4];
    /* keyframe poses as R | t, 12 doubles each: DYNAMIC shared memory sized by the window (960 bytes at 10 keyframes, where a static
     * array for the largest window took 6 KB): the pass is bound by HBM latency and bandwidth, its wavefronts are meant to sit on
     * CUs beside the extractor's workgroups, which leave ~10 KB of LDS free */
    extern __shared__ __attribute__((aligned(16))) double sRt[];
    const int tid = threadIdx.x;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    const int p = bx * BA_T + tid;
    BaStreamPos sp;
    if (STREAM) sp = ba_stream_begin(d, I, p); /* in flight beside the flag, the state and the poses */
    if (errflag[w]) { /* k_ba_setup rejected the window's observations: nothing may index with them */
        if (bx == 0 && tid == 0) { states[w].status = 1; states[w].err = 1; }
        return;
    }
    const BaState st = states[w];
    if (st.status) return;
    /* lambda of this trial is final unless it is the first one (k_ba_reduce derives it from the keyframe pass; k_ba_hinv then
     * writes the point records from the stored blocks). After a rejected step (need_lin == 0: same state, new lambda) the pass
     * simply runs again -- the same blocks, records for the new lambda -- so the blocks themselves are only stored in the
     * first trial: 72 of the pass's 282 bytes per point on every later one (the record carries the gradient). */
    const bool lam_known = st.iter > 0 || !st.need_lin;
    const tb_ba_obs* obs = obsAll + (size_t)w * d.obs_pitch;
    const double* T = D + d.oT + (size_t)st.cur * d.nkf * 7;
    const double* P = D + d.oP + (size_t)st.cur * d.npt * 3;
    for (int k = tid; k < d.nkf; k += BA_T) ba_pose_to_Rt(T + k * 7, sRt + k * 12);
    __syncthreads();
    const double delta = (double)sqrtf(5.991f);
    const bool in = p < d.npt;
    double chi = 0, maxd = 0;
    double Hll[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0}, X[3] = {0, 0, 0};
    if (in) { X[0] = P[3 * p]; X[1] = P[3 * p + 1]; X[2] = P[3 * p + 2]; }
    auto edge = [&](int kf, float ou, float ov, float ow) {
        BaLin L;
        ba_linearize(sRt + kf * 12, X, ou, ov, ow, d.fx, d.fy, d.cx, d.cy, delta, L);
        const double ww = L.ww, e0 = L.e0, e1 = L.e1;
        const double* Jl = L.Jl;
        chi += ba_huber_rho0(L.c2, delta);
        for (int a = 0; a < 3; a++) bl[a] = fma(-ww, fma(Jl[a], e0, Jl[3 + a] * e1), bl[a]);
        Hll[0] = fma(ww, fma(Jl[0], Jl[0], Jl[3] * Jl[3]), Hll[0]);
        Hll[1] = fma(ww, fma(Jl[0], Jl[1], Jl[3] * Jl[4]), Hll[1]);
        Hll[2] = fma(ww, fma(Jl[0], Jl[2], Jl[3] * Jl[5]), Hll[2]);
        Hll[3] = fma(ww, fma(Jl[1], Jl[1], Jl[4] * Jl[4]), Hll[3]);
        Hll[4] = fma(ww, fma(Jl[1], Jl[2], Jl[4] * Jl[5]), Hll[4]);
        Hll[5] = fma(ww, fma(Jl[2], Jl[2], Jl[5] * Jl[5]), Hll[5]);
    };
    if (STREAM) {
        ba_stream_walk(reinterpret_cast<const int4*>(I + d.oFreeKP), sp,
                       [&](const int4& r) { edge(r.x, __int_as_float(r.y), __int_as_float(r.z), __int_as_float(r.w)); });
    } else if (in) {
        const int eBeg = I[d.oPtStart + p], eEnd = I[d.oPtStart + p + 1];
        tb_ba_obs on = obs[min(eBeg, d.obs_pitch - 1)]; /* the next observation is in flight while this one is linearised */
        for (int e = eBeg; e < eEnd; e++) {
            const tb_ba_obs o = on;
            on = obs[min(e + 1, d.obs_pitch - 1)];
            edge(o.kf, o.u, o.v, o.inv_sigma2);
        }
    }
    if (in) {
        if (!lam_known) {
            for (int a = 0; a < 6; a++) D[d.oHll + (size_t)p * 6 + a] = Hll[a];
            for (int a = 0; a < 3; a++) D[d.oBl + (size_t)p * 3 + a] = bl[a];
        } else /* lambda of this trial is final; records sit in pattern order (renumbered windows: the point order) */
            ba_write_rec(D + d.oHq + (size_t)(d.renum ? p : I[d.oPtRank + p]) * 12, Hll, bl, X, st.lambda, states + w);
        maxd = fmax(fabs(Hll[0]), fmax(fabs(Hll[3]), fabs(Hll[5])));
    }
    const double s = ba_block_sum1(chi, red);
    const double m = ba_block_max1(maxd, red);
    if (tid == 0) {
        D[d.oPartP + (size_t)bx * 4] = s;
        D[d.oPartP + (size_t)bx * 4 + 1] = m;
    }
}

/* ---- B: keyframe pass: Hpp (21 unique) + bp (6) per free keyframe, chunked tree reductions */
/* Sum of 27 per-thread doubles over the 256 threads of a workgroup, result in threads 0..26 (value = thread index).
 * A butterfly of wave shuffles costs 12 LDS permutes and 6 adds PER VALUE (64-bit values travel as two dwords): 324
 * permutes per wavefront, more than the keyframe pass spends on its edges. Here every lane stores its values once, BA_KFG at a
 * time ([value][lane], row stride 65 doubles: conflict-free both ways), four lanes per value add 16 partials each in lane
 * order, one lane adds the four quarter sums, and threads 0..26 add the four wavefronts' sums: ~110 LDS / add slots per
 * wavefront, every sum of fixed shape. sh: BA_KFR_LDS doubles. */
#ifndef BA_KFG
#define BA_KFG 4   /* values per transpose round: 9.6 KB of LDS per workgroup, seven rounds. The pass reduces once per workgroup
                      now, not once per 512 edges, and the workgroup fits beside the FAST kernel's resident blocks, which leave
                      ~10 KB of a CU free. 14 (32 KB, two rounds): 0.294 against 0.316 ms per 171-window call alone, but 212
                      against 199 us per launch inside the step and 14.20 against 14.09 ms per step */
#endif
#define BA_KFW_LDS (BA_KFG * 65 + 4 * BA_KFG)     /* doubles per wavefront: transpose tile + quarter sums */
#define BA_KFR_LDS (4 * BA_KFW_LDS + 4 * 27)
__device__ __forceinline__ double ba_block_sum27(const double (&v)[27], double* sh) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double* T = sh + wave * BA_KFW_LDS;           /* this wavefront's transpose tile */
    double* Qs = T + BA_KFG * 65;                 /* its 4 BA_KFG quarter sums */
    double* red = sh + 4 * BA_KFW_LDS;            /* [4][27] wavefront sums */
#pragma unroll
    for (int g = 0; g < (27 + BA_KFG - 1) / BA_KFG; g++) {
        const int nv = min(BA_KFG, 27 - BA_KFG * g);
#pragma unroll
        for (int i = 0; i < BA_KFG; i++)
            if (i < nv) T[i * 65 + lane] = v[BA_KFG * g + i];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int q = lane / BA_KFG, i = lane - BA_KFG * q;    /* lanes 0..4 BA_KFG - 1: quarter q of value i */
        if (lane < 4 * BA_KFG && i < nv) {
            const double* src = T + i * 65 + 16 * q;
            double s = src[0];
#pragma unroll
            for (int k = 1; k < 16; k++) s += src[k];
            Qs[lane] = s;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < nv) red[wave * 27 + BA_KFG * g + lane] = (Qs[lane] + Qs[BA_KFG + lane]) + (Qs[2 * BA_KFG + lane] + Qs[3 * BA_KFG + lane]);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    __syncthreads();
    double r = 0;
    if (tid < 27) r = (red[tid] + red[27 + tid]) + (red[54 + tid] + red[81 + tid]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ void ba_kf_pass(const BaDims& d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw,
                                           const BaState* __restrict__ states, const int* __restrict__ errflag, int bid) {
    __shared__ double red[BA_KFR_LDS + 12];
    /* 1-D grid, a window per XCD at a time: workgroup ids go round-robin over the eight XCDs, so ids r, r + 8, r + 16, ... of a
     * run of 8 x (workgroups per window) ids serve ONE window -- all keyframes of a window gather from the same point array
     * (each touches most of its cache lines), which then comes from HBM once, into one L2, instead of once per keyframe */
    const int tid = threadIdx.x, nx = min(BA_KFBLK, d.kfChunks), per = nx * d.nfree;
    const int run = bid / (8 * per), rr_ = bid - run * (8 * per);
    const int w = run * 8 + (rr_ & 7), slot = rr_ >> 3;
    if (w >= d.W) return;
    if (errflag[w]) return; /* rejected input: the point pass flags the window, but runs BESIDE this pass now */
    const int share = slot % nx, kfree = slot / nx, kf = d.nfixed + kfree;
    const BaState st = states[w];
    if (st.status || !st.need_lin) return;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    const int beg = I[d.oKfStart + kf], end = I[d.oKfStart + kf + 1];
    /* The workgroup's share: a contiguous run [c0, c1) of the keyframe's occupied chunks, a function of the keyframe's edge
     * count alone (so a window sums the same way alone and in any batch). Its threads carry their 27 sums in registers over
     * the whole run -- thread t takes edges t, t + 256, t + 512, ... of the run in list order -- and the workgroup reduces ONCE:
     * with a reduction per 512-edge chunk (one chunk per workgroup at the bench's ~2100 edges per keyframe) close to half of a
     * wavefront's instructions were the pose conversion, the tree and its barriers, not edges. k_ba_reduce's contract stays:
     * it adds a keyframe's occupied chunk slots in index order; the run's total goes to its first slot, exact zeros to the rest. */
    const int nch = (end - beg + BA_KFCH - 1) / BA_KFCH, cps = (nch + nx - 1) / nx;
    const int c0 = share * cps, c1 = min(c0 + cps, nch);
    if (c0 >= c1) return;
    const int eb = beg + c0 * BA_KFCH, ee = min(beg + c1 * BA_KFCH, end); /* the share's edges */
    /* the keyframe's R|t: the first wavefront converts the quaternion, the others read the 12 doubles -- and every wavefront
     * holds them in scalar registers (they are uniform), which is what leaves room for the double buffer below */
    double Tk[12];
#if BA_KF_POSE_ONCE
    double* sRt = red + BA_KFR_LDS;
    if (tid < 64) {
        ba_pose_to_Rt(D + d.oT + ((size_t)st.cur * d.nkf + kf) * 7, Tk);
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 12; i++) sRt[i] = Tk[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 12; i++) Tk[i] = ba_uniform(sRt[i]);
#else
    ba_pose_to_Rt(D + d.oT + ((size_t)st.cur * d.nkf + kf) * 7, Tk);
#pragma unroll
    for (int i = 0; i < 12; i++) Tk[i] = ba_uniform(Tk[i]);
#endif
    const double* P = D + d.oP + (size_t)st.cur * d.npt * 3;
    const double delta = (double)sqrtf(5.991f);
    const int4* KR = reinterpret_cast<const int4*>(I + d.oKfRec);
    const int nr = (ee - eb + BA_KFE * BA_T - 1) / (BA_KFE * BA_T);
    /* the keyframe-ordered 16-byte records of a round's edges (written by the setup kernel: coalesced, no edge-id ->
     * observation gather). Lanes past the share -- the tail round's, and the look-ahead past the last round -- read the
     * share's last record, one cache line for all of them, and are marked: no branch in the loop, nothing out of bounds */
    auto load_rec = [&](int r, int4 (&rec)[BA_KFE]) {
#pragma unroll
        for (int j = 0; j < BA_KFE; j++) {
            const int idx = eb + (r * BA_KFE + j) * BA_T + tid;
            rec[j] = KR[min(idx, ee - 1)];
            if (idx >= ee) rec[j].x = -1;
        }
    };
    auto gather = [&](const int4 (&rec)[BA_KFE], double (&X)[BA_KFE][3]) {
#pragma unroll
        for (int j = 0; j < BA_KFE; j++) {
            const int p = min(max(rec[j].x, 0), d.npt - 1);
            X[j][0] = P[3 * p]; X[j][1] = P[3 * p + 1]; X[j][2] = P[3 * p + 2];
        }
    };
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0;
    auto edges = [&](const int4 (&rec)[BA_KFE], const double (&XX)[BA_KFE][3]) {
#pragma unroll
        for (int j = 0; j < BA_KFE; j++) {
            if (rec[j].x < 0) continue;
            const float ou = __int_as_float(rec[j].y), ov = __int_as_float(rec[j].z), ow = __int_as_float(rec[j].w);
            const double* X = XX[j];
            double Jp[12];
            BaLin L; /* residual and Huber weight exactly as the point pass computes them (same helper): cheaper than a
                        24-byte-per-edge round trip through HBM */
            ba_residual(Tk, X, ou, ov, ow, d.fx, d.fy, d.cx, d.cy, delta, L);
            ba_jac_pose_iz(L.pc, L.invz, d.fx, d.fy, Jp);
            const double ww = L.ww, e0 = L.e0, e1 = L.e1;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double wa = ww * Jp[a], wb = ww * Jp[6 + a];
                acc[21 + a] -= fma(wa, e0, wb * e1);
#pragma unroll
                for (int c = a; c < 6; c++) {
                    const int at = a * 6 - (a * (a - 1)) / 2 + (c - a);
                    acc[at] += fma(wa, Jp[c], wb * Jp[6 + c]);
                }
            }
        }
    };
#if BA_KF_AHEAD
    /* Register double buffer over the chain record -> point -> arithmetic: while round r's arithmetic runs, round r + 1's
     * points (their records arrived during round r - 1) and round r + 2's records are in flight. A load-use-load chain per
     * round was one memory latency per load step, paid by every workgroup; the pass is bound by exactly these latencies,
     * most of all inside the pipeline where the extractor's kernels load the memory system. */
    int4 ra[BA_KFE], rb[BA_KFE];
    double Xa[BA_KFE][3];
    load_rec(0, ra);
    load_rec(1, rb);
    gather(ra, Xa);
    for (int r = 0; r < nr; r++) {
        int4 rc[BA_KFE];
        double Xb[BA_KFE][3];
        gather(rb, Xb);
        load_rec(r + 2, rc);
        edges(ra, Xa);
#pragma unroll
        for (int j = 0; j < BA_KFE; j++) {
            ra[j] = rb[j]; rb[j] = rc[j];
            Xa[j][0] = Xb[j][0]; Xa[j][1] = Xb[j][1]; Xa[j][2] = Xb[j][2];
        }
    }
#else
    for (int r = 0; r < nr; r++) {
        int4 ra[BA_KFE];
        double Xa[BA_KFE][3];
        load_rec(r, ra);
        gather(ra, Xa);
        edges(ra, Xa);
    }
#endif
    const double tot = ba_block_sum27(acc, red);
    if (tid < 27) {
        double* out = D + d.oPartKF + ((size_t)kfree * d.kfChunks + c0) * 27 + tid;
        out[0] = tot;
        for (int ch = 1; ch < c1 - c0; ch++) out[ch * 27] = 0.0;
    }
}

/* ---- C: ordered reduction of the partials, lambda_0 */
template <bool STREAM>
__global__ void __launch_bounds__(BA_T)
k_ba_points(BaDims d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states,
            const int* __restrict__ errflag) {
    ba_points_pass<STREAM>(d, obsAll, dw, iw, states, errflag, (int)blockIdx.x, (int)blockIdx.y);
}
/* four wavefronts per SIMD asked for: the double-buffered pass compiles to 130 registers without the bound, 128 (no spill) with it */
__global__ void __launch_bounds__(BA_T, 4)
k_ba_kf(BaDims d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw, const BaState* __restrict__ states,
        const int* __restrict__ errflag) {
    ba_kf_pass(d, obsAll, dw, iw, states, errflag, (int)blockIdx.x);
}
/* ---- A + B in one launch, for small batches (the replayed graph): the point pass and the keyframe pass are independent of each
 * other (both read the state, each writes its own partials), so a batch that fills a fraction of the GPU runs them side by
 * side and saves a launch per trial (the 8-frame BA call 1.02 -> 0.97 ms). The keyframe pass's workgroups come first (ids
 * 0 ..: their window-per-XCD order needs id mod 8), then the point pass's. Large batches keep two launches: measured inside the
 * pipeline, the fused launch cost 17.6 against 16.6-17.0 ms per 512-frame step when the keyframe pass carried 32 KB of LDS into
 * every workgroup, and still 14.5-15.2 against 14.0-14.1 now that it carries 9.6 KB (BA_LIN_FUSE_ALL) -- the point pass's
 * workgroups then also take the keyframe pass's 128 registers. */
template <bool STREAM>
__global__ void __launch_bounds__(BA_T, 4)
k_ba_lin(BaDims d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states,
         const int* __restrict__ errflag, int nKfBlocks) {
    if ((int)blockIdx.x < nKfBlocks) ba_kf_pass(d, obsAll, dw, iw, states, errflag, (int)blockIdx.x);
    else {
        const int b = (int)blockIdx.x - nKfBlocks;
        ba_points_pass<STREAM>(d, obsAll, dw, iw, states, errflag, b % d.nblkP, b / d.nblkP);
    }
}

/* per-keyframe Hpp / bp from the chunk partials in order, chi2 of the linearisation state and the first lambda: a launch of its
 * own in the first trial (k_ba_hinv needs that lambda before the Schur kernel runs) and for large windows, the prologue of
 * k_ba_solve -- one workgroup per window as well -- in every later trial (a launch less per trial: 5 us, the critical path of a
 * small batch) */
__device__ __forceinline__ void ba_reduce_body(const BaDims& d, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states,
                                               int w, double* red) {
    const int tid = threadIdx.x;
    BaState* st = states + w;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    double maxd = 0;
    for (int i = tid; i < d.nfree * 27; i += BA_T) {
        const int kf = i / 27, c = i - kf * 27;
        const int nedges = I[d.oKfStart + d.nfixed + kf + 1] - I[d.oKfStart + d.nfixed + kf];
        const int nch = (nedges + BA_KFCH - 1) / BA_KFCH;
        double s = 0;
        for (int ch = 0; ch < nch; ch++) s += D[d.oPartKF + ((size_t)kf * d.kfChunks + ch) * 27 + c];
        if (c >= 21) D[d.oBp + kf * 6 + (c - 21)] = s;
        else {
            /* c -> (a, b) of the upper triangle, row-major */
            int a = 0, rem = c;
            while (rem >= 6 - a) { rem -= 6 - a; a++; }
            const int b = a + rem;
            D[d.oHpp + (size_t)kf * 36 + a * 6 + b] = s;
            D[d.oHpp + (size_t)kf * 36 + b * 6 + a] = s;
            if (a == b) maxd = fmax(maxd, fabs(s));
        }
    }
    const double mH = ba_block_max1(maxd, red);
    if (tid == 0) {
        double chi = 0, mL = 0;
        for (int b = 0; b < d.nblkP; b++) { chi += D[d.oPartP + (size_t)b * 4]; mL = fmax(mL, D[d.oPartP + (size_t)b * 4 + 1]); }
        st->currentChi = chi;
        if (st->iter == 0) { st->chi0 = chi; st->lambda = 1e-5 * fmax(mH, mL); st->ni = 2; }
        st->hq_fresh = st->iter > 0 ? 1 : 0; /* the point pass ran with this trial's final lambda */
        st->need_lin = 0;
    }
}

__global__ void __launch_bounds__(BA_T)
k_ba_reduce(BaDims d, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states) {
    __shared__ double red[4];
    const int w = blockIdx.x;
    if (states[w].status || !states[w].need_lin) return;
    ba_reduce_body(d, dw, iw, states, w, red);
}

/* ---- C2: damped point-block inverses for this trial's lambda, one thread per point: the 6 unique entries of
 * (Hll + lambda I)^-1 (ba_inv3's result is symmetric bit for bit) followed by bl, or zeros for a singular block.
 * The Schur wavefronts fetch these 9-double records with their edge rows instead of inverting on 4 lanes. */
__global__ void __launch_bounds__(BA_T)
k_ba_hinv(BaDims d, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states) {
    const int w = blockIdx.y, p = blockIdx.x * BA_T + threadIdx.x;
    const BaState st = states[w];
    if (st.status || st.hq_fresh || p >= d.npt) return; /* hq_fresh: k_ba_points wrote the records for this lambda */
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    double ph[6], pb[3], X[3];
#pragma unroll
    for (int i = 0; i < 6; i++) ph[i] = D[d.oHll + (size_t)p * 6 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) { pb[i] = D[d.oBl + (size_t)p * 3 + i]; X[i] = D[d.oP + ((size_t)st.cur * d.npt + p) * 3 + i]; }
    ba_write_rec(D + d.oHq + (size_t)(d.renum ? p : I[d.oPtRank + p]) * 12, ph, pb, X, st.lambda, states + w);
}

/* ---- D: Schur complement S' (np x np, lower triangle) and reduced rhs, pattern-compact MFMA form (round 3).
 * Nothing per edge is stored between the passes: S' = sum_l Z_l Z_l^T with Z_l = Hpl_l U_l (6 nfree x 3), where U_l
 * comes from the point record (A_l^-1 = U_l U_l^T) and every Hpl block = ww Jp^T Jl is rebuilt from the 16-byte
 * free-edge record and the linearisation state.
 *
 * Rounds 1-2 densified Z into a (6 nfree)-row tile and ran v_mfma_f64_16x16x4 over all of it: a point is seen by ~3.4 of
 * the 8 free keyframes, so 2.97 x the algorithmic flops were products with zero rows. Here the points of a window are
 * SORTED BY VISIBILITY PATTERN once per call (k_ba_groups: the mask of free keyframes that see the point), a group is a
 * run of up to BA_PCAP points / BA_EMAX edges with ONE pattern of k keyframes, and its tile holds only the 6 k rows that
 * exist (+ one row for the rhs): Zc[6 slot + a][3 pl + c], slot = rank of the keyframe inside the pattern. The block
 * product Zc Zc^T runs on v_mfma_f64_4x4x4 (four independent 4x4x4 products per instruction, 16 clocks: the same
 * 32 flop / clock / SIMD as the 16x16x4 form, measured in tools/ubench/mfma_f64_4x4.hip) at 4-row granularity:
 *   operand V_m      = rows 16 m .. 16 m + 15 of the tile (lane 16 kq + r: row r, column 4 ks + kq -- the 16x16x4 A layout
 *                      IS the 4x4x4 layout of four consecutive row blocks), one ds_read_b64;
 *   rot_s(V_m)       = its four row blocks rotated by s (DPP row_ror, two 32-bit moves): mfma(rot_s(V_m), V_m') is the
 *                      block diagonal s of tile (m, m'); s = 0, 1, 2 cover a diagonal tile's ten unique blocks, s = 0..3
 *                      the sixteen of an off-diagonal one;
 *   W_r              = one row block broadcast to all four positions (LDS read with a repeated address), for the
 *                      nb mod 4 row blocks behind the last full tile: one instruction per full tile instead of four.
 * Instructions per 4 columns: 3 (k = 2), 5 (k = 3), 9 (k = 4), 10 (k = 5), ... 25 (k = 8) against 6 x 4 = 24 block-equivalents
 * of the dense 48-row form whatever k is. The rhs sum_l Z_l (U_l^T bl_l) is row 6 k of the same product (its own row of the
 * tile holds U^T bl per column). A group's result is a compact (6 k + 1) x 6 k triangle: it goes through LDS once
 * (4x4 blocks, aliasing the tile) and is added into the wavefront's DENSE accumulators, which live in registers for the
 * whole kernel -- one register per 6 x 6 block pair (a >= b), lanes 0..35 its entries -- by a wave-uniform walk over the
 * pairs the pattern has. Every sum has a fixed order (groups in index order per wavefront, wavefronts in order, workgroups
 * in order in k_ba_solve), so the result is reproducible bit for bit.
 * Records are prefetched two groups ahead into one of two register sets, as before. */
#define BA_MAXT 4 /* 16-row tiles per side of the dense system (np <= 60) */
#define BA_REC 12
#define BA_RECS_LDS 256 /* staged point records of a group: BA_PCAP * BA_REC <= 256 doubles */
#define BA_KMFMA 5      /* patterns of up to this many keyframes run on the MFMA path */
#define BA_ZERO_LDS 40  /* a block of zeros behind them: what the block pairs a pattern does not have read */
/* The Schur tile is private to one wavefront and the LDS executes a wavefront's instructions in issue order, so
 * cross-lane visibility needs no counter wait: a wavefront-scope fence only pins the compiler's ordering (a
 * workgroup-scope one would also drain vmcnt, i.e. the prefetched records, on every phase change). */
__device__ __forceinline__ void ba_wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

/* geometry of a pattern with k keyframes: points per group, 4-row blocks (6 k rows + the rhs row), tile row stride.
 * The stride is 2 mod 4: the operand reads (16 rows x 2 columns per half wavefront) then hit 32 different 8-byte banks. */
__host__ __device__ constexpr int ba_c_cap(int k) { return (BA_EMAX / k) < BA_PCAP ? (BA_EMAX / k) : BA_PCAP; }
__host__ __device__ constexpr int ba_c_nb(int k) { return (6 * k + 1 + 3) / 4; }
__host__ __device__ constexpr int ba_c_ld(int k) { return ((3 * ba_c_cap(k) + 3) / 4) * 4 + 2; }
__host__ __device__ constexpr int ba_c_tile(int k) { return 4 * ba_c_nb(k) * ba_c_ld(k); }
#define BA_CB 37 /* doubles per 6 x 6 block of a group's compact result: 36 + 1, so that lanes reading different blocks at one offset spread over the banks */
__host__ __device__ constexpr int ba_c_rhs(int k) { return BA_CB * (k * (k + 1) / 2); }   /* the compact rhs starts behind the blocks */
__host__ __device__ constexpr int ba_c_tri(int k) { return ba_c_rhs(k) + 6 * k; }         /* compact result of a group */
__host__ __device__ constexpr int ba_c_nacc(int k) { /* block-product instructions per k-step (= accumulators) of pattern size k */
    const int nb = ba_c_nb(k), nvf = nb / 4, rem = nb % 4;
    return 3 * nvf + 2 * nvf * (nvf - 1) + rem * (nvf + 1);
}
struct BaCTab { int cap[BA_SMALL_MAXF + 1], ld[BA_SMALL_MAXF + 1], nacc[BA_SMALL_MAXF + 1]; };
__host__ __device__ constexpr BaCTab ba_c_tab() {
    BaCTab t = {};
    for (int k = 1; k <= BA_SMALL_MAXF; k++) { t.cap[k] = ba_c_cap(k); t.ld[k] = ba_c_ld(k); t.nacc[k] = ba_c_nacc(k); }
    return t;
}
__device__ const BaCTab ba_ctab = ba_c_tab();
static int ba_c_wave_lds(int nfree) {
    int m = 0;
    for (int k = 1; k <= nfree; k++) m = std::max(m, std::max(ba_c_tile(k), k <= BA_KMFMA ? ba_c_tri(k) : 0));
    return ((m + 3) & ~3) + BA_RECS_LDS + BA_ZERO_LDS;
}

/* Stable partition of src[0..n) by a predicate into dst (zeros first, both classes in source order) by one 256-thread
 * workgroup: every wavefront owns a contiguous quarter, counts, one barrier gives the bases, ballots rank. One pass of the
 * LSD pattern sort. tmp: >= 4 ints of LDS. Ends with a barrier (dst visible to the workgroup). */
template <class IsZero>
__device__ __forceinline__ void ba_stable_split(int n, int* tmp, const int* src, int* dst, IsZero isZero) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = (((n + 3) >> 2) + 63) & ~63, lo = min(wave * q, n), hi = min(lo + q, n);
    int cnt = 0;
    for (int e = lo + lane; e < hi; e += 64) cnt += isZero(src[e]) ? 1 : 0;
    cnt = tb_wave_sum(cnt);
    if (lane == 0) tmp[wave] = cnt;
    __syncthreads();
    int z = 0;
    for (int v = 0; v < wave; v++) z += tmp[v];
    int o = (tmp[0] + tmp[1] + tmp[2] + tmp[3]) + (lo - z); /* ones start behind all zeros; lo - z of them come before this quarter */
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int e0 = lo; e0 < hi; e0 += 64) {
        const int e = e0 + lane;
        const bool valid = e < hi;
        const int v = valid ? src[e] : 0;
        const bool f = valid && isZero(v);
        const unsigned long long m0 = __ballot(f), m1 = __ballot(valid && !f);
        if (valid) dst[f ? z + __popcll(m0 & lt) : o + __popcll(m1 & lt)] = v;
        z += __popcll(m0);
        o += __popcll(m1);
    }
    __threadfence_block();
    __syncthreads();
}

/* ---- once per call, before k_ba_setup (windows on the MFMA path with up to BA_SORT_LDS points and BA_PREP_MAXKF keyframes):
 * renumber the points in visibility-pattern order and build every index table of the call, one workgroup per window with its
 * tables in LDS.
 * The Schur kernel wants the points of one pattern adjacent; with the records alone stored in that order (first version of
 * round 3) the point-parallel passes wrote and read 96-byte records at scattered ranks, 10-15 % of their time. Here the
 * window's observations are copied once with pt := rank -- points of ascending mask, ties in the caller's order, each point's
 * edges in the caller's order -- and every later kernel runs on that copy: all per-point arrays are in pattern order, all
 * passes stream. k_ba_finish writes the points back through perm. Sums over a point's edges keep their order; sums over
 * points (chi2, keyframe blocks) run in the new order.
 * The tables: ptStart (CSR by point), the keyframe lists (kfStart, 16-byte records in ascending edge order: a stable counting
 * sort by keyframe, ballots per 64-edge slab), the free-keyframe edge records of the Schur kernel (a point's edges by
 * ascending keyframe = row block of its group's tile), the group descriptors, their cost prefix and the Schur wavefronts'
 * cuts. k_ba_setup built the lists with one workgroup per keyframe, each reading all observations twice (24 passes over the
 * window's observations, the largest HBM reader of the call), and k_ba_groups followed with the patterns; for the windows
 * that come here setup only checks the input and converts the state.
 * grid (W) x 1024 threads. Input that k_ba_setup's check rejects (indices out of range, not grouped by point) only has to stay
 * in range here: out-of-range observations are skipped and every write is bounded by the counts. */
#define BA_RT 1024          /* one workgroup per window walks all its observations a few times: latency, not bandwidth */
#define BA_PREP_MAXKF 64    /* keyframes of a window that takes this path (one lane per keyframe in the counting sort) */
__global__ void __launch_bounds__(BA_RT)
k_ba_prepare(BaDims d, const tb_ba_obs* __restrict__ obsAll, const int32_t* __restrict__ obsCounts, int* __restrict__ iw,
             tb_ba_obs* __restrict__ obs2All) {
    extern __shared__ __attribute__((aligned(16))) unsigned prep_lds[]; /* 16 bytes per point + 16 (host: 16 npt + 16) */
    unsigned* word = prep_lds;                                 /* edges of the (old) point << 16 | visibility mask */
    int* first = reinterpret_cast<int*>(prep_lds + d.npt);     /* first edge of every (old) point; later the free-edge prefix by rank */
    int* start2 = first + d.npt;                               /* [npt + 1] first edge of every rank in the copy; later the groups' cost prefix */
    unsigned short* pbuf = reinterpret_cast<unsigned short*>(start2 + d.npt + 1); /* two permutation buffers */
    constexpr int NW = BA_RT / 64;
    __shared__ int tmp[NW + 2];
    __shared__ int bins[1 << BA_SMALL_MAXF];   /* points per pattern, then first rank of every pattern */
    __shared__ int kfc[NW][BA_PREP_MAXKF];     /* edges of keyframe k in wavefront v's range, then their first list position */
    const int w = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const tb_ba_obs* obs = obsAll + (size_t)w * d.obs_pitch;
    tb_ba_obs* obs2 = obs2All + (size_t)w * d.obs_pitch;
    const int nobs = min(max(obsCounts[w], 0), d.obs_pitch);
    int* I = iw + (size_t)w * d.istride;
    for (int p = tid; p < d.npt; p += BA_RT) { word[p] = 0; first[p] = 0; }
    for (int i = tid; i < (1 << BA_SMALL_MAXF); i += BA_RT) bins[i] = 0;
    __syncthreads();
    for (int e0 = tid; e0 < nobs; e0 += 4 * BA_RT) { /* four independent observations (and their predecessors' points) in flight */
        tb_ba_obs o[4];
        int prev[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = min(e0 + i * BA_RT, nobs - 1);
            o[i] = obs[e];
            prev[i] = obs[max(e - 1, 0)].pt;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = e0 + i * BA_RT;
            if (e >= nobs || (unsigned)o[i].pt >= (unsigned)d.npt || (unsigned)o[i].kf >= (unsigned)d.nkf) continue;
            atomicAdd(&word[o[i].pt], 0x10000u);
            if (o[i].kf >= d.nfixed) atomicOr(&word[o[i].pt], 1u << (o[i].kf - d.nfixed));
            if (e == 0 || prev[i] != o[i].pt) first[o[i].pt] = e;
        }
    }
    /* LSD sort by mask, one stable ballot-ranked split per free keyframe (as k_ba_groups does for windows it sorts itself) */
    unsigned short* pa_ = pbuf;
    unsigned short* pb_ = pbuf + d.npt;
    for (int p = tid; p < d.npt; p += BA_RT) pa_[p] = (unsigned short)p;
    __syncthreads();
    {
        const int q = (((d.npt + NW - 1) / NW) + 63) & ~63, lo = min(wave * q, d.npt), hi = min(lo + q, d.npt);
        for (int b = 0; b < d.nfree; b++) {
            int cnt = 0;
            for (int e = lo + lane; e < hi; e += 64) cnt += ((word[pa_[e]] >> b) & 1) ? 0 : 1;
            cnt = tb_wave_sum(cnt);
            if (lane == 0) tmp[wave] = cnt;
            __syncthreads();
            int z = 0, all = 0;
            for (int v = 0; v < NW; v++) { const int c = tmp[v]; all += c; if (v < wave) z += c; }
            int o = all + (lo - z);
            for (int e0 = lo; e0 < hi; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < hi;
                const int v = valid ? pa_[e] : 0;
                const bool f = valid && !((word[v] >> b) & 1);
                const unsigned long long m0 = __ballot(f), m1 = __ballot(valid && !f);
                if (valid) pb_[f ? z + __popcll(m0 & lt) : o + __popcll(m1 & lt)] = (unsigned short)v;
                z += __popcll(m0);
                o += __popcll(m1);
            }
            __syncthreads();
            unsigned short* t = pa_; pa_ = pb_; pb_ = t;
        }
    }
    /* pa_[r] = the point that becomes r; its edges start behind those of the ranks before it */
    for (int r = tid; r < d.npt; r += BA_RT) {
        const int p = pa_[r];
        I[d.oPerm + r] = p;
        I[d.oPtRank + r] = r;             /* the point records are stored in point order */
        start2[r] = (int)(word[p] >> 16);
        pb_[p] = (unsigned short)r;       /* rank of the old point */
    }
    __syncthreads();
    const int total = tb_block_excl_scan(start2, d.npt, tmp);
    if (tid == 0) start2[d.npt] = total;
    __syncthreads();
    for (int r = tid; r <= d.npt; r += BA_RT) I[d.oPtStart + r] = start2[r];
    for (int e0 = tid; e0 < nobs; e0 += 4 * BA_RT) {
        tb_ba_obs o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = obs[min(e0 + i * BA_RT, nobs - 1)];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = e0 + i * BA_RT;
            if (e >= nobs || (unsigned)o[i].pt >= (unsigned)d.npt || (unsigned)o[i].kf >= (unsigned)d.nkf) continue;
            const int r = pb_[o[i].pt], j = e - first[o[i].pt];
            if ((unsigned)j >= (word[o[i].pt] >> 16)) continue; /* not grouped by point: rejected by k_ba_setup */
            o[i].pt = r;
            obs2[start2[r] + j] = o[i];
        }
    }
    __threadfence_block();
    __syncthreads(); /* the copy is complete and visible to the workgroup; first[] is free */
    if (d.stream) {
        /* the same observations once more as the point passes' stream (ba_stream_walk): a wavefront per 64-rank block walks the
         * block's slots exactly as the readers do and writes every slot's entries as one contiguous run. In a window that
         * k_ba_setup rejects the copy has slots nobody wrote; they are copied as they are, no pass reads them, and every
         * position lies inside the block's own range of ptStart. */
        int4* S = reinterpret_cast<int4*>(I + d.oFreeKP);
        for (int r0 = 64 * wave; r0 < d.npt; r0 += 64 * NW) {
            const int r = r0 + lane, eBeg = (r < d.npt) ? start2[r] : 0, deg = (r < d.npt) ? start2[r + 1] - eBeg : 0;
            int base = start2[r0];
            for (int j = 0;; j++) {
                const unsigned long long m = __ballot(j < deg);
                if (m == 0) break;
                const int idx = tbm::ba_stream_slot_self(m, &base);
                if (j < deg) {
                    const tb_ba_obs o = obs2[eBeg + j];
                    S[idx] = make_int4(o.kf, __float_as_int(o.u), __float_as_int(o.v), __float_as_int(o.inv_sigma2));
                }
            }
        }
    }
    /* masks by rank (the sort is done with the old order), free-edge prefix by rank, points per pattern */
    for (int r = tid; r < d.npt; r += BA_RT) {
        const unsigned m = word[pa_[r]] & 0xffffu;
        first[r] = __popc(m);
        if (m) atomicAdd(&bins[m], 1);
    }
    __syncthreads();
    for (int r = tid; r < d.npt; r += BA_RT) pb_[r] = (unsigned short)(word[pa_[r]] & 0xffffu); /* pb_: mask of rank r from here on */
    const int nfreeE = tb_block_excl_scan(first, d.npt, tmp); /* first[r]: the point's first record in the Schur kernel's list */
    (void)nfreeE;
    unsigned short* mk = pb_;
    /* ---- keyframe lists: stable counting sort of the copy's edges by keyframe. Every wavefront owns a contiguous range. */
    {
        const int q = (((total + NW - 1) / NW) + 63) & ~63, lo = min(wave * q, total), hi = min(lo + q, total);
        int cnt = 0; /* lane k: edges of keyframe k in this range */
        for (int e0 = lo; e0 < hi; e0 += 256) { /* four slabs' loads in flight (one at a time: a cache round trip per slab) */
            int kf4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int e = e0 + 64 * u + lane; kf4[u] = (e < hi) ? obs2[e].kf : -1; }
#pragma unroll
            for (int u = 0; u < 4; u++)
                for (int k = 0; k < d.nkf; k++) {
                    const unsigned long long m = __ballot(kf4[u] == k);
                    if (lane == k) cnt += __popcll(m);
                }
        }
        if (lane < d.nkf) kfc[wave][lane] = cnt;
        __syncthreads();
        if (tid < d.nkf) { /* thread k: keyframe k's list start, and every wavefront's first position in it */
            int base = 0;
            for (int k = 0; k < tid; k++)
                for (int v = 0; v < NW; v++) base += kfc[v][k];
            I[d.oKfStart + tid] = base;
            int run = base;
            for (int v = 0; v < NW; v++) run += kfc[v][tid];
            if (tid == d.nkf - 1) I[d.oKfStart + d.nkf] = run;
        }
        __syncthreads();
        if (tid < d.nkf) {
            int run = I[d.oKfStart + tid];
            for (int v = 0; v < NW; v++) { const int c = kfc[v][tid]; kfc[v][tid] = run; run += c; }
        }
        __syncthreads();
        int4* KR = reinterpret_cast<int4*>(I + d.oKfRec);
        for (int e00 = lo; e00 < hi; e00 += 256) {
            tb_ba_obs o4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e00 + 64 * u + lane;
                o4[u].kf = -1; o4[u].pt = 0; o4[u].u = o4[u].v = o4[u].inv_sigma2 = 0.f;
                if (e < hi) o4[u] = obs2[e];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) { /* slab by slab: the list positions follow the edge order */
                const int e = e00 + 64 * u + lane;
                const tb_ba_obs o = o4[u];
                unsigned long long mine = 0;
                int add = 0;
                for (int k = 0; k < d.nkf; k++) {
                    const unsigned long long m = __ballot(o.kf == k);
                    if (o.kf == k) mine = m;
                    if (lane == k) add = __popcll(m);
                }
                if (o.kf >= 0 && o.kf < d.nkf) {
                    const int pos = kfc[wave][o.kf] + __popcll(mine & lt);
                    I[d.oKfEdges + pos] = e;
                    KR[pos] = make_int4(o.pt, __float_as_int(o.u), __float_as_int(o.v), __float_as_int(o.inv_sigma2));
                }
                ba_wave_lds_fence();
                if (lane < d.nkf) kfc[wave][lane] += add;
                ba_wave_lds_fence();
            }
        }
    }
    /* ---- the Schur kernel's edge records: a point's free-keyframe edges by ascending keyframe, points in rank order */
    int4* KPs = reinterpret_cast<int4*>(I + d.oKPs);
    for (int r = tid; r < d.npt; r += BA_RT) {
        const int m = mk[r];
        if (m == 0) continue;
        const int base = first[r];
        for (int e = start2[r]; e < start2[r + 1]; e++) {
            const tb_ba_obs o = obs2[e];
            const int fk = o.kf - d.nfixed;
            if ((unsigned)fk >= (unsigned)d.nfree) continue; /* a fixed keyframe -- or, in a rejected window, a slot of the copy nobody wrote */
            KPs[base + __popc(m & ((1 << fk) - 1))] = make_int4((int)(((unsigned)r << 6) | (unsigned)fk), __float_as_int(o.u), __float_as_int(o.v),
                                                                 __float_as_int(o.inv_sigma2));
        }
    }
    /* ---- groups: every ba_c_cap(k)-th point of a pattern's run starts one */
    tb_block_excl_scan(bins, 1 << BA_SMALL_MAXF, tmp); /* bins[m]: first rank of pattern m (ranks ascend with the mask; mask 0 first) */
    int zero_pts = 0;
    {   /* points without a free-keyframe edge come first and are not in the bins */
        int c = 0;
        for (int r = tid; r < d.npt; r += BA_RT) c += (mk[r] == 0) ? 1 : 0;
        c = tb_wave_sum(c);
        __syncthreads();
        if (lane == 0) tmp[wave] = c;
        __syncthreads();
        for (int v = 0; v < NW; v++) zero_pts += tmp[v];
        __syncthreads();
    }
    auto pat_first = [&](int m) { return zero_pts + bins[m]; };
    auto pat_count = [&](int m) { return ((m + 1 < (1 << BA_SMALL_MAXF)) ? bins[m + 1] : d.npt - zero_pts) - bins[m]; };
    int* gflag = start2; /* start2 went to global memory above: from here the group index of every rank, then the cost prefix */
    __syncthreads();
    for (int r = tid; r < d.npt; r += BA_RT) {
        const int m = mk[r];
        gflag[r] = (m != 0 && (r - pat_first(m)) % ba_ctab.cap[__popc(m)] == 0) ? 1 : 0;
    }
    __syncthreads();
    const int ng = tb_block_excl_scan(gflag, d.npt, tmp);
    int4* GD = reinterpret_cast<int4*>(I + d.oGDesc);
    for (int r = tid; r < d.npt; r += BA_RT) {
        const int m = mk[r];
        if (m == 0) continue;
        const int k = __popc(m), at = r - pat_first(m);
        if (at % ba_ctab.cap[k] != 0) continue;
        GD[gflag[r]] = make_int4(r, first[r], m, min(ba_ctab.cap[k], pat_count(m) - at));
    }
    if (tid == 0) I[d.oGDesc + 4 * (size_t)d.npt] = ng;
    __threadfence_block();
    __syncthreads();
    /* cost estimate per group (shader clocks / 64 of the Schur kernel's phases, measured: a fixed part for the linearisation
     * and the bookkeeping, the k-steps times the pattern's products, the direct form per tile column), as an exclusive
     * prefix: the Schur wavefronts cut the group list into runs of equal cost */
    int* GC = gflag;
    for (int g = tid; g < ng; g += BA_RT) {
        const int4 gd = GD[g];
        const int k = __popc(gd.z), nks = (3 * gd.w + 3) >> 2;
        GC[g] = 55 + ((k <= BA_KMFMA) ? nks * ba_ctab.nacc[k] : 12 * gd.w);
    }
    __syncthreads();
    const int cost = tb_block_excl_scan(GC, ng, tmp);
    if (tid == 0) GC[ng] = cost;
    __syncthreads();
    const int nwv = ba_schur_waves(d, w);
    for (int v = tid; v <= nwv; v += BA_RT) {
        const long long target = ((long long)cost * v + nwv - 1) / nwv;
        int lo = 0, hi = ng;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (GC[mid] < target) lo = mid + 1; else hi = mid;
        }
        I[d.oGCut + v] = (v == 0) ? 0 : (v == nwv) ? ng : lo;
    }
}

/* ---- once per call, windows on the MFMA path: visibility patterns, pattern sort, ranks, pattern-ordered edge records,
 * group descriptors. grid (W) x 256 threads. */
__global__ void __launch_bounds__(BA_T)
k_ba_groups(BaDims d, int* __restrict__ iw, const int* __restrict__ errflag) {
    __shared__ int cntb[1 << BA_SMALL_MAXF], bst[1 << BA_SMALL_MAXF], ebin[1 << BA_SMALL_MAXF], tmp[16];
    __shared__ unsigned short sortbuf[3 * BA_SORT_LDS];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (errflag[w]) return; /* observations rejected by k_ba_setup: k_ba_points ends the window before anything reads the tables */
    int* I = iw + (size_t)w * d.istride;
    const int4* KP = reinterpret_cast<const int4*>(I + d.oFreeKP);
    const int nbins = 1 << d.nfree;
    for (int i = tid; i < nbins; i += BA_T) cntb[i] = 0;
    __syncthreads();
    for (int p = tid; p < d.npt; p += BA_T) {
        const int e0 = I[d.oPtFree + p], e1 = I[d.oPtFree + p + 1];
        int m = 0;
        for (int e = e0; e < e1; e++) m |= 1 << (KP[e].x & 63);
        I[d.oPtMask + p] = m;
        if (d.npt > BA_SORT_LDS) I[d.oPermA + p] = p;
        atomicAdd(&cntb[m], 1); /* counts only: the order of the adds does not matter */
    }
    __threadfence_block();
    __syncthreads();
    /* LSD sort of the points by mask, one stable split per free keyframe: equal masks end up adjacent, in point order.
     * Windows of up to BA_SORT_LDS points keep the masks and both permutation buffers in LDS (16-bit entries): a pass is
     * two sweeps of LDS reads instead of two chains of dependent global loads (the kernel is one workgroup per window, pure
     * latency: 190 -> ~40 us). Larger windows sort through the global buffers. */
    int* src = I + d.oPermA;
    int* dst = I + d.oPermB;
    if (d.npt <= BA_SORT_LDS) {
        unsigned short* mk = sortbuf;                  /* mask of point p */
        unsigned short* pa_ = sortbuf + BA_SORT_LDS;   /* permutation, ping */
        unsigned short* pb_ = sortbuf + 2 * BA_SORT_LDS;
        for (int p = tid; p < d.npt; p += BA_T) { mk[p] = (unsigned short)I[d.oPtMask + p]; pa_[p] = (unsigned short)p; }
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;
        const int q = (((d.npt + 3) >> 2) + 63) & ~63, lo = min(wave * q, d.npt), hi = min(lo + q, d.npt);
        const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        for (int b = 0; b < d.nfree; b++) {
            int cnt = 0;
            for (int e = lo + lane; e < hi; e += 64) cnt += ((mk[pa_[e]] >> b) & 1) ? 0 : 1;
            cnt = tb_wave_sum(cnt);
            if (lane == 0) tmp[wave] = cnt;
            __syncthreads();
            int z = 0;
            for (int v = 0; v < wave; v++) z += tmp[v];
            int o = (tmp[0] + tmp[1] + tmp[2] + tmp[3]) + (lo - z);
            for (int e0 = lo; e0 < hi; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < hi;
                const int v = valid ? pa_[e] : 0;
                const bool f = valid && !((mk[v] >> b) & 1);
                const unsigned long long m0 = __ballot(f), m1 = __ballot(valid && !f);
                if (valid) pb_[f ? z + __popcll(m0 & lt) : o + __popcll(m1 & lt)] = (unsigned short)v;
                z += __popcll(m0);
                o += __popcll(m1);
            }
            __syncthreads();
            unsigned short* t = pa_; pa_ = pb_; pb_ = t;
        }
        for (int r = tid; r < d.npt; r += BA_T) src[r] = pa_[r]; /* the later stages read the order from the global buffer */
        __threadfence_block();
        __syncthreads();
    } else {
        for (int b = 0; b < d.nfree; b++) {
            ba_stable_split(d.npt, tmp, src, dst, [&](int p) { return ((I[d.oPtMask + p] >> b) & 1) == 0; });
            int* t = src; src = dst; dst = t;
        }
    }
    for (int r = tid; r < d.npt; r += BA_T) I[d.oPtRank + src[r]] = r;
    /* first rank and first pattern-ordered edge of every pattern */
    for (int i = tid; i < nbins; i += BA_T) { bst[i] = cntb[i]; ebin[i] = cntb[i] * __popc(i); }
    __syncthreads();
    tb_block_excl_scan(bst, nbins, tmp);
    tb_block_excl_scan(ebin, nbins, tmp);
    __threadfence_block();
    __syncthreads();
    /* the free-keyframe edge records in pattern order; a point's edges in ascending keyframe order (slot = row block) */
    int4* KPs = reinterpret_cast<int4*>(I + d.oKPs);
    for (int p = tid; p < d.npt; p += BA_T) {
        const int m = I[d.oPtMask + p];
        if (m == 0) continue;
        const int k = __popc(m), base = ebin[m] + (I[d.oPtRank + p] - bst[m]) * k;
        const int e0 = I[d.oPtFree + p], e1 = I[d.oPtFree + p + 1];
        for (int e = e0; e < e1; e++) {
            const int4 rec = KP[e];
            KPs[base + __popc(m & ((1 << (rec.x & 63)) - 1))] = rec;
        }
    }
    /* groups: every ba_c_cap(k)-th point of a pattern's run starts one */
    int unused = 0;
    int4* GD = reinterpret_cast<int4*>(I + d.oGDesc);
    auto starts = [&](int r) {
        const int m = I[d.oPtMask + src[r]];
        return m != 0 && (r - bst[m]) % ba_ctab.cap[__popc(m)] == 0;
    };
    const int ng = ba_ordered_rank(d.npt, tmp, starts, [](int) { return false; }, &unused, [&](int r, int g, bool hit) {
        if (!hit) return;
        const int m = I[d.oPtMask + src[r]], k = __popc(m), at = r - bst[m];
        GD[g] = make_int4(r, ebin[m] + at * k, m, min(ba_ctab.cap[k], cntb[m] - at));
    });
    if (tid == 0) I[d.oGDesc + 4 * (size_t)d.npt] = ng;
    /* cost estimate per group (shader clocks / 64 of the Schur kernel's phases, measured: a fixed part for the linearisation
     * and the bookkeeping, the k-steps times the pattern's products, the direct form per tile column), as an exclusive
     * prefix: the Schur wavefronts cut the group list into runs of equal cost */
    __threadfence_block();
    __syncthreads();
    int* GC = I + d.oGCost;
    for (int g = tid; g < ng; g += BA_T) {
        const int4 gd = GD[g];
        const int k = __popc(gd.z), nks = (3 * gd.w + 3) >> 2;
        GC[g] = 55 + ((k <= BA_KMFMA) ? nks * ba_ctab.nacc[k] : 12 * gd.w);
    }
    if (tid == 0) GC[ng] = 0;
    __threadfence_block();
    __syncthreads();
    const int total = tb_block_excl_scan(GC, ng, tmp);
    if (tid == 0) GC[ng] = total;
    __threadfence_block();
    __syncthreads();
    /* where the window's Schur wavefronts start: wavefront v takes the groups whose cost prefix lies in
     * [v, v + 1) / nwv of the total (a binary search per wavefront at kernel start cost 18 dependent loads) */
    const int nwv = ba_schur_waves(d, w);
    for (int v = tid; v <= nwv; v += BA_T) {
        const long long target = ((long long)total * v + nwv - 1) / nwv;
        int lo = 0, hi = ng;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (GC[mid] < target) lo = mid + 1; else hi = mid;
        }
        I[d.oGCut + v] = (v == 0) ? 0 : (v == nwv) ? ng : lo;
    }
}

/* broadcast of one lane's double through the scalar unit (lane index wave-uniform) */
__device__ __forceinline__ double ba_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
/* rot_S: lane x of every row of 16 lanes reads lane x + 4 S of the same row (row_ror:16 - 4 S moves data 16 - 4 S lanes up) */
template <int S>
__device__ __forceinline__ double ba_rot(double v) {
    static_assert(S >= 1 && S <= 3, "rotation by whole row blocks");
    /* every lane has a source inside its row: the `old` operand is never used, passing the source avoids a zero fill */
    const int l0 = __double2loint(v), h0 = __double2hiint(v);
    const int lo = __builtin_amdgcn_update_dpp(l0, l0, 0x120 + 16 - 4 * S, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(h0, h0, 0x120 + 16 - 4 * S, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int S>
__device__ __forceinline__ double ba_rot_any(double v) {
    if constexpr (S == 0) return v;
    else return ba_rot<S>(v);
}

#ifdef BA_TIMING   /* debug build: shader clocks of the Schur kernel's phases (wavefront 0 of every 16th window's workgroups) */
__device__ unsigned long long ba_times[24];
extern "C" int tb_debug_ba_times(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ba_times), sizeof(unsigned long long) * 24) != hipSuccess) return -1;
    if (reset) { unsigned long long z[24] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(ba_times), z, sizeof z); }
    return 0;
}
#define BA_TK(i) do { const unsigned long long t1_ = __builtin_readcyclecounter(); tk_[i] += t1_ - t0_; t0_ = t1_; } while (0)
#else
#define BA_TK(i) do { } while (0)
#endif

/* one prefetched Schur group */
struct BaPreC {
    int key;           /* lane < edges of the group: pt << 6 | free keyframe index, else -1 */
    float u, v, w;     /* pixel, information scale */
    double r0, r1, r2, r3; /* doubles lane, 64 + lane, ... of the group's point records */
    int4 cur;          /* the group this set holds: first rank, first edge, pattern, points */
    int4 nxt;          /* the group it fetches next */
};

/* Block product of a group's tile for a pattern of K keyframes. Result into C in the layout the dense accumulators
 * read: 6 x 6 block (sa >= sb) of the pattern's keyframe slots at C[BA_CB (sa (sa + 1) / 2 + sb)], row major, diagonal
 * blocks with both halves; the rhs (row 6 K) at C[ba_c_rhs(K)].
 * C may alias the tile: it is written after the last operand read. Patterns of up to BA_KMFMA = 5 keyframes come here (at
 * most 10 accumulators); the accumulators of larger ones (25 at K = 8) would set the kernel's register allocation for
 * every path, so those take the direct form in the kernel.
 * Where an accumulator's 64 entries go depends only on (K, accumulator, lane): BaCGeom<K>::where() is that map, evaluated
 * once per workgroup into an LDS table (ba_c_build_table) -- computing it per group cost more than the products
 * (divisions by 6, triangular indices: ~35 instructions per accumulator against one table read and two stores). */
template <int K> struct BaCGeom {
    static constexpr int NB = ba_c_nb(K), LD = ba_c_ld(K), NVF = NB / 4, REM = NB % 4;
    static constexpr int LASTROW = 4 * NB - 1;
    static constexpr int NV = NVF + ((REM > 1) ? 1 : 0);  /* operands with four row blocks: the full tiles, then the partial one */
    static constexpr int NAF = 3 * NVF + 2 * NVF * (NVF - 1); /* accumulators of the full tile rows */
    static constexpr int NACC = NAF + REM * (NVF + 1);
    static_assert(NACC <= 12 && NACC > 0 && NACC == ba_c_nacc(K), "accumulators of a pattern on the MFMA path");
    __host__ __device__ static constexpr int aofs(int m) { return 3 * m + 2 * m * (m - 1); } /* first accumulator of tile row m */
    /* destination of accumulator t's entry in this lane: main | mirror << 16, in doubles from the start of the wavefront's
     * LDS; 0xffff for entries that are not part of the result */
    __host__ __device__ static constexpr unsigned where(int t, int lane) {
        constexpr int trash = 0xffff;
        /* result lane 16 i + 4 q + j = entry (i, j) of position q's block */
        const int i = lane >> 4, q = (lane >> 2) & 3, j = lane & 3;
        int row = 0, col = 0;
        bool ok = true;
        if (t < NAF) {
            int m = 0;
            while (m + 1 < NVF && aofs(m + 1) <= t) m++;
            const int u = t - aofs(m);                 /* 0..2: the diagonal tile's rotations; then four per tile left of it */
            const int mp = (u < 3) ? m : (u - 3) >> 2, sr = (u < 3) ? u : (u - 3) & 3;
            row = 16 * m + 4 * ((q + sr) & 3) + i;     /* rot_sr brings this block to position q */
            col = 16 * mp + 4 * q + j;
            if (u == 2) ok = q < 2;                    /* positions 2, 3 repeat 0, 1 transposed */
        } else {
            const int r = (t - NAF) / (NVF + 1), mp = (t - NAF) % (NVF + 1);
            row = 4 * (4 * NVF + r) + i;
            if (mp < NVF) col = 16 * mp + 4 * q + j;
            else { col = 4 * (4 * NVF + ((REM > 1) ? q : r)) + j; ok = (REM > 1) ? (q <= r) : (q == 0); }
        }
        /* a wrapped position holds the transposed upper block; the upper half of a diagonal 4 x 4 block repeats the lower */
        const int rr = row > col ? row : col, cc = row > col ? col : row;
        const int sa = rr / 6, sb = cc / 6, ii = rr - 6 * sa, jj = cc - 6 * sb;
        const int blk = BA_CB * (sa * (sa + 1) / 2 + sb);
        unsigned mainw = (unsigned)trash, mirr = (unsigned)trash;
        if (ok && rr < 6 * K) {
            mainw = (unsigned)(blk + 6 * ii + jj);
            if (sa == sb) mirr = (unsigned)(blk + 6 * jj + ii);
        }
        if (ok && rr == 6 * K) mainw = (unsigned)(ba_c_rhs(K) + cc);
        return mainw | (mirr << 16);
    }
};
__host__ __device__ constexpr int ba_c_tab_ofs(int k) { /* first table row of pattern size k */
    int o = 0;
    if (k > 1) o += BaCGeom<1>::NACC;
    if (k > 2) o += BaCGeom<2>::NACC;
    if (k > 3) o += BaCGeom<3>::NACC;
    if (k > 4) o += BaCGeom<4>::NACC;
    if (k > 5) o += BaCGeom<5>::NACC;
    return o;
}
#define BA_CTAB_ROWS (ba_c_tab_ofs(BA_KMFMA + 1))
struct BaCWhere { unsigned v[BA_CTAB_ROWS * 64]; };
template <int K>
__host__ __device__ constexpr void ba_c_where_rows(BaCWhere& t) {
    for (int a = 0; a < BaCGeom<K>::NACC; a++)
        for (int l = 0; l < 64; l++) t.v[(ba_c_tab_ofs(K) + a) * 64 + l] = BaCGeom<K>::where(a, l);
}
__host__ __device__ constexpr BaCWhere ba_c_where_table() {
    BaCWhere t = {};
    ba_c_where_rows<1>(t); ba_c_where_rows<2>(t); ba_c_where_rows<3>(t); ba_c_where_rows<4>(t); ba_c_where_rows<5>(t);
    return t;
}
__device__ const BaCWhere ba_cwhere = ba_c_where_table(); /* evaluated by the compiler; every workgroup copies it into LDS */

#define BA_CACC 12 /* accumulators of the MFMA path (the largest pattern on it needs 10) */
/* acc += block product of the tile (nks k-steps). The accumulators are the caller's: consecutive groups of one pattern
 * keep adding into them, the compact result is written once per run (ba_c_store). */
template <int K>
__device__ __forceinline__ void ba_c_mac(double (&acc)[BA_CACC], const double* __restrict__ Zt, int nks, int lane) {
    typedef BaCGeom<K> G;
    constexpr int NVF = G::NVF, REM = G::REM, NV = G::NV, NAF = G::NAF, LD = G::LD;
    /* the operand offsets below depend only on the lane: left alone, the compiler computes them for all five patterns ahead
     * of the group loop and keeps ~25 registers alive through the linearisation, the kernel's register peak */
    asm volatile("" : "+v"(lane));
    const int kq = lane >> 4, r16 = lane & 15;
    int vofs[NV + 1], wofs[REM + 1];
#pragma unroll
    for (int m = 0; m < NV; m++) vofs[m] = min(16 * m + r16, G::LASTROW) * LD + kq; /* the partial tile's rows are clamped (unused blocks) */
#pragma unroll
    for (int r = 0; r < REM; r++) wofs[r] = (4 * (4 * NVF + r) + (lane & 3)) * LD + kq;
    auto step = [&](const double (&V)[NV + 1], const double (&W)[REM + 1]) {
#pragma unroll
        for (int m = 0; m < NVF; m++) {
            const int o = G::aofs(m);
            const double r1 = ba_rot<1>(V[m]), r2 = ba_rot<2>(V[m]);
            acc[o] = __builtin_amdgcn_mfma_f64_4x4x4f64(V[m], V[m], acc[o], 0, 0, 0);
            acc[o + 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(r1, V[m], acc[o + 1], 0, 0, 0);
            acc[o + 2] = __builtin_amdgcn_mfma_f64_4x4x4f64(r2, V[m], acc[o + 2], 0, 0, 0);
            if (m > 0) {
                const double r3 = ba_rot<3>(V[m]);
#pragma unroll
                for (int mp = 0; mp < m; mp++) {
                    const int p = o + 3 + 4 * mp;
                    acc[p] = __builtin_amdgcn_mfma_f64_4x4x4f64(V[m], V[mp], acc[p], 0, 0, 0);
                    acc[p + 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(r1, V[mp], acc[p + 1], 0, 0, 0);
                    acc[p + 2] = __builtin_amdgcn_mfma_f64_4x4x4f64(r2, V[mp], acc[p + 2], 0, 0, 0);
                    acc[p + 3] = __builtin_amdgcn_mfma_f64_4x4x4f64(r3, V[mp], acc[p + 3], 0, 0, 0);
                }
            }
        }
        if (REM > 0) {
            const double VP = (REM > 1) ? V[NV - 1] : W[0]; /* one trailing block: every position of W[0] x W[0] is that block */
#pragma unroll
            for (int r = 0; r < REM; r++) {
                const int o = NAF + r * (NVF + 1);
#pragma unroll
                for (int mp = 0; mp < NVF; mp++) acc[o + mp] = __builtin_amdgcn_mfma_f64_4x4x4f64(W[r], V[mp], acc[o + mp], 0, 0, 0);
                acc[o + NVF] = __builtin_amdgcn_mfma_f64_4x4x4f64(W[r], VP, acc[o + NVF], 0, 0, 0);
            }
        }
    };
    auto fetch = [&](double (&V)[NV + 1], double (&W)[REM + 1], int ks) {
        const double* z = Zt + 4 * ks;
#pragma unroll
        for (int m = 0; m < NV; m++) V[m] = z[vofs[m]];
#pragma unroll
        for (int r = 0; r < REM; r++) W[r] = z[wofs[r]];
    };
    /* three operand sets in turn: the reads of k-steps ks + 1 and ks + 2 are in flight during the products of k-step ks --
     * with two wavefronts per SIMD and eight per CU on the LDS, one k-step of products (80-160 clocks) does not cover a
     * read. The reads behind the last k-step stay inside the wavefront's LDS and are never used. */
    double Va[NV + 1], Wa[REM + 1], Vb[NV + 1], Wb[REM + 1], Vc[NV + 1], Wc[REM + 1];
    fetch(Va, Wa, 0);
    fetch(Vb, Wb, 1);
    int ks = 0;
    for (; ks + 2 < nks; ks += 3) {
        fetch(Vc, Wc, ks + 2);
        step(Va, Wa);
        fetch(Va, Wa, ks + 3);
        step(Vb, Wb);
        fetch(Vb, Wb, ks + 4);
        step(Vc, Wc);
    }
    if (ks < nks) step(Va, Wa);
    if (ks + 1 < nks) step(Vb, Wb);
    ba_wave_lds_fence();
    asm volatile("; end of ba_c_mac<%0>" : : "n"(K)); /* see ba_c_store */
}
/* accumulators -> compact result, and clear them: destination pair of every entry from the table (0xffff: not part of the
 * result) */
template <int K>
__device__ __forceinline__ void ba_c_store(double (&acc)[BA_CACC], double* __restrict__ C, const unsigned* __restrict__ tab, int lane) {
    constexpr int NACC = BaCGeom<K>::NACC;
    unsigned wh[NACC];
#pragma unroll
    for (int t = 0; t < NACC; t++) wh[t] = tab[(ba_c_tab_ofs(K) + t) * 64 + lane];
#pragma unroll
    for (int t = 0; t < NACC; t++) {
        /* predicated: 60 lanes storing to ONE spare address would serialise in its bank */
        if ((wh[t] & 0xffffu) != 0xffffu) C[wh[t] & 0xffffu] = acc[t];
        if ((wh[t] >> 16) != 0xffffu) C[wh[t] >> 16] = acc[t];
        acc[t] = 0;
    }
    ba_wave_lds_fence();
    /* a different statement per pattern size: the compiler otherwise merges the tails of the callers' switch cases ("store
     * and clear the LAST accumulator" of every size) into one block behind a pointer phi, and the accumulators it selects
     * between -- five of them -- live in scratch memory from then on, loaded and stored around every MFMA */
    asm volatile("; end of ba_c_store<%0>" : : "n"(K));
}

template <int R> /* 16-row tiles of the dense pose block; NF = free keyframes this instantiation holds */
__global__ void __launch_bounds__(BA_T, 2)
k_ba_schur_c(BaDims d, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sRtfAll[4][BA_SMALL_MAXF * 12]; /* per wavefront: its window's free keyframes at the linearisation state: R, t */
    __shared__ unsigned ctab[BA_CTAB_ROWS * 64]; /* where the block products' accumulator entries go (BaCGeom::where) */
    constexpr int NF = (R == 1) ? 2 : (R == 2) ? 5 : (R == 3) ? 8 : BA_SMALL_MAXF;
    constexpr int NPAIR = NF * (NF + 1) / 2;
#ifdef BA_TIMING
    const unsigned long long tstart_ = __builtin_readcyclecounter();
#endif
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = tid; i < BA_CTAB_ROWS * 64; i += BA_T) ctab[i] = ba_cwhere.v[i];
    __syncthreads();
    /* which window, and which of its wavefronts: a 1-D grid of exactly the units the batch has (a (G, W) grid with idle
     * workgroups for the windows that have one fewer pushed real ones out of the resident round -- 172 windows ran 1.43 x
     * as long as 171 -- and, at four per window, parked all idle ones on two of the eight XCDs) */
    int w, wv, g0 = 0;
    if (d.wgReduce) {
        ba_schur_unit(blockIdx.x, d.Gbase, d.Gextra, w, g0);
        wv = 4 * g0 + wave;
    } else {
        const int u = blockIdx.x * 4 + wave;
        if (u >= d.Vbase * d.W + d.Vextra) return; /* the last workgroup's spare wavefronts (no barrier below on this path) */
        ba_schur_unit(u, d.Vbase, d.Vextra, w, wv);
    }
    w = __builtin_amdgcn_readfirstlane(w); wv = __builtin_amdgcn_readfirstlane(wv);
    const BaState st = states[w];
    if (st.status) return;
    double* sRtf = sRtfAll[wave];
    double* Zt = lds + (size_t)wave * d.schurWaveLds;          /* the group's tile, then its compact result */
    double* Hi = Zt + (d.schurWaveLds - BA_RECS_LDS - BA_ZERO_LDS); /* the group's point records, then a block of zeros */
    const int zeroOfs = d.schurWaveLds - BA_ZERO_LDS;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    for (int k = lane; k < d.nfree; k += 64) ba_pose_to_Rt(D + d.oT + ((size_t)st.cur * d.nkf + d.nfixed + k) * 7, sRtf + k * 12);
    /* dense accumulators: lane p < NPAIR = block pair (a >= b) of free keyframes, register 6 i + j = entry (i, j) of its
     * 6 x 6 block -- a group's compact blocks are added with one LDS read per register at a per-lane base address */
    double S[36];
#pragma unroll
    for (int e = 0; e < 36; e++) S[e] = 0;
    double rhs = 0;  /* lane = dense row */
    int pa = 0;      /* this lane's pair: p = pa (pa + 1) / 2 + pb */
    while ((pa + 1) * (pa + 2) / 2 <= lane) pa++;
    const int pb = lane - pa * (pa + 1) / 2;
    if (lane < BA_ZERO_LDS) Zt[zeroOfs + lane] = 0;
    ba_wave_lds_fence();
    const double delta = (double)sqrtf(5.991f);
    const int lastE = d.obs_pitch - 1;
    const double* Hq = D + d.oHq;
    const int4* KPs = reinterpret_cast<const int4*>(I + d.oKPs);
    const int4* GD = reinterpret_cast<const int4*>(I + d.oGDesc);
    const unsigned lastQ = (unsigned)d.npt * BA_REC - 1u;
    /* every wavefront takes a contiguous run of groups: the groups are in pattern order, so consecutive ones mostly share
     * their pattern and keep adding into the same product accumulators */
    const int gBeg = I[d.oGCut + wv], gEnd = I[d.oGCut + wv + 1], lastG = gEnd - 1;
    auto range = [&](BaPreC& X, int g) {
        X.nxt = GD[min(g, max(lastG, 0))];
        if (g > lastG) X.nxt.w = 0; /* past the end: an empty group */
    };
    auto preload = [&](BaPreC& X, int g) { /* X.nxt = descriptor of group g (fetched one fill earlier); then the one of g + 2 */
        const int4 gd = X.nxt;
        const int4 r = KPs[(unsigned)min(gd.y + lane, lastE)];
        X.key = (lane < gd.w * __popc(gd.z)) ? r.x : -1;
        X.u = __int_as_float(r.y); X.v = __int_as_float(r.z); X.w = __int_as_float(r.w);
        const unsigned qb = (unsigned)gd.x * BA_REC + (unsigned)lane;
        X.r0 = Hq[min(qb, lastQ)];
        X.r1 = Hq[min(qb + 64u, lastQ)];
        X.r2 = Hq[min(qb + 128u, lastQ)];
        X.r3 = Hq[min(qb + 192u, lastQ)];
        X.cur = gd;
        range(X, g + 2);
    };
#ifdef BA_TIMING
    unsigned long long tk_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t0_ = __builtin_readcyclecounter();
    tk_[4] = t0_ - tstart_; /* prologue */
#endif
    double acc[BA_CACC]; /* block products of the pattern `pend` that are not in the dense accumulators yet */
#pragma unroll
    for (int i = 0; i < BA_CACC; i++) acc[i] = 0;
    int pend = 0;
    /* products of pattern m: accumulators -> compact result -> dense accumulators. Block pair (a >= b) of the pattern is
     * the compact block of the two keyframes' slots; pairs the pattern does not have read the zeros. A dozen reads in
     * flight at a time. */
    auto finish = [&](int m) {
        const int k = __popc(m);
        switch (k) {
            case 1: ba_c_store<1>(acc, Zt, ctab, lane); break;
            case 2: ba_c_store<2>(acc, Zt, ctab, lane); break;
            case 3: if constexpr (NF >= 3) ba_c_store<3>(acc, Zt, ctab, lane); break;
            case 4: if constexpr (NF >= 4) ba_c_store<4>(acc, Zt, ctab, lane); break;
            default: if constexpr (NF >= 5) ba_c_store<5>(acc, Zt, ctab, lane); break;
        }
        const bool has = lane < NPAIR && ((m >> pa) & 1) && ((m >> pb) & 1);
        const int sa = __popc(m & ((1 << pa) - 1)), sb = __popc(m & ((1 << pb) - 1));
        const int ra = min(lane / 6, NF - 1), i6 = lane - 6 * (lane / 6);
        const bool hasr = lane < 6 * NF && ((m >> ra) & 1);
        const double* cb = Zt + (has ? BA_CB * (sa * (sa + 1) / 2 + sb) : zeroOfs);
#pragma unroll
        for (int e0 = 0; e0 < 36; e0 += 12) {
            double t[12];
#pragma unroll
            for (int e = 0; e < 12; e++) t[e] = cb[e0 + e];
#pragma unroll
            for (int e = 0; e < 12; e++) S[e0 + e] += t[e];
            __builtin_amdgcn_sched_barrier(0);
        }
        rhs += Zt[hasr ? BA_CB * (k * (k + 1) / 2) + 6 * __popc(m & ((1 << ra) - 1)) + i6 : zeroOfs];
        ba_wave_lds_fence();
    };
    auto group = [&](BaPreC& X, int g) {
        BA_TK(5);
        const int mask = __builtin_amdgcn_readfirstlane(X.cur.z), npts = __builtin_amdgcn_readfirstlane(X.cur.w);
        const int k = __popc(mask), ld = ba_ctab.ld[k];
        if (pend != 0 && pend != mask) { finish(pend); pend = 0; } /* the compact result goes through the tile's storage: before the tile is rewritten */
        BA_TK(3);
        Hi[lane] = X.r0;
        Hi[64 + lane] = X.r1;
        Hi[128 + lane] = X.r2;
        Hi[192 + lane] = X.r3;
        ba_wave_lds_fence();
        /* this lane's edge: linearise at the stored state, one Z block (6 x 3) into the compact tile */
        const bool live = X.key >= 0;
        const int pl = live ? (lane * ((65536 + k - 1) / k)) >> 16 : 0; /* lane / k, exact for lane < 64 */
        const int slot = live ? lane - pl * k : 0, kf = live ? (X.key & 63) : 0;
        if (live) {
            const double* q = Hi + pl * BA_REC;
            const double u00 = q[0], u01 = q[1], u02 = q[2], u11 = q[3], u12 = q[4], u22 = q[5];
            const double Xp[3] = {q[9], q[10], q[11]};
            BaLin L;
            double Jp[12];
            ba_linearize(sRtf + kf * 12, Xp, X.u, X.v, X.w, d.fx, d.fy, d.cx, d.cy, delta, L);
            ba_jac_pose_iz(L.pc, L.invz, d.fx, d.fy, Jp);
            /* Z = Hpl U = (ww Jp)^T (Jl U): the 2 x 3 factor Jl U first, then 6 rows of two products each */
            double JU[6];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                JU[3 * r] = L.Jl[3 * r] * u00;
                JU[3 * r + 1] = fma(L.Jl[3 * r], u01, L.Jl[3 * r + 1] * u11);
                JU[3 * r + 2] = fma(L.Jl[3 * r], u02, fma(L.Jl[3 * r + 1], u12, L.Jl[3 * r + 2] * u22));
            }
            double* z = Zt + (6 * slot) * ld + 3 * pl;
#pragma unroll
            for (int i = 0; i < 6; i++) JU[i] *= L.ww; /* the weight once, on the 2 x 3 factor */
#pragma unroll
            for (int a = 0; a < 6; a++) {
                /* rows 3 and 4 of Jp^T have one structural zero each (ba_jac_pose_iz: J[9], J[4]): one product, not two */
#pragma unroll
                for (int c = 0; c < 3; c++)
                    z[a * ld + c] = (a == 3) ? Jp[3] * JU[c] : (a == 4) ? Jp[10] * JU[3 + c] : fma(Jp[a], JU[c], Jp[6 + a] * JU[3 + c]);
            }
            if (slot == 0) { /* the rhs row: U^T bl of the point under its three columns */
                double* zr = Zt + (6 * k) * ld + 3 * pl;
                ba_rec_utb(q, zr);
            }
        }
        const int ncol = 3 * npts, nks = (ncol + 3) >> 2;
        if (lane <= 6 * k) { /* columns that pad the last k-step: zero in every row that is read back */
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (ncol + c < 4 * nks) Zt[lane * ld + ncol + c] = 0;
        }
        ba_wave_lds_fence();
        BA_TK(0);
        /* this set is free again: issue the loads of the group it holds next, before the products */
        preload(X, g + 2);
        BA_TK(1);
        if (k <= BA_KMFMA) {
            switch (k) {
                case 1: ba_c_mac<1>(acc, Zt, nks, lane); break;
                case 2: ba_c_mac<2>(acc, Zt, nks, lane); break;
                case 3: if constexpr (NF >= 3) ba_c_mac<3>(acc, Zt, nks, lane); break;
                case 4: if constexpr (NF >= 4) ba_c_mac<4>(acc, Zt, nks, lane); break;
                default: if constexpr (NF >= 5) ba_c_mac<5>(acc, Zt, nks, lane); break;
            }
            pend = mask;
        } else if constexpr (NF > BA_KMFMA) {
            /* patterns of more than BA_KMFMA keyframes: the 6 x 6 block products on the vector ALU, straight into the
             * dense accumulators -- lane = block pair, per tile column six values of either keyframe's rows and 36
             * multiply-adds; no compact result, no extra registers. About 1.5 x the time of the dense-tile kernel of round 2
             * on windows where every keyframe sees every point, the price of keeping the common sparse case lean. */
            const bool has = lane < NPAIR && ((mask >> pa) & 1) && ((mask >> pb) & 1);
            const int sa = __popc(mask & ((1 << pa) - 1)), sb = __popc(mask & ((1 << pb) - 1));
            const int ra = min(lane / 6, NF - 1), i6 = lane - 6 * (lane / 6);
            const bool hasr = lane < 6 * NF && ((mask >> ra) & 1);
            const int sr = __popc(mask & ((1 << ra) - 1));
            if (has) {
                const double* za = Zt + 6 * sa * ld;
                const double* zb = Zt + 6 * sb * ld;
#pragma unroll 1
                for (int c = 0; c < ncol; c++, za++, zb++) {
                    double bv[6];
#pragma unroll
                    for (int j = 0; j < 6; j++) bv[j] = zb[j * ld];
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double av = za[i * ld];
#pragma unroll
                        for (int j = 0; j < 6; j++) S[6 * i + j] = fma(av, bv[j], S[6 * i + j]);
                    }
                }
            }
            if (hasr) {
                const double* zr = Zt + (6 * sr + i6) * ld;
                const double* zu = Zt + 6 * k * ld;
#pragma unroll 1
                for (int c = 0; c < ncol; c++) rhs = fma(zr[c], zu[c], rhs);
            }
            ba_wave_lds_fence();
        }
        BA_TK(2);
#ifdef BA_TIMING
        tk_[6] += 1; tk_[7] += (unsigned long long)npts;
#endif
    };
    if (gBeg < gEnd) {
        BaPreC A, B;
        int g = gBeg;
        range(A, g);
        range(B, g + 1);
        preload(A, g);
        preload(B, g + 1);
        for (; g + 1 < gEnd; g += 2) {
            group(A, g);
            group(B, g + 1);
        }
        if (g < gEnd) group(A, g);
        if (pend != 0) finish(pend);
    }
#ifdef BA_TIMING
    BA_TK(8); /* first preload + tail of the loop */
#endif
    /* every wavefront writes its own partial system in the 64 x 64 layout k_ba_solve reads (lower triangle at [row][col],
     * reduced rhs in column np): lane = block pair, its 36 entries; k_ba_solve adds the 4 G partials of the window in
     * wavefront order. (Rounds 1-2 summed the four wavefronts through LDS first: a barrier -- every wavefront waiting for
     * the slowest -- and four serial passes, 8 % of the kernel. Small batches still do: with tens of workgroups per window
     * the single workgroup of k_ba_solve would add four times as many partial systems.) */
    if (d.wgReduce) {
        __syncthreads(); /* every wave is past its last tile read: the tile storage becomes the 64 x 64 sum */
        double* sum = lds;
        for (int wq = 0; wq < 4; wq++) {
            if (wave == wq) {
                if (lane < NPAIR) {
#pragma unroll
                    for (int e = 0; e < 36; e++) {
                        const int idx = (6 * pa + e / 6) * 64 + 6 * pb + e % 6;
                        sum[idx] = (wq == 0) ? S[e] : sum[idx] + S[e];
                    }
                }
                ba_wave_lds_fence();
                if (lane < d.np) sum[lane * 64 + d.np] = (wq == 0) ? rhs : sum[lane * 64 + d.np] + rhs;
            }
            __syncthreads();
        }
        double* out = D + d.oPartS + (size_t)g0 * 64 * 64;
        for (int i = tid; i < 64 * 64; i += BA_T) {
            const int r = i >> 6, c = i & 63;
            if (r < d.np && (c <= r || c == d.np)) out[i] = sum[i];
        }
    } else {
        double* out = D + d.oPartS + (size_t)wv * 64 * 64;
        if (lane < NPAIR) {
#pragma unroll
            for (int e = 0; e < 36; e++) out[(6 * pa + e / 6) * 64 + 6 * pb + e % 6] = S[e];
        }
        if (lane < d.np) out[lane * 64 + d.np] = rhs;
    }
#ifdef BA_TIMING
    BA_TK(9); /* epilogue */
    if (tid == 0 && (w & 15) == 0) { for (int i = 0; i < 10; i++) atomicAdd(&ba_times[i], tk_[i]); atomicAdd(&ba_times[10], 1ull); }
#endif
}

/* ---- E: assemble S (lower triangle), Cholesky in registers, pose update */
/* 1 / sqrt(x) for x > 0: v_rsq_f64 refined by two Newton steps (relative error ~1e-16). The Cholesky below needs a square
 * root and a reciprocal per column, on its critical path: the IEEE sqrt and division sequences are ~40 instructions each. */
__device__ __forceinline__ double ba_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    r = fma(r, fma(-h * r, r, 0.5), r);
    r = fma(r, fma(-h * r, r, 0.5), r);
    return r;
}
#define BA_SOLVE_T 256 /* threads of k_ba_solve: all of them assemble, one wavefront factorises (its rows + L^T need ~200 registers: no more than four wavefronts) */
template <int NS> /* padded system size: np rounded up to 16 */
__global__ void __launch_bounds__(BA_SOLVE_T)
k_ba_solve(BaDims d, double* __restrict__ dw, const int* __restrict__ iw, BaState* __restrict__ states, int with_reduce) {
    __shared__ double A[64 * 65];
    __shared__ double x[64];
    __shared__ double Lcol[2][64];
    const int w = blockIdx.x, tid = threadIdx.x;
#ifdef BA_TIMING
    unsigned long long ts_[6]; ts_[0] = __builtin_readcyclecounter();
#endif
    BaState* st = states + w;
    if (with_reduce) { /* the keyframe pass's partials -> Hpp, bp, chi2 (trials after the first: see ba_reduce_body) */
        __shared__ double redf[4];
        if (st->status) return;
        if (st->need_lin) ba_reduce_body(d, dw, iw, states, w, redf);
        __threadfence_block();
        __syncthreads();
    }
    double* D = dw + (size_t)w * d.wstride;
    const int np = d.np, nPart = d.wgReduce ? ba_schur_waves(d, w) / 4 : ba_schur_waves(d, w); /* one partial system per Schur workgroup or per wavefront */
    /* Assembly: S = Hpp + lambda I - sum of the partial systems (lower triangle), rhs = bp - sum of the partial rhs (kept as
     * row np of A). Every thread owns up to BA_SOLVE_E entries of the two together and adds the partials in order. The kernel
     * is a chain of memory latencies in front of a one-wavefront factorisation (~2 us each: the partials come from other
     * XCDs' L2s), so the loads are issued as early and as many at a time as registers allow: addresses first (they do not
     * depend on the window's state), the first BA_SOLVE_G partials of every entry and its Hpp / bp value in one go -- 12
     * partials, all a large batch has, are ONE round trip -- and only then the state (status, lambda), which arrives
     * with them. (Rounds 2-3: state, then 4 partials per trip, then Hpp: eight round trips at 20 partials.) */
    constexpr int BA_SOLVE_E = (NS * (NS + 1) / 2 + NS + BA_SOLVE_T - 1) / BA_SOLVE_T;
    constexpr int BA_SOLVE_G = (BA_SOLVE_E <= 5) ? 12 : 6; /* partials in flight per entry: what the registers hold */
    {
        const int ne = np * (np + 1) / 2, nall = ne + np;
        int dst[BA_SOLVE_E];          /* where the entry goes in A */
        bool diag[BA_SOLVE_E];
        const double* ps[BA_SOLVE_E];
        double acc[BA_SOLVE_E], h[BA_SOLVE_E];
        double t[BA_SOLVE_G][BA_SOLVE_E];
#pragma unroll
        for (int k = 0; k < BA_SOLVE_E; k++) {
            const int e = min(tid + k * BA_SOLVE_T, nall - 1);
            int r, c;
            const double* hp;
            if (e < ne) {
                r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
                while ((r + 1) * (r + 2) / 2 <= e) r++;
                while (r * (r + 1) / 2 > e) r--;
                c = e - r * (r + 1) / 2;
                hp = (r / 6 == c / 6) ? D + d.oHpp + (size_t)(r / 6) * 36 + (r % 6) * 6 + (c % 6) : nullptr;
                dst[k] = r * 65 + c;
            } else {
                r = e - ne; c = np;
                hp = D + d.oBp + r;
                dst[k] = np * 65 + r;
            }
            diag[k] = r == c;
            ps[k] = D + d.oPartS + r * 64 + c;
            acc[k] = 0;
            h[k] = hp ? *hp : 0.0;
#pragma unroll
            for (int g = 0; g < BA_SOLVE_G; g++) t[g][k] = ps[k][(size_t)min(g, nPart - 1) * 4096];
        }
        if (st->status) return;
        const double lambda = st->lambda;
        for (int g0 = 0; g0 < nPart; g0 += BA_SOLVE_G) { /* adds in partial order; further trips only for small batches */
            if (g0 > 0) {
#pragma unroll
                for (int g = 0; g < BA_SOLVE_G; g++)
#pragma unroll
                    for (int k = 0; k < BA_SOLVE_E; k++) t[g][k] = ps[k][(size_t)min(g0 + g, nPart - 1) * 4096];
            }
#pragma unroll
            for (int g = 0; g < BA_SOLVE_G; g++)
#pragma unroll
                for (int k = 0; k < BA_SOLVE_E; k++) acc[k] += (g0 + g < nPart) ? t[g][k] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < BA_SOLVE_E; k++) {
            if (tid + k * BA_SOLVE_T >= nall) continue;
            A[dst[k]] = (diag[k] ? h[k] + lambda : h[k]) - acc[k];
        }
    }
    const double lambda = st->lambda;
    __syncthreads();
#ifdef BA_TIMING
    ts_[1] = __builtin_readcyclecounter();
#endif
    /* The matrix lives in REGISTERS: lane i holds row i of the 64 x 64 system (rows >= np are identity, so the padded part
     * factors to itself), right-looking Cholesky on the lower triangle, no forward substitution (the rhs is one more row),
     * back-substitution by ONE wavefront on a register copy of L^T (lane i = column i, transposed once through LDS). Rounds
     * 1-2: one wavefront, columns broadcast with v_readlane, IEEE square root and division per column, branchy triangular
     * solves: 54 us per launch; round 3: 28 us (171 windows). */
    /* Factorisation on all four wavefronts (round 3, last change): lane i of EVERY wavefront is row i, wavefront v keeps the
     * columns k with k % 4 == v. Column j's owner forms the pivot's reciprocal square root, scales its column and publishes
     * it (LDS, double-buffered by column parity); after one barrier every wavefront subtracts it from ITS columns. The lone
     * wavefront of rounds 1-3 was bound by its instruction count (~5000 in this loop; a version blocked by keyframe, with an
     * eighth of the cross-lane exchanges, took the same time): here each wavefront issues a quarter of the multiply-adds and
     * broadcast reads. */
    __shared__ double dinvS[64];
    __shared__ int goodS;
    const int i = tid & 63, wv = tid >> 6;
    constexpr int NC = NS / 4; /* columns per wavefront */
    double myc[NC];
#pragma unroll
    for (int kl = 0; kl < NC; kl++) {
        /* lane np carries the reduced rhs (row np of A) as one more row below the matrix: the column steps turn it into
         * y = L^-1 rhs -- no forward substitution. Unconditional reads + selects: conditional ones became branches. */
        const int k = 4 * kl + wv;
        const double a = A[min(i, np) * 65 + k];
        myc[kl] = (i <= np && k < np && k <= i) ? a : ((k == i) ? 1.0 : 0.0);
    }
    if (tid == 0) goodS = st->sing == 0 ? 1 : 0;
    if (tid < 64) dinvS[tid] = 1.0;
    __syncthreads(); /* every wavefront has its columns out of A: A is free until the transpose */
#pragma unroll
    for (int j = 0; j < NS; j++) {
        double* Lc = Lcol[j & 1];
        if (wv == (j & 3)) { /* the owner of column j (wave-uniform) */
            constexpr int dummy = 0; (void)dummy;
            double& cj = myc[j >> 2];
            /* padding columns (j >= np) are identity -- and lane np, the rhs row, must not be read as a pivot */
            const double djr = ba_readlane(cj, j);
            const double dj = (j < np) ? djr : 1.0;
            const bool ok = (dj > 0) && isfinite(dj);
            const double sg = ok ? dj : 1.0;
            const double isj = ba_rsqrt(sg), sj = sg * isj;
            cj = (i == j) ? sj : cj * isj; /* lanes i < j hold unused upper-triangle values */
            Lc[i] = cj;
            if (i == j) { dinvS[j] = isj; if (!ok) goodS = 0; }
        }
        __syncthreads();
        const double lij = Lc[i];
#pragma unroll
        for (int kl = 0; kl < NC; kl++) {
            const int k = 4 * kl + wv; /* only lanes i >= k are ever read back */
            if (4 * kl + 3 > j) myc[kl] = (k > j) ? fma(-lij, Lc[k], myc[kl]) : myc[kl];
        }
    }
    /* L (lower triangle, the rhs row = y in row np) back into A for the back-substitution's transposed read */
    if (i < NS || i == np) {
#pragma unroll
        for (int kl = 0; kl < NC; kl++) {
            const int k = 4 * kl + wv;
            A[i * 65 + k] = (k <= i) ? myc[kl] : 0.0;
        }
    }
    __syncthreads();
#ifdef BA_TIMING
    if (tid == 0) ts_[2] = __builtin_readcyclecounter();
#endif
    if (tid < 64) {
        const bool good = goodS != 0;
        const double dinv = dinvS[i]; /* 1 / L[i][i] */
        /* L^T into registers: lane i gets column i of L; lane np's row is y */
        double col[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) col[k] = A[k * 65 + min(i, NS - 1)]; /* L[k][i], zero for k < i */
        double xi = (i < np) ? A[np * 65 + i] : 0.0, xfin = 0.0;
#pragma unroll
        for (int j = NS - 1; j >= 0; j--) { /* backward: L^T x = y. Straight-line: every lane scales, lane j's product is x_j,
                                             * every lane subtracts (col[j] is zero for the lanes above j; lane j's own xi is
                                             * not read again). The branchy form cost 300 clocks per step. */
            const double xjr = ba_readlane(xi * dinv, j);
            const double xj = (j < np) ? xjr : 0.0;
            xfin = (i == j) ? xj : xfin;
            xi = fma(-col[j], xj, xi);
        }
        xi = xfin;
#ifdef BA_TIMING
        ts_[3] = __builtin_readcyclecounter();
#endif
        if (!good) xi = 0;
        double term = 0.0;
        if (i < np) {
            x[i] = xi;
            D[d.oXp + i] = xi;
            term = xi * (lambda * xi + D[d.oBp + i]);
        }
        const double sc = po_wave_sum(term);
        if (i == 0) { st->scale_p = sc; st->ok2 = good ? 1 : 0; }
    }
    __syncthreads();
    const double* T = D + d.oT + (size_t)st->cur * d.nkf * 7;
    double* Tn = D + d.oT + (size_t)(st->cur ^ 1) * d.nkf * 7;
    for (int k = tid; k < d.nkf; k += BA_SOLVE_T) {
        const PoSE3 Tk = ba_load_se3(T + k * 7);
        if (k < d.nfixed) ba_store_se3(Tn + k * 7, Tk);
        else {
            double u[6];
            for (int a = 0; a < 6; a++) u[a] = x[6 * (k - d.nfixed) + a];
            ba_store_se3(Tn + k * 7, po_exp_mul(u, Tk));
        }
    }
#ifdef BA_TIMING
    if (tid == 0) {
        ts_[4] = __builtin_readcyclecounter();
        atomicAdd(&ba_times[11], ts_[1] - ts_[0]); atomicAdd(&ba_times[12], ts_[2] - ts_[1]); atomicAdd(&ba_times[13], ts_[3] - ts_[2]);
        atomicAdd(&ba_times[14], ts_[4] - ts_[3]); atomicAdd(&ba_times[15], 1ull);
    }
#endif
}

/* ---- large windows (11..64 free keyframes, reduced system up to 384 x 384; SURVEY a17's 50-keyframe case).
 * The 64 x 64 MFMA tile set above does not hold them, and S' = sum_l Z_l Z_l^T is block sparse per point (a point seen
 * by E free keyframes touches E (E + 1) / 2 of the 6 x 6 blocks: ~10 % fill at 48 free keyframes), so the large path is
 * organised by OUTPUT block instead:
 *   setup, once per call: for every block pair (a >= b) the list of (edge of a, edge of b) items whose point both
 *     keyframes see, in ascending edge order (k_ba_pairs, count pass + scan + fill pass; a wavefront per keyframe a
 *     ranks its edges per b with ballots, so the order is fixed without sorting);
 *   per trial: k_ba_schur_pairs gives each pair one wavefront, lane = item (both Z = Hpl U blocks rebuilt from the
 *     16-byte edge records), 36 register accumulators, a fixed butterfly sum, and writes the damped reduced system (and
 *     the rhs, as row np) directly -- no partial matrices, no atomics;
 *     k_ba_solve_big factors it panel by panel in LDS. */
__device__ __forceinline__ int ba_pair_index(int a, int b) { return a * (a + 1) / 2 + b; }

template <bool FILL>
__global__ void __launch_bounds__(64)
k_ba_pairs(BaDims d, const tb_ba_obs* __restrict__ obsAll, int* __restrict__ iw, const int* __restrict__ errflag) {
    __shared__ int tb[64 * 65]; /* [lane][free keyframe b] -> compact edge of (b, this lane's point), or -1 */
    const int w = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    if (errflag[w]) return;
    const tb_ba_obs* obs = obsAll + (size_t)w * d.obs_pitch;
    int* I = iw + (size_t)w * d.istride;
    const int4* KP = reinterpret_cast<const int4*>(I + d.oFreeKP);
    for (int i = lane; i < 64 * 65; i += 64) tb[i] = -1;
    const int l0 = I[d.oKfStart + d.nfixed + a], l1 = I[d.oKfStart + d.nfixed + a + 1];
    const unsigned long long ltmask = (1ull << lane) - 1ull;
    int cnt = 0; /* lane b: items of pair (a, b) so far */
    const int base = (FILL && lane <= a) ? I[d.oPairStart + ba_pair_index(a, lane)] : 0;
    __syncthreads();
    for (int r0 = l0; r0 < l1; r0 += 64) {
        const bool valid = r0 + lane < l1;
        int f0 = 0, f1 = 0;
        if (valid) {
            const int p = obs[I[d.oKfEdges + r0 + lane]].pt;
            f0 = I[d.oPtFree + p];
            f1 = min(I[d.oPtFree + p + 1], f0 + BA_BIG_MAXF);
            for (int j = f0; j < f1; j++) tb[lane * 65 + (KP[j].x & 63)] = j;
        }
        ba_wave_lds_fence();
        const int ea = tb[lane * 65 + a];
        for (int b = 0; b <= a; b++) {
            const int eb = tb[lane * 65 + b];
            const unsigned long long m = __ballot(valid && eb >= 0);
            if (m == 0) continue;
            const int at = __builtin_amdgcn_readlane(base, b) + __builtin_amdgcn_readlane(cnt, b) + __popcll(m & ltmask);
            if (FILL && valid && eb >= 0) *reinterpret_cast<int2*>(I + d.oPairItems + 2 * (size_t)at) = make_int2(ea, eb);
            if (lane == b) cnt += __popcll(m);
        }
        ba_wave_lds_fence();
        for (int j = f0; j < f1; j++) tb[lane * 65 + (KP[j].x & 63)] = -1;
        ba_wave_lds_fence();
    }
    if (!FILL && lane <= a) I[d.oPairCnt + ba_pair_index(a, lane)] = cnt;
}

__global__ void __launch_bounds__(BA_T)
k_ba_pair_scan(BaDims d, int* __restrict__ iw, const int* __restrict__ errflag) {
    __shared__ int tot[BA_T];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (errflag[w]) return;
    int* I = iw + (size_t)w * d.istride;
    const int per = (d.npairs + BA_T - 1) / BA_T, i0 = min(tid * per, d.npairs), i1 = min(i0 + per, d.npairs);
    int sum = 0;
    for (int i = i0; i < i1; i++) sum += I[d.oPairCnt + i];
    tot[tid] = sum;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < tid; t++) run += tot[t];
    for (int i = i0; i < i1; i++) { I[d.oPairStart + i] = run; run += I[d.oPairCnt + i]; }
    if (tid == BA_T - 1) I[d.oPairStart + d.npairs] = run;
}

/* Z = Hpl U = (ww Jp)^T (Jl U) (6 x 3, row-major) of one free-keyframe edge from its 16-byte record and its point's
 * record q = [U (6), bl (3), X (3)]; the same arithmetic as the tile fill of k_ba_schur */
__device__ __forceinline__ void ba_edge_z(const double* __restrict__ sRtf, const int4 r, const double* __restrict__ q,
                                          double fx, double fy, double cx, double cy, double delta, double* __restrict__ z) {
    const double u00 = q[0], u01 = q[1], u02 = q[2], u11 = q[3], u12 = q[4], u22 = q[5];
    const double Xp[3] = {q[9], q[10], q[11]};
    BaLin L;
    double Jp[12], JU[6];
    ba_linearize(sRtf + (r.x & 63) * 12, Xp, __int_as_float(r.y), __int_as_float(r.z), __int_as_float(r.w), fx, fy, cx, cy, delta, L);
    ba_jac_pose_iz(L.pc, L.invz, fx, fy, Jp);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        JU[3 * k] = L.Jl[3 * k] * u00;
        JU[3 * k + 1] = fma(L.Jl[3 * k], u01, L.Jl[3 * k + 1] * u11);
        JU[3 * k + 2] = fma(L.Jl[3 * k], u02, fma(L.Jl[3 * k + 1], u12, L.Jl[3 * k + 2] * u22));
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double p0w = L.ww * Jp[a], p1w = L.ww * Jp[6 + a];
        z[3 * a] = fma(p0w, JU[0], p1w * JU[3]);
        z[3 * a + 1] = fma(p0w, JU[1], p1w * JU[4]);
        z[3 * a + 2] = fma(p0w, JU[2], p1w * JU[5]);
    }
}

/* one wavefront per block pair (a >= b): A[6a.., 6b..] = [a == b] (Hpp_a + lambda I) - sum_items Z_ea Z_eb^T; the
 * diagonal pairs also give row np of A, the reduced rhs bp_a - sum Z U^T bl. Lane = item; both Z blocks are rebuilt
 * from the two 16-byte edge records and the point record they share (128 B per item; a stored Z would be 288 B per
 * item plus a pass that writes it), the FP64 work this costs is a few percent of the vector peak at these sizes. */
__global__ void __launch_bounds__(BA_T)
k_ba_schur_pairs(BaDims d, double* __restrict__ dw, const int* __restrict__ iw, const BaState* __restrict__ states) {
    __shared__ double sRtf[BA_BIG_MAXF * 12];
    const int w = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const BaState st = states[w];
    if (st.status) return;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    for (int k = tid; k < d.nfree; k += BA_T) ba_pose_to_Rt(D + d.oT + ((size_t)st.cur * d.nkf + d.nfixed + k) * 7, sRtf + k * 12);
    __syncthreads();
    const int pr = blockIdx.x * 4 + (tid >> 6);
    if (pr >= d.npairs) return; /* wave-uniform, no barriers below */
    int a = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= pr) a++;
    while (a * (a + 1) / 2 > pr) a--;
    const int b = pr - a * (a + 1) / 2;
    const int i0 = I[d.oPairStart + pr], i1 = I[d.oPairStart + pr + 1];
    const int2* items = reinterpret_cast<const int2*>(I + d.oPairItems);
    const int4* KP = reinterpret_cast<const int4*>(I + d.oFreeKP);
    const double delta = (double)sqrtf(5.991f);
    double acc[36], rh[6];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) rh[k] = 0;
    if (i0 < i1) {
        /* three-level fetch chain (item -> edge records -> point record), each level one round ahead of the next, so
         * every load has a round of arithmetic to land in; indices past the list are clamped and their lanes add zeros */
        const int last = i1 - 1;
        const double* Hq = D + d.oHq;
        int it = i0 + lane;
        int2 e2 = items[min(it + 64, last)];
        int4 ra0, rb0, ra1, rb1;
        { const int2 e0 = items[min(it, last)]; ra0 = KP[e0.x]; rb0 = KP[e0.y]; }
        ra1 = KP[e2.x]; rb1 = KP[e2.y];
        e2 = items[min(it + 128, last)];
        double2 q0[6];
        {
            const double2* q2 = reinterpret_cast<const double2*>(Hq + (size_t)((unsigned)ra0.x >> 6) * 12);
#pragma unroll
            for (int k = 0; k < 6; k++) q0[k] = q2[k];
        }
        for (int base = i0; base < i1; base += 64, it += 64) {
            const int2 e3 = items[min(it + 192, last)];
            const int4 ra2 = KP[e2.x], rb2 = KP[e2.y];
            double2 q1[6];
            {
                const double2* q2 = reinterpret_cast<const double2*>(Hq + (size_t)((unsigned)ra1.x >> 6) * 12);
#pragma unroll
                for (int k = 0; k < 6; k++) q1[k] = q2[k];
            }
            const bool live = it < i1;
            double q[12];
#pragma unroll
            for (int k = 0; k < 6; k++) { q[2 * k] = q0[k].x; q[2 * k + 1] = q0[k].y; }
            double za[18], zb[18];
            ba_edge_z(sRtf, ra0, q, d.fx, d.fy, d.cx, d.cy, delta, za);
#pragma unroll
            for (int k = 0; k < 18; k++) za[k] = live ? za[k] : 0.0;
            if (a == b) {
#pragma unroll
                for (int k = 0; k < 18; k++) zb[k] = za[k];
                double ub[3];
                ba_rec_utb(q, ub);
#pragma unroll
                for (int k = 0; k < 6; k++) rh[k] += za[3 * k] * ub[0] + za[3 * k + 1] * ub[1] + za[3 * k + 2] * ub[2];
            } else ba_edge_z(sRtf, rb0, q, d.fx, d.fy, d.cx, d.cy, delta, zb);
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++)
                    acc[6 * i + j] += za[3 * i] * zb[3 * j] + za[3 * i + 1] * zb[3 * j + 1] + za[3 * i + 2] * zb[3 * j + 2];
            ra0 = ra1; rb0 = rb1; ra1 = ra2; rb1 = rb2; e2 = e3;
#pragma unroll
            for (int k = 0; k < 6; k++) q0[k] = q1[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = po_wave_sum(acc[k]);
    double* A = D + d.oBigA;
    const int np = d.np;
    double mine = 0; /* lane k < 36 stores entry k */
#pragma unroll
    for (int k = 0; k < 36; k++) mine = (lane == k) ? acc[k] : mine;
    if (lane < 36) {
        const int i = lane / 6, j = lane - i * 6;
        double h = 0;
        if (a == b) h = D[d.oHpp + (size_t)a * 36 + lane] + ((i == j) ? st.lambda : 0.0);
        if (a != b || j <= i) A[(size_t)(6 * a + i) * np + 6 * b + j] = h - mine;
    }
    if (a == b) {
#pragma unroll
        for (int k = 0; k < 6; k++) rh[k] = po_wave_sum(rh[k]);
        double r = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) r = (lane == k) ? rh[k] : r;
        if (lane < 6) A[(size_t)np * np + 6 * a + lane] = D[d.oBp + 6 * a + lane] - r;
    }
}

/* Factor the damped reduced system of a large window and update the free poses; one workgroup per window. Right-looking
 * Cholesky on the lower triangle, BA_PB columns at a time: the panel (all rows below its diagonal block, plus row np =
 * the rhs, which turns into y = L^-1 rhs on the way) sits in LDS while its columns are eliminated, then every thread
 * applies the rank-BA_PB update to 4 x 4 register tiles of the trailing matrix in global memory (1.2 MB at np = 384,
 * L2 resident). The back-substitution walks the panels in reverse. */
#define BA_PB 32
#define BA_ST 1024 /* threads of the large-window solve: the trailing update and the row solves are data parallel */
#define BA_PLD (BA_PB + 1)
__global__ void __launch_bounds__(BA_ST)
k_ba_solve_big(BaDims d, double* __restrict__ dw, BaState* __restrict__ states) {
    extern __shared__ __attribute__((aligned(16))) double Pn[]; /* [np + 1 - k0][BA_PLD] */
    __shared__ double xs[6 * BA_BIG_MAXF], part[(BA_ST / BA_PB) * BA_PB], red[BA_ST / 64];
    const int w = blockIdx.x, tid = threadIdx.x;
    BaState* st = states + w;
    if (st->status) return;
    double* D = dw + (size_t)w * d.wstride;
    const int np = d.np;
    const double lambda = st->lambda;
    double* A = D + d.oBigA; /* [np + 1][np] */
    __shared__ double invd[BA_PB], Ld[BA_PB * BA_PLD];
    __shared__ int sgood;
    if (tid == 0) sgood = st->sing == 0;
    __syncthreads();
    for (int k0 = 0; k0 < np; k0 += BA_PB) {
        const int nb = min(BA_PB, np - k0), mr = np + 1 - k0;
        if (tid < 64) {
            /* diagonal block in one wavefront, lane = row, the row in registers, columns broadcast with readlane (as in
             * k_ba_solve); rows >= nb are identity and factor to themselves */
            const int r = tid;
            double dr[BA_PB];
#pragma unroll
            for (int c = 0; c < BA_PB; c++)
                dr[c] = (r < nb && c < nb) ? ((c <= r) ? A[(size_t)(k0 + r) * np + k0 + c] : 0.0) : ((c == r) ? 1.0 : 0.0);
            bool good = sgood != 0;
#pragma unroll
            for (int j = 0; j < BA_PB; j++) {
                const double dj = ba_readlane(dr[j], j);
                if (!(dj > 0) || !isfinite(dj)) good = false;
                const double sj = sqrt(good ? dj : 1.0), isj = 1.0 / sj;
                dr[j] = (r == j) ? sj : dr[j] * isj;
#pragma unroll
                for (int k = j + 1; k < BA_PB; k++) dr[k] -= dr[j] * ba_readlane(dr[j], k);
            }
            if (r < BA_PB) { /* identity-padded copy for the row solves below: no bounds tests in their inner loops */
#pragma unroll
                for (int c = 0; c < BA_PB; c++) {
                    Ld[r * BA_PLD + c] = (c <= r) ? dr[c] : 0.0;
                    if (c == r) invd[r] = 1.0 / dr[c];
                    if (r < nb && c <= r) A[(size_t)(k0 + r) * np + k0 + c] = dr[c];
                }
            }
            if (r == 0) sgood = good ? 1 : 0;
        }
        __syncthreads();
        /* rows below the block (and the rhs row): L[r][:] = A[r][:] L_d^-T, every thread its own row, no barriers;
         * columns >= nb of the panel are zero */
        static_assert(BA_ST > 6 * BA_BIG_MAXF, "one thread per row below the diagonal block");
        if (const int r = nb + tid; r < mr) { /* not a loop: the L_d reads below must not be hoisted out of one */
            double row[BA_PB];
            double* Ar = A + (size_t)(k0 + r) * np + k0;
#pragma unroll
            for (int c = 0; c < BA_PB; c++) { /* all 32 loads in flight (A is padded by a panel width), then masked */
                row[c] = Ar[c];
                asm volatile("" : "+v"(row[c]));
            }
#pragma unroll
            for (int c = 0; c < BA_PB; c++) row[c] = (c < nb) ? row[c] : 0.0;
#pragma unroll
            for (int c = 0; c < BA_PB; c++) {
                row[c] *= invd[c];
#pragma unroll
                for (int c2 = c + 1; c2 < BA_PB; c2++) row[c2] -= row[c] * Ld[c2 * BA_PLD + c];
                /* pin this column's updates here: left alone, the scheduler issues the broadcast reads of all 496
                 * steps first and spills them */
#pragma unroll
                for (int c2 = c + 1; c2 < BA_PB; c2++) asm volatile("" : "+v"(row[c2]) : : "memory");
            }
#pragma unroll
            for (int c = 0; c < BA_PB; c++) {
                Pn[r * BA_PLD + c] = row[c];
                if (c < nb) Ar[c] = row[c];
            }
        }
        __syncthreads();
        /* trailing update: rows i in [k0 + nb, np], columns j in [k0 + nb, min(i, np - 1)], 4 x 4 tiles (ti >= tj) */
        const int mt = np - k0 - nb;
        if (mt > 0) {
            const int nT = (mt + 1 + 3) >> 2, last = mr - 1;
            for (int t = tid; t < nT * (nT + 1) / 2; t += BA_ST) {
                int ti = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
                while (ti * (ti + 1) / 2 > t) ti--;
                const int tj = t - ti * (ti + 1) / 2;
                const int ra = nb + 4 * ti, rb = nb + 4 * tj; /* panel rows of the tile's rows / columns */
                double acc[4][4] = {};
#pragma unroll 4
                for (int c = 0; c < BA_PB; c++) { /* columns >= nb are zero */
                    double av[4], bv[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) { av[q] = Pn[min(ra + q, last) * BA_PLD + c]; bv[q] = Pn[min(rb + q, last) * BA_PLD + c]; }
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int s = 0; s < 4; s++) acc[q][s] = fma(av[q], bv[s], acc[q][s]);
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        const int i = k0 + ra + q, j = k0 + rb + s;
                        if (i <= np && j < np && j <= i) A[(size_t)i * np + j] -= acc[q][s];
                    }
            }
        }
        __syncthreads();
    }
    /* L^T x = y, panels in reverse; y = row np of the factored array */
    for (int i = tid; i < np; i += BA_ST) xs[i] = A[(size_t)np * np + i];
    __syncthreads();
    for (int k0 = ((np - 1) / BA_PB) * BA_PB; k0 >= 0; k0 -= BA_PB) {
        const int nb = min(BA_PB, np - k0), mr = np - k0;
        for (int idx = tid; idx < mr * nb; idx += BA_ST) {
            const int r = idx / nb, c = idx - r * nb;
            Pn[r * BA_PLD + c] = (c <= r) ? A[(size_t)(k0 + r) * np + k0 + c] : 0.0;
        }
        __syncthreads();
        {   /* sum_{i >= k0 + nb} L[i][k0 + c] x_i: BA_ST / BA_PB row classes per column, combined in order */
            const int c = tid & (BA_PB - 1), cls = tid >> 5;
            double s = 0;
            if (c < nb)
                for (int r = nb + cls; r < mr; r += BA_ST / BA_PB) s += Pn[r * BA_PLD + c] * xs[k0 + r];
            part[cls * BA_PB + c] = s;
        }
        __syncthreads();
        if (tid < 64) { /* the nb x nb triangle in one wavefront: lane c holds t_c */
            const int c = tid;
            double t = 0;
            if (c < nb) {
                double s = 0;
                for (int k = 0; k < BA_ST / BA_PB; k++) s += part[k * BA_PB + c];
                t = xs[k0 + c] - s;
            }
            for (int j = nb - 1; j >= 0; j--) {
                const double xj = ba_readlane(t, j) / Pn[j * BA_PLD + j];
                if (c == j) t = xj;
                else if (c < j) t -= Pn[j * BA_PLD + c] * xj;
            }
            if (c < nb) xs[k0 + c] = t;
        }
        __syncthreads();
    }
    const bool good = sgood != 0;
    double term = 0;
    for (int i = tid; i < np; i += BA_ST) {
        const double xi = good ? xs[i] : 0.0;
        xs[i] = xi;
        D[d.oXp + i] = xi;
        term += xi * (lambda * xi + D[d.oBp + i]);
    }
    term = po_wave_sum(term);
    if ((tid & 63) == 0) red[tid >> 6] = term;
    __syncthreads();
    if (tid == 0) {
        double sc = 0;
        for (int k = 0; k < BA_ST / 64; k++) sc += red[k];
        st->scale_p = sc; st->ok2 = good ? 1 : 0;
    }
    __syncthreads();
    const double* T = D + d.oT + (size_t)st->cur * d.nkf * 7;
    double* Tn = D + d.oT + (size_t)(st->cur ^ 1) * d.nkf * 7;
    for (int k = tid; k < d.nkf; k += BA_ST) {
        const PoSE3 Tk = ba_load_se3(T + k * 7);
        if (k < d.nfixed) ba_store_se3(Tn + k * 7, Tk);
        else {
            double u[6];
            for (int a = 0; a < 6; a++) u[a] = xs[6 * (k - d.nfixed) + a];
            ba_store_se3(Tn + k * 7, po_exp_mul(u, Tk));
        }
    }
}

/* ---- F: point back-substitution and trial errors (STREAM: as in the point pass) */
template <bool STREAM>
__global__ void __launch_bounds__(BA_T)
k_ba_update(BaDims d, const tb_ba_obs* __restrict__ obsAll, double* __restrict__ dw, const int* __restrict__ iw,
            const BaState* __restrict__ states) {
    __shared__ double red[4];
    /* dynamic shared memory sized by the window (see k_ba_points): trial poses, linearisation state, pose increments */
    extern __shared__ __attribute__((aligned(16))) double sdyn[];
    double* const sRt = sdyn;                      /* [nkf][12] trial poses */
    double* const sRtc = sdyn + (size_t)d.nkf * 12;/* [nkf][12] linearisation state */
    double* const sx = sdyn + (size_t)d.nkf * 24;  /* [np] */
    const int w = blockIdx.y, tid = threadIdx.x;
    double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    const int p = blockIdx.x * BA_T + tid;
    BaStreamPos sp;
    if (STREAM) sp = ba_stream_begin(d, I, p); /* in flight beside the state, the poses and the increments */
    /* the point record of this trial: A^-1 = U U^T (all zero for a singular block: xl stays 0), the gradient bl, and X at the
     * linearisation state -- the point pass (or k_ba_hinv) stored the very doubles of P there, so P is not read again */
    const bool in = p < d.npt;
    double q[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    /* renumbered windows (STREAM implies d.renum): the record sits at p, an address that is in range whatever the window's
     * state, so its load goes out beside the state's. The other windows find it through oPtRank, which k_ba_groups does not
     * write for a window that k_ba_setup rejected: there nothing is loaded before the status says the window runs. */
    if (STREAM && in) ba_load_rec(D + d.oHq + (size_t)p * 12, q);
    const BaState st = states[w];
    if (st.status) return;
    if (!STREAM && in) ba_load_rec(D + d.oHq + (size_t)(d.renum ? p : I[d.oPtRank + p]) * 12, q);
    const tb_ba_obs* obs = obsAll + (size_t)w * d.obs_pitch;
    const double* Tn = D + d.oT + (size_t)(st.cur ^ 1) * d.nkf * 7;
    for (int k = tid; k < d.nkf; k += BA_T) ba_pose_to_Rt(D + d.oT + ((size_t)st.cur * d.nkf + k) * 7, sRtc + k * 12);
    double* Pn = D + d.oP + (size_t)(st.cur ^ 1) * d.npt * 3;
    for (int k = tid; k < d.nkf; k += BA_T) ba_pose_to_Rt(Tn + k * 7, sRt + k * 12);
    for (int i = tid; i < d.np; i += BA_T) sx[i] = D[d.oXp + i];
    __syncthreads();
    const double delta = (double)sqrtf(5.991f);
    double chi = 0, sc = 0;
    double r[3] = {q[6], q[7], q[8]};
    const double bl[3] = {r[0], r[1], r[2]};
    const double Xc[3] = {q[9], q[10], q[11]};
    double xl[3] = {0, 0, 0}, X[3] = {0, 0, 0};
    /* r = bl - sum_k Hpl_k^T x_k with Hpl_k = ww Jp^T Jl rebuilt from the observation (a 144-byte block per edge
     * would cost more to fetch than its ~150 flops): Hpl^T x = ww Jl^T (Jp x) */
    auto back = [&](int kf, float ou, float ov, float ow) {
        if (kf < d.nfixed) return;
        BaLin L;
        double Jp[12];
        ba_linearize(sRtc + kf * 12, Xc, ou, ov, ow, d.fx, d.fy, d.cx, d.cy, delta, L);
        ba_jac_pose_iz(L.pc, L.invz, d.fx, d.fy, Jp);
        const double* xp = sx + 6 * (kf - d.nfixed);
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) { s0 = fma(Jp[a], xp[a], s0); s1 = fma(Jp[6 + a], xp[a], s1); }
#pragma unroll
        for (int c = 0; c < 3; c++) r[c] = fma(-L.ww, fma(L.Jl[c], s0, L.Jl[3 + c] * s1), r[c]);
    };
    auto step = [&]() { /* xl = U (U^T r), the trial point, the point's share of the gain's scale */
        if (st.ok2) {
            const double u00 = q[0], u01 = q[1], u02 = q[2], u11 = q[3], u12 = q[4], u22 = q[5];
            const double t0 = u00 * r[0], t1 = u01 * r[0] + u11 * r[1], t2 = u02 * r[0] + u12 * r[1] + u22 * r[2]; /* U^T r */
            xl[0] = u00 * t0 + u01 * t1 + u02 * t2;
            xl[1] = u11 * t1 + u12 * t2;
            xl[2] = u22 * t2;
        }
        for (int a = 0; a < 3; a++) {
            X[a] = Xc[a] + xl[a];
            Pn[3 * p + a] = X[a];
            sc += xl[a] * (st.lambda * xl[a] + bl[a]);
        }
    };
    auto trial = [&](int kf, float ou, float ov, float ow) {
        BaLin L; /* the same residual arithmetic as the point pass: rho compares like with like */
        ba_residual(sRt + kf * 12, X, ou, ov, ow, d.fx, d.fy, d.cx, d.cy, delta, L);
        chi += ba_huber_rho0(L.c2, delta);
    };
    if (STREAM) {
        /* both walks read the block's entries from the stream: the second finds them in the cache the first filled, and its
         * residuals are too short to cover a load each, so it fetches BA_UPD_BATCH slots at a time (the registers are there:
         * the kernel's count is set by the back-substitution) */
        const int4* S = reinterpret_cast<const int4*>(I + d.oFreeKP);
        if (st.ok2)
            ba_stream_walk(S, sp, [&](const int4& e) { back(e.x, __int_as_float(e.y), __int_as_float(e.z), __int_as_float(e.w)); });
        if (in) step();
        ba_stream_walk_batched<BA_UPD_BATCH>(S, sp, [&](const int4& e) { trial(e.x, __int_as_float(e.y), __int_as_float(e.z), __int_as_float(e.w)); });
    } else if (in) {
        const int eBeg = I[d.oPtStart + p], eEnd = I[d.oPtStart + p + 1];
        if (st.ok2) {
            tb_ba_obs on = obs[min(eBeg, d.obs_pitch - 1)]; /* next observation in flight while this one is processed */
            for (int e = eBeg; e < eEnd; e++) {
                const tb_ba_obs o = on;
                on = obs[min(e + 1, d.obs_pitch - 1)];
                back(o.kf, o.u, o.v, o.inv_sigma2);
            }
        }
        step();
        tb_ba_obs on2 = obs[min(eBeg, d.obs_pitch - 1)];
        for (int e = eBeg; e < eEnd; e++) {
            const tb_ba_obs o = on2;
            on2 = obs[min(e + 1, d.obs_pitch - 1)];
            trial(o.kf, o.u, o.v, o.inv_sigma2);
        }
    }
    const double s1 = ba_block_sum1(chi, red);
    const double s2 = ba_block_sum1(sc, red);
    if (tid == 0) {
        D[d.oPartP + (size_t)blockIdx.x * 4 + 2] = s1;
        D[d.oPartP + (size_t)blockIdx.x * 4 + 3] = s2;
    }
}

/* ---- G: accept / reject (g2o OptimizationAlgorithmLevenberg::solve), one thread per window */
__global__ void __launch_bounds__(64)
k_ba_decide(BaDims d, const double* __restrict__ dw, BaState* __restrict__ states, int* __restrict__ running) {
    /* one wavefront per window: the lanes fetch the point blocks' partial sums together and add them in a fixed tree (a
     * single thread walking 2 x nblkP dependent loads made this trivial kernel 8 us of every LM trial) */
    const int w = blockIdx.x, lane = threadIdx.x;
    BaState* st = states + w;
    if (st->status) return;
    const double* D = dw + (size_t)w * d.wstride;
    double tc = 0, sc = 0;
    for (int b = lane; b < d.nblkP; b += 64) { tc += D[d.oPartP + (size_t)b * 4 + 2]; sc += D[d.oPartP + (size_t)b * 4 + 3]; }
    tc = po_wave_sum(tc);
    sc = po_wave_sum(sc);
    if (lane != 0) return;
    double tempChi = tc, scale = st->scale_p + sc;
    if (!st->ok2) tempChi = 1.7976931348623157e308;
    scale += 1e-3;
    const double rho = (st->currentChi - tempChi) / scale;
    if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - pow(2 * rho - 1, 3);
        alpha = fmin(alpha, 2. / 3.);
        st->lambda *= fmax(1. / 3., alpha);
        st->ni = 2;
        st->currentChi = tempChi;
        st->cur ^= 1;
        st->need_lin = 1;
    } else {
        st->lambda *= st->ni;
        st->ni *= 2;
    }
    st->qmax++;
    st->rho = rho;
    st->sing = 0;
    st->hq_fresh = 0;
    if (!(rho < 0 && st->qmax < 10)) { /* this LM iteration is over */
        st->done_iters++;
        const bool terminate = (st->qmax == 10 || rho == 0);
        st->iter++;
        st->qmax = 0;
        st->need_lin = 1;
        if (terminate || st->iter >= d.iters) st->status = 1;
    }
    if (!st->status) atomicAdd(running, 1);
}

/* ---- write back */
__global__ void __launch_bounds__(BA_T)
k_ba_finish(BaDims d, const double* __restrict__ dw, const int* __restrict__ iw, const BaState* __restrict__ states,
            float* __restrict__ poses, float* __restrict__ pts, double* __restrict__ stats) {
    const int w = blockIdx.x, tid = threadIdx.x;
    const BaState st = states[w];
    const double* D = dw + (size_t)w * d.wstride;
    const int* I = iw + (size_t)w * d.istride;
    if (!st.err) {
        for (int k = tid; k < d.nkf; k += BA_T) {
            const PoSE3 s = ba_load_se3(D + d.oT + ((size_t)st.cur * d.nkf + k) * 7);
            double R[9];
            po_to_R(s, R);
            float* T = poses + ((size_t)w * d.nkf + k) * 16;
            for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)R[i * 3 + j]; }
            T[3] = (float)s.tx; T[7] = (float)s.ty; T[11] = (float)s.tz;
            T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
        }
        for (int i = tid; i < d.npt * 3; i += BA_T) { /* renumbered windows: back to the caller's point order */
            const int r = i / 3, c = i - 3 * r;
            pts[(size_t)w * d.npt * 3 + (d.renum ? 3 * (size_t)I[d.oPerm + r] + c : (size_t)i)] = (float)D[d.oP + (size_t)st.cur * d.npt * 3 + i];
        }
    }
    if (stats && tid == 0) {
        double* s = stats + 8 * w;
        s[0] = st.done_iters; s[1] = st.chi0; s[2] = st.currentChi; s[3] = st.lambda;
        s[4] = st.rho; s[5] = st.iter; s[6] = 0; s[7] = st.err ? -1.0 : 0.0;
    }
}

__global__ void k_ba_zero(int* __restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

static void ba_dims(BaDims& d, int num_cu, int peers, int W, const double K[4], int nkf, int nfixed, int npt, int obs_pitch, int iters) {
    memset(&d, 0, sizeof d);
    d.W = W; d.nkf = nkf; d.nfixed = nfixed; d.nfree = nkf - nfixed; d.np = 6 * d.nfree; d.npt = npt; d.obs_pitch = obs_pitch;
    d.iters = iters;
    d.nblkP = (npt + BA_T - 1) / BA_T;
    d.kfChunks = (obs_pitch + BA_KFCH - 1) / BA_KFCH;
    d.nChunks = 0;
    /* Schur workgroups: the kernel holds two per CU (226 registers per lane, ~62 KB of LDS), so the batch gets 2 num_cu of
     * them -- ONE resident round (855 workgroups for 171 windows ran as 1.67 rounds: the second, two-thirds full, cost as much
     * as the first) -- dealt to the windows as Gbase or Gbase + 1 each. A context that shares the GPU with `peers` - 1 others
     * running the same chain (tb_set_concurrency: the pipeline's BA partitions) takes 1 / peers of the slots: three
     * partitions of 171 windows queue 513 workgroups between them instead of 3 x 512 (measured: 18.37 -> 17.91 ms per step). At most 32 per window (k_ba_solve adds the
     * workgroups' partial systems in order) and no more than one per ~256 points. */
    {
        const int slots = std::max(2 * std::max(num_cu, 1) / std::max(peers, 1), 1), cap = std::min(32, std::max((npt / 64 + 3) / 4, 1));
        d.Gbase = std::min(std::max(slots / std::max(W, 1), 1), cap);
        d.Gextra = (d.Gbase < cap && slots > d.Gbase * W) ? std::min(slots - d.Gbase * W, W) : 0;
        d.G = d.Gbase + (d.Gextra > 0 ? 1 : 0);
        d.wgReduce = d.Gbase > 4 ? 1 : 0;
        /* large batches: the round's 4 x slots wavefronts dealt to the windows one by one -- with whole workgroups 171 windows
         * got three each but one of them two, and that window's wavefronts (half as many again to do) ended the launch */
        const int T = 4 * std::max(slots, W);
        d.Vbase = std::min(T / std::max(W, 1), 4 * cap);
        d.Vextra = d.Vbase < 4 * cap ? T % std::max(W, 1) : 0;
    }
    d.big = d.nfree > BA_SMALL_MAXF;
    d.renum = (!d.big && npt <= BA_SORT_LDS && nkf <= BA_PREP_MAXKF) ? 1 : 0;
    d.stream = d.renum;
    d.schurWaveLds = d.big ? 0 : ba_c_wave_lds(d.nfree);
    d.npairs = d.nfree * (d.nfree + 1) / 2;
    d.maxItems = (unsigned long long)obs_pitch * (d.nfree + 1) / 2 + 1; /* sum_p E_p (E_p + 1) / 2 with E_p <= nfree */
    d.fx = K[0]; d.fy = K[1]; d.cx = K[2]; d.cy = K[3];
    unsigned long long o = 0;
    auto take = [&](unsigned long long n) { unsigned long long r = o; o += (n + 1) & ~1ull; return r; };
    d.oT = take(2ull * nkf * 7);
    d.oP = take(2ull * npt * 3);
    d.oHll = take(6ull * npt);
    d.oBl = take(3ull * npt);
    d.oHq = take(12ull * npt);
    d.oHpp = take(36ull * std::max(d.nfree, 1));
    d.oBp = take(std::max(64, d.np));
    d.oXp = take(std::max(64, d.np));
    d.oPartKF = take(27ull * std::max(d.nfree, 1) * d.kfChunks);
    d.oPartP = take(4ull * d.nblkP);
    const int maxWaves = d.wgReduce ? 4 * d.G : d.Vbase + (d.Vextra > 0 ? 1 : 0); /* Schur wavefronts of a window at most */
    d.oPartS = take(d.big ? 0 : 4096ull * (d.wgReduce ? d.G : maxWaves));
    d.oBigA = take(d.big ? (unsigned long long)(d.np + 1) * d.np + 32 : 0); /* + BA_PB: the last panel's row loads */
    d.wstride = o;
    unsigned long long io = 0;
    auto itake = [&](unsigned long long n) { unsigned long long r = io; io += (n + 3) & ~3ull; return r; };
    d.oPtStart = itake(npt + 1);
    d.oPtFree = itake(npt + 1);
    d.oKfStart = itake(nkf + 1);
    d.oKfEdges = itake(obs_pitch);
    d.oFreeKP = itake(4ull * obs_pitch);
    d.oKfRec = itake(4ull * obs_pitch);
    d.oPtRank = itake(npt);
    d.oPerm = itake(d.renum ? npt : 0);
    d.oPtMask = itake(d.big ? 0 : npt);
    d.oPermA = itake(d.big ? 0 : npt);
    d.oPermB = itake(d.big ? 0 : npt);
    d.oKPs = itake(d.big ? 0 : 4ull * obs_pitch);
    d.oGDesc = itake(d.big ? 0 : 4ull * npt + 4);
    d.oGCost = itake(d.big ? 0 : (unsigned long long)npt + 1);
    d.oGCut = itake(d.big ? 0 : (unsigned long long)maxWaves + 1);
    d.oPairStart = itake(d.big ? d.npairs + 1 : 0);
    d.oPairCnt = itake(d.big ? d.npairs : 0);
    d.oPairItems = itake(d.big ? 2 * d.maxItems : 0);
    d.istride = io;
}

/* ---- the host side. One call is planned once (BaPlan: shapes, workspace pointers, kernels, LDS sizes); the head and the
 * trials are queued from the plan, directly or through a captured graph. */
#define BA_RING 1000 /* still-running counters: one per trial (the host refuses calls that could run more) */

struct BaPlan {
    BaDims d;
    /* the caller's arrays */
    float *poses, *pts;
    const tb_ba_obs* obs_in;
    const int32_t* counts;
    void* work;
    /* the workspace, in this order: per-window doubles and ints, the LM states, one still-running counter per trial (no
     * memset node between the trials), one rejected-input flag per window (zeroed together with the counters before the
     * set-up kernel) and, for renumbered windows, the observations with the points in pattern order, laid out as the
     * caller's array */
    double* dw;
    int* iw;
    BaState* states;
    int *running, *errflag;
    tb_ba_obs* obs2;
    size_t work_bytes;
    const tb_ba_obs* obs; /* what the passes walk: obs2 for renumbered windows, else the caller's array */
    /* the template instances this shape runs, and the dynamic LDS of the kernels that size it by the window */
    decltype(&k_ba_schur_c<1>) schur;
    decltype(&k_ba_solve<16>) solve;
    decltype(&k_ba_lin<true>) lin;
    decltype(&k_ba_points<true>) points;
    decltype(&k_ba_update<true>) update;
    size_t prepare_lds, pass_lds, schur_lds, big_lds, update_lds;
};

static BaPlan ba_plan(const tb_ctx* ctx, int W, const double K[4], int nkf, int nfixed, int npt, int obs_pitch, int iters, float* d_poses,
                      float* d_pts, const tb_ba_obs* d_obs, const int32_t* d_counts, void* d_work) {
    BaPlan p;
    BaDims& d = p.d;
    ba_dims(d, ctx->num_cu, ctx->peers, W, K, nkf, nfixed, npt, obs_pitch, iters);
    if (ctx->dbg_ba_plain_obs) d.stream = 0; /* test hook: the array-of-structs walk for every window (part of the graph key) */
    p.poses = d_poses; p.pts = d_pts; p.obs_in = d_obs; p.counts = d_counts; p.work = d_work;
    /* The layout, said once: the regions follow each other from d_work, and the total is what they add up to. An aligned
     * region starts at the next multiple of its alignment in the caller's address space, so the total counts the whole
     * alignment for it. */
    uintptr_t at = (uintptr_t)d_work;
    size_t total = 0;
    auto take = [&](size_t bytes, size_t align) {
        at = (at + align - 1) / align * align;
        const uintptr_t r = at;
        at += bytes;
        total += bytes + (align > 1 ? align : 0);
        return r;
    };
    p.dw = (double*)take((size_t)W * d.wstride * sizeof(double), 1);
    p.iw = (int*)take((size_t)W * d.istride * sizeof(int), 1);
    p.states = (BaState*)take((size_t)W * sizeof(BaState), 1);
    p.running = (int*)take(BA_RING * sizeof(int), 1);
    p.errflag = (int*)take((size_t)W * sizeof(int), 1);
    p.obs2 = d.renum ? (tb_ba_obs*)take((size_t)W * obs_pitch * sizeof(tb_ba_obs), 64) : nullptr;
    p.work_bytes = total + 96; /* callers size their buffers by this value: the 96 spare bytes it has always had stay */
    p.obs = d.renum ? p.obs2 : d_obs;
    const int R = (d.np + 15) >> 4;
    p.schur = R == 1 ? k_ba_schur_c<1> : R == 2 ? k_ba_schur_c<2> : R == 3 ? k_ba_schur_c<3> : k_ba_schur_c<4>;
    p.solve = d.np <= 16 ? k_ba_solve<16> : d.np <= 32 ? k_ba_solve<32> : d.np <= 48 ? k_ba_solve<48> : k_ba_solve<64>;
    p.lin = d.stream ? k_ba_lin<true> : k_ba_lin<false>;
    p.points = d.stream ? k_ba_points<true> : k_ba_points<false>;
    p.update = d.stream ? k_ba_update<true> : k_ba_update<false>;
    p.prepare_lds = (size_t)npt * 16 + 16;
    p.pass_lds = (size_t)d.nkf * 12 * sizeof(double);
    /* Schur kernel: four wavefronts' tiles (small batches reuse them for the 64 x 64 sum of the wavefronts' systems) */
    p.schur_lds = std::max<size_t>(4 * (size_t)d.schurWaveLds, d.wgReduce ? 64 * 64 : 0) * sizeof(double);
    p.big_lds = (size_t)(d.np + 1) * BA_PLD * sizeof(double);
    p.update_lds = ((size_t)d.nkf * 24 + d.np) * sizeof(double);
    return p;
}

size_t tbk_local_ba_work_bytes(const tb_ctx* ctx, int W, int nkf, int nfixed, int npt, int obs_pitch) {
    const double K[4] = {1, 1, 0, 0};
    return ba_plan(ctx, W, K, nkf, nfixed, npt, obs_pitch, 1, nullptr, nullptr, nullptr, nullptr, nullptr).work_bytes;
}

/* once per call: LM state, CSR tables, pattern groups (block-pair lists for large windows) */
static int ba_enqueue_head(tb_ctx* ctx, const BaPlan& p) {
    const BaDims& d = p.d;
    const int W = d.W;
    /* a kernel, not hipMemsetAsync: as a memset NODE of a replayed graph the fill came back as stale pointer-sized
     * values on one of three contexts replaying from their own host threads (ROCm 7.2), the windows then read a set
     * rejected-input flag and returned their input */
    TB_TRY(tb_launch(ctx, nullptr, k_ba_zero, dim3((BA_RING + W + 255) / 256), dim3(256), 0, p.running, BA_RING + W));
    if (d.renum) TB_TRY(tb_launch(ctx, "k_ba_prepare", k_ba_prepare, dim3(W), dim3(BA_RT), p.prepare_lds, d, p.obs_in, p.counts, p.iw, p.obs2));
    TB_TRY(tb_launch(ctx, "k_ba_setup", k_ba_setup, dim3(d.nkf + 2, W), dim3(BA_T), 0, d, p.poses, p.pts, p.obs_in, p.obs, p.counts, p.dw, p.iw,
                     p.states, p.errflag));
    if (d.renum) {
        /* k_ba_prepare did it */
    } else if (!d.big) {
        TB_TRY(tb_launch(ctx, "k_ba_groups", k_ba_groups, dim3(W), dim3(BA_T), 0, d, p.iw, p.errflag));
    } else {
        /* block-pair item lists of the large-window Schur kernel: count, scan, fill -- one profile record over the three */
        tb_prof_begin(ctx, "k_ba_pairs");
        TB_TRY(tb_launch(ctx, nullptr, k_ba_pairs<false>, dim3(d.nfree, W), dim3(64), 0, d, p.obs, p.iw, p.errflag));
        TB_TRY(tb_launch(ctx, nullptr, k_ba_pair_scan, dim3(W), dim3(BA_T), 0, d, p.iw, p.errflag));
        TB_TRY(tb_launch(ctx, nullptr, k_ba_pairs<true>, dim3(d.nfree, W), dim3(64), 0, d, p.obs, p.iw, p.errflag));
        tb_prof_end(ctx);
    }
    return TB_OK;
}

/* one LM trial of every window: eight launches */
static int ba_enqueue_round(tb_ctx* ctx, const BaPlan& p, int round) {
    const BaDims& d = p.d;
    const int W = d.W;
    const int nKfBlocks = ((W + 7) / 8) * 8 * std::min(BA_KFBLK, d.kfChunks) * d.nfree;
    if (W <= 32 || BA_LIN_FUSE_ALL) {
        TB_TRY(tb_launch(ctx, "k_ba_lin", p.lin, dim3(nKfBlocks + d.nblkP * W), dim3(BA_T), p.pass_lds, d, p.obs, p.dw, p.iw, p.states, p.errflag,
                         nKfBlocks));
    } else {
        TB_TRY(tb_launch(ctx, "k_ba_points", p.points, dim3(d.nblkP, W), dim3(BA_T), p.pass_lds, d, p.obs, p.dw, p.iw, p.states, p.errflag));
        TB_TRY(tb_launch(ctx, "k_ba_kf", k_ba_kf, dim3(nKfBlocks), dim3(BA_T), 0, d, p.obs, p.dw, p.iw, p.states, p.errflag));
    }
    const bool reduce_in_solve = !d.big && round > 0;
    if (!reduce_in_solve) TB_TRY(tb_launch(ctx, "k_ba_reduce", k_ba_reduce, dim3(W), dim3(BA_T), 0, d, p.dw, p.iw, p.states));
    if (round == 0) /* the first trial's lambda comes out of k_ba_reduce; later ones are known to k_ba_points */
        TB_TRY(tb_launch(ctx, "k_ba_hinv", k_ba_hinv, dim3(d.nblkP, W), dim3(BA_T), 0, d, p.dw, p.iw, p.states));
    if (d.big) {
        TB_TRY(tb_launch(ctx, "k_ba_schur_pairs", k_ba_schur_pairs, dim3((d.npairs + 3) / 4, W), dim3(BA_T), 0, d, p.dw, p.iw, p.states));
        TB_TRY(tb_launch(ctx, "k_ba_solve_big", k_ba_solve_big, dim3(W), dim3(BA_ST), p.big_lds, d, p.dw, p.states));
    } else {
        TB_TRY(tb_launch(ctx, "k_ba_schur", p.schur, dim3(d.wgReduce ? d.Gbase * W + d.Gextra : (d.Vbase * W + d.Vextra + 3) / 4), dim3(BA_T),
                         p.schur_lds, d, p.dw, p.iw, p.states));
        TB_TRY(tb_launch(ctx, "k_ba_solve", p.solve, dim3(W), dim3(BA_SOLVE_T), 0, d, p.dw, p.iw, p.states, reduce_in_solve ? 1 : 0));
    }
    TB_TRY(tb_launch(ctx, "k_ba_update", p.update, dim3(d.nblkP, W), dim3(BA_T), p.update_lds, d, p.obs, p.dw, p.iw, p.states));
    return tb_launch(ctx, "k_ba_decide", k_ba_decide, dim3(W), dim3(64), 0, d, p.dw, p.states, p.running + round % BA_RING);
}

/* The head and the first nfirst trials as one graph, from the context's cache or captured now. The kernels read their state
 * from the workspace, so a graph per (shape, buffers, stream) is the same every time it is replayed. */
static int ba_graph(tb_ctx* ctx, const BaPlan& p, int nfirst, hipGraphExec_t* exec) {
    struct Key { BaDims d; const void *poses, *pts, *obs, *counts, *work; hipStream_t s; } key;
    memset(&key, 0, sizeof key);
    key.d = p.d; key.poses = p.poses; key.pts = p.pts; key.obs = p.obs_in; key.counts = p.counts; key.work = p.work; key.s = ctx->stream;
    const std::string kb((const char*)&key, sizeof key);
    for (auto& g : ctx->ba_graphs)
        if (g.first == kb) { *exec = g.second; return TB_OK; }
    /* one capture at a time in the process: the pipeline drives its BA partitions from one host thread each, and
     * three threads capturing on three streams at once produced graphs that did not replay the call (wrong poses,
     * no error) -- a capture is rare (once per shape and buffer set), so it simply takes a lock */
    static std::mutex capture_lock;
    std::lock_guard<std::mutex> guard(capture_lock);
    hipGraph_t graph = nullptr;
    TB_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    int rc = ba_enqueue_head(ctx, p);
    for (int r = 0; r < nfirst && rc == TB_OK; r++) rc = ba_enqueue_round(ctx, p, r);
    const hipError_t e = hipStreamEndCapture(ctx->stream, &graph); /* always ends the capture, also after a failed launch */
    if (rc != TB_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    TB_HIP(ctx, e);
    const hipError_t e2 = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    TB_HIP(ctx, e2);
    if (ctx->ba_graphs.size() >= 8) { /* a caller cycling through more buffer sets than this re-captures */
        hipGraphExecDestroy(ctx->ba_graphs.front().second);
        ctx->ba_graphs.erase(ctx->ba_graphs.begin());
    }
    ctx->ba_graphs.emplace_back(kb, *exec);
    return TB_OK;
}

int tbk_local_ba_batch(tb_ctx* ctx, int W, const double K[4], int nkf, int nfixed, float* d_poses, int npt, float* d_pts,
                       const tb_ba_obs* d_obs, const int32_t* d_counts, int obs_pitch, int iters, double* d_stats, void* d_work,
                       size_t work_bytes) {
    if (W <= 0) return TB_OK;
    const int nfree = nkf - nfixed;
    if (nfree < 1 || nfree > BA_BIG_MAXF)
        return tb_fail(ctx, TB_EUNSUPPORTED, "local BA: %d free keyframes (this build supports 1..64)", nfree);
    if (nkf > TB_MAX_LEVELS * 8) return tb_fail(ctx, TB_EUNSUPPORTED, "local BA: too many keyframes");
    if (npt > (1 << 25)) return tb_fail(ctx, TB_EUNSUPPORTED, "local BA: more than 2^25 points per window");
    if (nfree > BA_SMALL_MAXF && (unsigned long long)obs_pitch * (nfree + 1) >= (1ull << 31))
        return tb_fail(ctx, TB_EUNSUPPORTED, "local BA: large window with more than 2^31 / (free keyframes + 1) observations");
    if (iters > 99) return tb_fail(ctx, TB_EUNSUPPORTED, "local BA: more than 99 LM iterations (one still-running counter per trial, 1000 of them)");
    const BaPlan p = ba_plan(ctx, W, K, nkf, nfixed, npt, obs_pitch, iters, d_poses, d_pts, d_obs, d_counts, d_work);
    const BaDims& d = p.d;
    if (p.work_bytes > work_bytes) return tb_fail(ctx, TB_ENOMEM, "local BA workspace too small");
    hipStream_t s = ctx->stream;
    /* before any capture begins: the limits of the kernels whose dynamic LDS grows with the window (tb_lds_limit only raises) */
    if (!d.big) TB_TRY(tb_lds_limit(ctx, (const void*)p.schur, p.schur_lds));
    if (d.renum) TB_TRY(tb_lds_limit(ctx, (const void*)k_ba_prepare, p.prepare_lds));
    if (d.big) TB_TRY(tb_lds_limit(ctx, (const void*)k_ba_solve_big, p.big_lds));
    const int max_rounds = std::min(iters * 10 + 1, BA_RING);
    int batch = iters; /* what every window needs at least; a speculative extra round (rounds 1-3) was seven empty launches on
                          every call to save one host round trip on the calls with a rejected step */
    const int nfirst = std::min(batch, max_rounds);
    /* Small batches: the set-up and the first `iters` trials -- ~100 launches of a few microseconds each, which a host
     * thread cannot queue as fast as the GPU retires them -- are captured ONCE into a HIP graph per (shape, buffers) and
     * replayed with one call. Large batches launch directly: their kernels are long enough for the queue to stay ahead
     * (DESIGN.md section 4), and the per-kernel timing hooks need ordinary launches. */
    const bool use_graph = W <= 32 && !ctx->prof && nfirst > 0;
    int rounds = 0;
    if (use_graph) {
        hipGraphExec_t exec = nullptr;
        TB_TRY(ba_graph(ctx, p, nfirst, &exec));
        TB_HIP(ctx, hipGraphLaunch(exec, s));
        rounds = nfirst;
    } else {
        TB_TRY(ba_enqueue_head(ctx, p));
    }
    /* no trial asked for (iters == 0): nothing was queued behind the head, no counter was written and none is read -- the
     * write-back returns the input as the set-up stored it */
    int host_running = nfirst > 0 ? 1 : 0;
    bool replayed = use_graph; /* the first batch of trials is already queued */
    while (host_running > 0 && (rounds < max_rounds || replayed)) {
        if (!replayed)
            for (int r = 0; r < batch && rounds < max_rounds; r++, rounds++) TB_TRY(ba_enqueue_round(ctx, p, rounds));
        replayed = false;
        /* windows still running after the expected number of trials (rejected steps): one sync, then continue */
        TB_HIP(ctx, hipMemcpyAsync(&host_running, p.running + (rounds - 1) % BA_RING, sizeof(int), hipMemcpyDeviceToHost, s));
        TB_HIP(ctx, hipStreamSynchronize(s));
        batch = 4;
    }
    return tb_launch(ctx, "k_ba_finish", k_ba_finish, dim3(W), dim3(BA_T), 0, d, p.dw, p.iw, p.states, d_poses, d_pts, d_stats);
}
