/* ORB-SLAM's ORBmatcher::SearchBySim3, batched (tb_search_by_sim3_batch_dev, include/tb_capi.h has the rules; the definition is
 * tests/sim3_search_reference.py, statement for statement): every key of one side that carries a point is taken through the
 * similarity into the other side's image, a scale-dependent window there is searched by Hamming distance, and the pairs on which
 * both directions agree are listed.
 *
 * k_sim3_search: grid (chunks of 256 source keys, 2 directions, pairs), one lane a source key. The projection, the range test, the
 * predicted level and the radius are float64 from the float32 inputs, one rounding a statement (-ffp-contract=off). The search is
 * a tiled scan: the target side's (x, y, octave) pass through LDS in tiles of S3S_TILE keys, every lane walks the tile (all lanes
 * read the same LDS word: a broadcast, no bank conflict) and only a key inside the window costs a descriptor read. The best
 * candidate is the minimum of the packed (distance << 32 | index), so the visiting order decides nothing. A lane leaves a code in
 * match[i]: j >= 0 accepted, -1 searched and nothing accepted, -2 tried and skipped before the search, -3 not tried.
 * k_sim3_search_agree: one workgroup a pair. It checks the problem (octaves, s), counts the codes (integer sums through ballots and
 * LDS, no atomic), lists the mutual pairs in ascending i by ordered compaction, and only then turns every code below 0 into -1. */
#include "tb_internal.h"
#include "tb_device.h"

#pragma clang fp contract(off)

#define S3S_T 256
#define S3S_TILE 1024

struct S3sSide {
    const tb_keypoint* keys;   /* [frames][pitch] */
    const uint8_t* desc;       /* [frames][pitch][32] */
    const uint8_t* valid;      /* [frames][pitch] */
    const int32_t* counts;     /* [frames] */
    const int32_t* frame;      /* [pairs] the frame of pair p (nullptr: p) */
    const float* pts;          /* [pairs][pitch][3] */
    const uint8_t* matched;    /* [pairs][pitch] */
    int32_t* match;            /* [pairs][pitch] */
    int pitch;
};

struct S3sBatch {
    S3sSide side[2];
    const double* srt;         /* [pairs][8] */
    const int32_t* skip;       /* [pairs] nullable: non-zero = the pair is skipped (flag 2) */
    double fx, fy, cx, cy, width, height, th;
    float g[TB_MAX_LEVELS];    /* a level's pixel in level-0 pixels */
    int nlevels, th_high;
    tb_match* pairs; int cap; int32_t* pair_counts; int32_t* stats;
};

__device__ __forceinline__ bool s3s_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ double s3s_norm(double X, double Y, double Z) {
    double n = X * X;
    n = n + Y * Y;
    n = n + Z * Z;
    return sqrt(n);
}

/* R (row-major) of the quaternion w x y z as it is given: k_sim3.hip's s3_rotation, statement for statement */
__device__ __forceinline__ void s3s_rotation(const double* q, double (&R)[9]) {
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

__device__ __forceinline__ size_t s3s_frame(const S3sSide& S, int p) { return S.frame ? (size_t)max(S.frame[p], 0) : (size_t)p; }

__global__ void __launch_bounds__(S3S_T)
k_sim3_search(S3sBatch B) {
    __shared__ float tx[S3S_TILE], ty[S3S_TILE];
    __shared__ int to[S3S_TILE];
    __shared__ double g[TB_MAX_LEVELS];
    const int p = blockIdx.z, dir = blockIdx.y, tid = threadIdx.x;
    if (B.skip && B.skip[p]) return;
    const S3sSide& A = B.side[dir];
    const S3sSide& T = B.side[dir ^ 1];
    const size_t fa = s3s_frame(A, p), ft = s3s_frame(T, p);
    const int na = min(max(A.counts[fa], 0), A.pitch), nt = min(max(T.counts[ft], 0), T.pitch);
    if ((int)(blockIdx.x * S3S_T) >= na) return;
    if (tid < TB_MAX_LEVELS) g[tid] = (double)B.g[tid];
    __syncthreads();
    const int i = blockIdx.x * S3S_T + tid;
    const int nl = B.nlevels;
    int code = -3, L = 0;
    bool search = false;
    double u = 0.0, v = 0.0, r = 0.0;
    if (i < na && A.valid[fa * A.pitch + i] && !A.matched[(size_t)p * A.pitch + i]) {
        code = -2;
        const double* srt = B.srt + 8 * (size_t)p;
        const double s = srt[7], t0 = srt[4], t1 = srt[5], t2 = srt[6];
        double R[9];
        s3s_rotation(srt, R);
        const float* Xf = A.pts + 3 * ((size_t)p * A.pitch + i);
        const double X = (double)Xf[0], Y = (double)Xf[1], Z = (double)Xf[2];
        double P[3];
        if (dir == 0) {   /* P = R' (X1 - t) / s */
            const double d0 = X - t0, d1 = Y - t1, d2 = Z - t2;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double a = R[k] * d0;
                a = a + R[3 + k] * d1;
                a = a + R[6 + k] * d2;
                P[k] = a / s;
            }
        } else {          /* P = s (R X2) + t */
            const double t[3] = {t0, t1, t2};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double a = R[3 * k] * X;
                a = a + R[3 * k + 1] * Y;
                a = a + R[3 * k + 2] * Z;
                a = s * a;
                P[k] = a + t[k];
            }
        }
        if (P[2] > 0.0) {
            double a = P[0] / P[2];
            a = B.fx * a;
            u = a + B.cx;
            a = P[1] / P[2];
            a = B.fy * a;
            v = a + B.cy;
            if (u >= 0.0 && u < B.width && v >= 0.0 && v < B.height) {
                const int oct = min(max(A.keys[fa * A.pitch + i].octave, 0), nl - 1);   /* outside: the problem is flagged by the agreement pass */
                const double maxD = s3s_norm(X, Y, Z) * g[oct];
                const double minD = maxD / g[nl - 1];
                const double n = s3s_norm(P[0], P[1], P[2]);
                const double d = dir == 0 ? s * n : n / s;
                const double lo = 0.8 * minD, hi = 1.2 * maxD;
                if (d >= lo && d <= hi) {
                    L = nl - 1;
                    for (int l = nl - 2; l >= 0; l--)
                        if (g[l] * d >= maxD) L = l;
                    r = B.th * g[L];
                    search = true;
                    code = -1;
                }
            }
        }
    }
    unsigned long long best = ~0ull;
    unsigned long long da[4] = {0, 0, 0, 0};
    if (search) {
        const unsigned long long* a = reinterpret_cast<const unsigned long long*>(A.desc + 32 * (fa * A.pitch + i));
        da[0] = a[0]; da[1] = a[1]; da[2] = a[2]; da[3] = a[3];
    }
    const tb_keypoint* TK = T.keys + ft * T.pitch;
    const unsigned long long* TD = reinterpret_cast<const unsigned long long*>(T.desc + 32 * ft * T.pitch);
    for (int j0 = 0; j0 < nt; j0 += S3S_TILE) {
        const int m = min(S3S_TILE, nt - j0);
        __syncthreads();
        for (int j = tid; j < m; j += S3S_T) {
            const tb_keypoint k = TK[j0 + j];
            tx[j] = k.x; ty[j] = k.y; to[j] = k.octave;
        }
        __syncthreads();
        if (search)
            for (int j = 0; j < m; j++) {
                const int o = to[j];
                if (o != L && o != L - 1) continue;
                if (!(fabs((double)tx[j] - u) < r)) continue;
                if (!(fabs((double)ty[j] - v) < r)) continue;
                const unsigned long long* q = TD + 4 * (size_t)(j0 + j);
                const int dist = __popcll(da[0] ^ q[0]) + __popcll(da[1] ^ q[1]) + __popcll(da[2] ^ q[2]) + __popcll(da[3] ^ q[3]);
                const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)(j0 + j);
                best = key < best ? key : best;
            }
    }
    if (i < na) {
        if (search && best != ~0ull && (int)(best >> 32) <= B.th_high) code = (int)(best & 0xffffffffu);
        A.match[(size_t)p * A.pitch + i] = code;
    }
}

/* the sum of v over the 256 threads, in every thread; red: int[4] in LDS. Two barriers. */
__device__ __forceinline__ int s3s_block_sum(int v, int* red) {
    const int w = tb_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    const int s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(S3S_T)
k_sim3_search_agree(S3sBatch B) {
    __shared__ int red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const S3sSide& S1 = B.side[0];
    const S3sSide& S2 = B.side[1];
    int32_t* m1 = S1.match + (size_t)p * S1.pitch;
    int32_t* m2 = S2.match + (size_t)p * S2.pitch;
    tb_match* out = B.pairs ? B.pairs + (size_t)p * B.cap : nullptr;
    const bool skipped = B.skip && B.skip[p];
    int bad = 0, n1 = 0, n2 = 0;
    size_t f1 = 0, f2 = 0;
    if (!skipped) {
        f1 = s3s_frame(S1, p); f2 = s3s_frame(S2, p);
        n1 = min(max(S1.counts[f1], 0), S1.pitch); n2 = min(max(S2.counts[f2], 0), S2.pitch);
        const double s = B.srt[8 * (size_t)p + 7];
        bad = !(s > 0.0) || !s3s_finite(s);
        for (int i = tid; i < n1; i += S3S_T) { const int o = S1.keys[f1 * S1.pitch + i].octave; bad |= (o < 0 || o >= B.nlevels); }
        for (int j = tid; j < n2; j += S3S_T) { const int o = S2.keys[f2 * S2.pitch + j].octave; bad |= (o < 0 || o >= B.nlevels); }
    }
    bad = __syncthreads_or(bad);
    if (skipped || bad) {
        for (int i = tid; i < S1.pitch; i += S3S_T) m1[i] = -1;
        for (int j = tid; j < S2.pitch; j += S3S_T) m2[j] = -1;
        if (tid == 0) {
            if (B.pair_counts) B.pair_counts[p] = 0;
            if (B.stats) { for (int k = 0; k < 7; k++) B.stats[8 * (size_t)p + k] = 0; B.stats[8 * (size_t)p + 7] = skipped ? 2 : 1; }
        }
        return;
    }
    /* the codes: tried >= -2, searched >= -1, accepted >= 0 */
    int c[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n1; i += S3S_T) { const int m = m1[i]; c[0] += m >= -2; c[1] += m >= -1; c[4] += m >= 0; }
    for (int j = tid; j < n2; j += S3S_T) { const int m = m2[j]; c[2] += m >= -2; c[3] += m >= -1; c[5] += m >= 0; }
    int tot[6];
#pragma unroll
    for (int k = 0; k < 6; k++) tot[k] = s3s_block_sum(c[k], red);
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += S3S_T) {
        const int i = i0 + tid;
        int j = -1;
        if (i < n1) j = m1[i];
        const bool ok = j >= 0 && j < n2 && m2[j] == i;
        const int at = tb_block_ordered_slot(ok, base, red);
        if (ok && out && at < B.cap) {
            const unsigned long long* a = reinterpret_cast<const unsigned long long*>(S1.desc + 32 * (f1 * S1.pitch + i));
            const unsigned long long* b = reinterpret_cast<const unsigned long long*>(S2.desc + 32 * (f2 * S2.pitch + j));
            tb_match m;
            m.queryIdx = i; m.trainIdx = j; m.imgIdx = -1;
            m.distance = (float)(__popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]));
            out[at] = m;
        }
    }
    __syncthreads();   /* every read of a code is done: now the codes below 0 become -1, and so does what lies beyond the counts */
    for (int i = tid; i < S1.pitch; i += S3S_T) if (i >= n1 || m1[i] < 0) m1[i] = -1;
    for (int j = tid; j < S2.pitch; j += S3S_T) if (j >= n2 || m2[j] < 0) m2[j] = -1;
    if (tid == 0) {
        if (B.pair_counts) B.pair_counts[p] = base;
        if (B.stats) {
            int32_t* st = B.stats + 8 * (size_t)p;
            for (int k = 0; k < 6; k++) st[k] = tot[k];
            st[6] = base; st[7] = 0;
        }
    }
}

int tbk_sim3_search_batch(tb_ctx* ctx, int npairs, const double K[4], int width, int height, int nlevels, const float* level_px,
                          const tbk_sim3_search_side* s1, const tbk_sim3_search_side* s2, const double* d_srt, const int32_t* d_skip,
                          float th, int th_high, int32_t* d_match1, int32_t* d_match2, tb_match* d_pairs, int cap, int32_t* d_pair_counts,
                          int32_t* d_stats) {
    if (npairs <= 0) return TB_OK;
    S3sBatch B;
    const tbk_sim3_search_side* in[2] = {s1, s2};
    int32_t* match[2] = {d_match1, d_match2};
    for (int k = 0; k < 2; k++) {
        S3sSide& S = B.side[k];
        S.keys = in[k]->keys; S.desc = in[k]->desc; S.valid = in[k]->valid; S.counts = in[k]->counts; S.frame = in[k]->frame;
        S.pts = in[k]->points; S.matched = in[k]->matched; S.match = match[k]; S.pitch = in[k]->pitch;
    }
    B.srt = d_srt; B.skip = d_skip;
    B.fx = K[0]; B.fy = K[1]; B.cx = K[2]; B.cy = K[3]; B.width = (double)width; B.height = (double)height; B.th = (double)th;
    for (int l = 0; l < TB_MAX_LEVELS; l++) B.g[l] = l < nlevels ? level_px[l] : 0.f;
    B.nlevels = nlevels; B.th_high = th_high;
    B.pairs = d_pairs; B.cap = cap; B.pair_counts = d_pair_counts; B.stats = d_stats;
    const int chunks = (std::max(s1->pitch, s2->pitch) + S3S_T - 1) / S3S_T;
    TB_TRY(tb_launch(ctx, "k_sim3_search", k_sim3_search, dim3(chunks, 2, npairs), dim3(S3S_T), 0, B));
    return tb_launch(ctx, "k_sim3_search_agree", k_sim3_search_agree, dim3(npairs), dim3(S3S_T), 0, B);
}
