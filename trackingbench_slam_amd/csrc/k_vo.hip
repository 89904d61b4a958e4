/* Device-resident stereo VO loop (test/test_vo.cpp test_kitti, :674-850): the glue between the batched operators.
 *
 * One workgroup of 256 per sequence; ordered compaction with __ballot prefix counts (as k_stereo_obs, k_match.hip).
 * float32 arithmetic, one operation per statement (the library builds with -ffp-contract=off), left to right; the CPU
 * composition in tests/vo_reference.py does the same operations in the same order. */
#include "tb_internal.h"

/* Byte copy of nimg images into a tight [nimg][h][w] layout (the loop keeps the last left image for the next LK step). */
__global__ void __launch_bounds__(256)
k_vo_copy_image(const uint8_t* __restrict__ src, int w, int h, int stride, size_t pitch, uint8_t* __restrict__ dst) {
    const int s = blockIdx.y;
    const size_t npx = (size_t)w * h;
    const uint8_t* S = src + (size_t)s * pitch;
    uint8_t* D = dst + (size_t)s * npx;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
        D[i] = S[(size_t)y * stride + x];
    }
}

/* Frame t > 0, after searchByOPFlow(cur, last, pts, true, true) (test_vo.cpp:716) wrote the tracked points into the new key
 * list (`keys`, all n of them, lost ones included, :717-724):
 *   - key i carries the last frame's map point i when status[i] is set (:731-737);
 *   - PoseOptimization's rows: one per key that has a map point, in key order: px = the tracked point, Xw = the map point,
 *     invSigma2[octave 0] = 1 (LocalBA.cpp:333-363; the keys are default-constructed cv::KeyPoints);
 *   - outlier flags start false (a fresh Frame). */
__global__ void __launch_bounds__(256)
k_vo_track(const int32_t* __restrict__ prev_counts, const uint8_t* __restrict__ status, const float* __restrict__ keys,
           const float* __restrict__ prev_mp, const uint8_t* __restrict__ prev_valid, int pitch, int32_t* __restrict__ key_counts,
           float* __restrict__ mp, uint8_t* __restrict__ valid, tb_obs* __restrict__ obs, int32_t* __restrict__ obs_counts,
           uint8_t* __restrict__ outlier) {
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(prev_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    tb_obs* O = obs + o;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        tb_obs r = {0, 0, 0, 0, 0, 0};
        if (i < n) {
            ok = status[o + i] && prev_valid[o + i];
            float X = 0.f, Y = 0.f, Z = 0.f;
            if (ok) { X = prev_mp[3 * (o + i)]; Y = prev_mp[3 * (o + i) + 1]; Z = prev_mp[3 * (o + i) + 2]; }
            mp[3 * (o + i)] = X; mp[3 * (o + i) + 1] = Y; mp[3 * (o + i) + 2] = Z;
            valid[o + i] = ok ? 1 : 0;
            outlier[o + i] = 0;
            r.u = keys[2 * (o + i)]; r.v = keys[2 * (o + i) + 1];
            r.X = X; r.Y = Y; r.Z = Z;
            r.inv_sigma2 = 1.0f;
        }
        const unsigned long long bm = __ballot(ok);
        if (lane == 0) wsum[wave] = __popcll(bm);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; w++) off += wsum[w];
        const int at = off + __popcll(bm & ((1ull << lane) - 1));
        if (ok) O[at] = r; /* at < n <= pitch */
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) { key_counts[s] = n; obs_counts[s] = base; }
}

/* Descriptor trackers, frame t (test_vo.cpp:712-713 and test_vo_1 :193-227): the current frame's keys are its ORB records
 * (all m of them) and the matcher has matched them (query) against the keyframe's (train):
 *   - a fresh frame: no map point on any key, outlier flags false;
 *   - for every match whose keyframe entry trainIdx has a map point, key queryIdx gets that point (Frame::AddMapPoint
 *     overwrites, so a later match in list order wins -- win[] keeps the last such match per key; both matchers emit each
 *     queryIdx at most once, so this only decides malformed lists);
 *   - PoseOptimization's rows: one per key that has a map point, IN KEY ORDER (LocalBA.cpp:333-363 walks i = 0..N):
 *     px = the key, Xw = the map point, invSigma2 = invLevelSigma2[octave] (LocalBA.cpp:349);
 *   - keys_xy / key_counts = the records' (x, y) and m (what the stereo operator and tb_vo_state_dev read).
 * win [nseq][pitch] is work memory: it is written and read with atomics only (L2), so the three phases need no other fence. */
struct tb_vo_sigma {
    float v[TB_MAX_LEVELS];
    int n;
};

__global__ void __launch_bounds__(256)
k_vo_match_carry(const tb_keypoint* __restrict__ orb, const int32_t* __restrict__ orb_counts, const tb_match* __restrict__ matches,
                 const int32_t* __restrict__ match_counts, const float* __restrict__ kf_mp, const uint8_t* __restrict__ kf_valid,
                 const int32_t* __restrict__ kf_counts, int pitch, tb_vo_sigma sig, int32_t* __restrict__ win, float* __restrict__ keys,
                 int32_t* __restrict__ key_counts, float* __restrict__ mp, uint8_t* __restrict__ valid, tb_obs* __restrict__ obs,
                 int32_t* __restrict__ obs_counts, uint8_t* __restrict__ outlier) {
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(orb_counts[s], 0), pitch);
    const int nm = min(max(match_counts[s], 0), pitch);
    const int nk = min(max(kf_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    const tb_keypoint* K = orb + o;
    const tb_match* M = matches + o;
    int32_t* Wn = win + o;
    for (int i = tid; i < n; i += 256) atomicExch(&Wn[i], -1);
    __syncthreads();
    for (int k = tid; k < nm; k += 256) {
        const int q = M[k].queryIdx, tr = M[k].trainIdx;
        if (q >= 0 && q < n && tr >= 0 && tr < nk && kf_valid[o + tr]) atomicMax(&Wn[q], k);
    }
    __syncthreads();
    tb_obs* O = obs + o;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        tb_obs r = {0, 0, 0, 0, 0, 0};
        if (i < n) {
            const int k = atomicAdd(&Wn[i], 0);
            ok = k >= 0;
            float X = 0.f, Y = 0.f, Z = 0.f;
            if (ok) {
                const size_t j = o + M[k].trainIdx;
                X = kf_mp[3 * j]; Y = kf_mp[3 * j + 1]; Z = kf_mp[3 * j + 2];
            }
            mp[3 * (o + i)] = X; mp[3 * (o + i) + 1] = Y; mp[3 * (o + i) + 2] = Z;
            valid[o + i] = ok ? 1 : 0;
            outlier[o + i] = 0;
            const tb_keypoint kp = K[i];
            keys[2 * (o + i)] = kp.x; keys[2 * (o + i) + 1] = kp.y;
            r.u = kp.x; r.v = kp.y;
            r.X = X; r.Y = Y; r.Z = Z;
            r.inv_sigma2 = sig.v[min(max(kp.octave, 0), sig.n - 1)];   /* the extractor's octaves are in [0, nlevels) */
        }
        const unsigned long long bm = __ballot(ok);
        if (lane == 0) wsum[wave] = __popcll(bm);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; w++) off += wsum[w];
        const int at = off + __popcll(bm & ((1ull << lane) - 1));
        if (ok) O[at] = r; /* at < n <= pitch */
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) { key_counts[s] = n; obs_counts[s] = base; }
}

/* Keyframe, first half: SetKeys(orb_keys) (test_vo.cpp:785). The ORB records become (x, y) pairs (what the stereo op reads)
 * and the map-point list is resized to m: mvpMapPoints.resize(m, nullptr) (Frame.cpp:114) KEEPS entries [0, min(n, m)) --
 * the map points step 2 attached to the previous key list at those indices -- and entries [n, m) are null. n = the key
 * count before the call (0 at frame 0: nothing was tracked). */
__global__ void __launch_bounds__(256)
k_vo_kf_pack(const tb_keypoint* __restrict__ orb, const int32_t* __restrict__ orb_counts, int orb_pitch, int pitch,
             float* __restrict__ keys, int32_t* __restrict__ key_counts, uint8_t* __restrict__ valid) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(orb_counts[s], 0), pitch);
    const int n = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    const tb_keypoint* K = orb + (size_t)s * orb_pitch;
    for (int j = tid; j < m; j += 256) {
        keys[2 * (o + j)] = K[j].x;
        keys[2 * (o + j) + 1] = K[j].y;
        if (j >= n) valid[o + j] = 0;
    }
    __syncthreads(); /* every lane has read key_counts[s] */
    if (tid == 0) key_counts[s] = m;
}

/* Keyframe, second half (test_vo.cpp:802-832): for every key j with depth[j] > 0 a new map point replaces entry j:
 * u = (int)x, v = (int)y, norm = ((u - cx) / fx, (v - cy) / fy, 1) in double (fx, cx are double, :633) stored as float,
 * Xw = R * norm * depth + t with R, t = the rotation / translation of Twc (Frame::SetPose, Frame.cpp:51-61) at the optimised
 * pose: Rwc = Rcw^T, twc = -(Rcw^T tcw). A depth that is not finite (zero disparity) creates no point (documented deviation:
 * the reference would create one at infinity). */
__global__ void __launch_bounds__(256)
k_vo_kf_spawn(const float* __restrict__ keys, const int32_t* __restrict__ key_counts, const float* __restrict__ depth,
              const float* __restrict__ Tcw, double fx, double fy, double cx, double cy, int pitch, float* __restrict__ mp,
              uint8_t* __restrict__ valid) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    const float* T = Tcw + 16 * s;
    float R[9], t[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i * 3 + j] = T[j * 4 + i];
    for (int i = 0; i < 3; i++) {
        float a = R[i * 3 + 0] * T[3];
        const float b = R[i * 3 + 1] * T[7];
        a = a + b;
        const float c = R[i * 3 + 2] * T[11];
        a = a + c;
        t[i] = -a;
    }
    for (int j = tid; j < m; j += 256) {
        const float d = depth[o + j];
        if (!(d > 0.f) || !isfinite(d)) continue;
        const int u = (int)keys[2 * (o + j)], v = (int)keys[2 * (o + j) + 1];
        const float n0 = (float)(((double)u - cx) / fx), n1 = (float)(((double)v - cy) / fy), n2 = 1.0f;
        for (int i = 0; i < 3; i++) {
            float a = R[i * 3 + 0] * n0;
            const float b = R[i * 3 + 1] * n1;
            a = a + b;
            const float c = R[i * 3 + 2] * n2;
            a = a + c;
            a = a * d;
            a = a + t[i];
            mp[3 * (o + j) + i] = a;
        }
        valid[o + j] = 1;
    }
}

int tbk_vo_copy_image(tb_ctx* ctx, int nimg, const uint8_t* d_src, int w, int h, int stride, size_t pitch, uint8_t* d_dst) {
    if (nimg <= 0) return TB_OK;
    const int bx = (int)std::min<size_t>(((size_t)w * h + 255) / 256, 512);
    tb_prof_begin(ctx, "k_vo_copy_image");
    hipLaunchKernelGGL(k_vo_copy_image, dim3(bx, nimg), dim3(256), 0, ctx->stream, d_src, w, h, stride, pitch, d_dst);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
}

int tbk_vo_track(tb_ctx* ctx, int nseq, const int32_t* d_prev_counts, const uint8_t* d_status, const float* d_keys, const float* d_prev_mp,
                 const uint8_t* d_prev_valid, int pitch, int32_t* d_key_counts, float* d_mp, uint8_t* d_valid, tb_obs* d_obs,
                 int32_t* d_obs_counts, uint8_t* d_outlier) {
    if (nseq <= 0) return TB_OK;
    tb_prof_begin(ctx, "k_vo_track");
    hipLaunchKernelGGL(k_vo_track, dim3(nseq), dim3(256), 0, ctx->stream, d_prev_counts, d_status, d_keys, d_prev_mp, d_prev_valid, pitch,
                       d_key_counts, d_mp, d_valid, d_obs, d_obs_counts, d_outlier);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
}

int tbk_vo_kf_pack(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, int orb_pitch, int pitch, float* d_keys,
                   int32_t* d_key_counts, uint8_t* d_valid) {
    if (nseq <= 0) return TB_OK;
    tb_prof_begin(ctx, "k_vo_kf_pack");
    hipLaunchKernelGGL(k_vo_kf_pack, dim3(nseq), dim3(256), 0, ctx->stream, d_orb, d_orb_counts, orb_pitch, pitch, d_keys, d_key_counts,
                       d_valid);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
}

int tbk_vo_kf_spawn(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const float* d_depth, const float* d_Tcw,
                    const double K[4], int pitch, float* d_mp, uint8_t* d_valid) {
    if (nseq <= 0) return TB_OK;
    tb_prof_begin(ctx, "k_vo_kf_spawn");
    hipLaunchKernelGGL(k_vo_kf_spawn, dim3(nseq), dim3(256), 0, ctx->stream, d_keys, d_key_counts, d_depth, d_Tcw, K[0], K[1], K[2], K[3],
                       pitch, d_mp, d_valid);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
}

int tbk_vo_match_carry(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, const tb_match* d_matches,
                       const int32_t* d_match_counts, const float* d_kf_mp, const uint8_t* d_kf_valid, const int32_t* d_kf_counts, int pitch,
                       const float* inv_sigma2, int nlevels, int32_t* d_win, float* d_keys, int32_t* d_key_counts, float* d_mp,
                       uint8_t* d_valid, tb_obs* d_obs, int32_t* d_obs_counts, uint8_t* d_outlier) {
    if (nseq <= 0) return TB_OK;
    if (nlevels < 1 || nlevels > TB_MAX_LEVELS) return TB_EINVAL;
    tb_vo_sigma sig = {};
    for (int l = 0; l < nlevels; l++) sig.v[l] = inv_sigma2[l];
    sig.n = nlevels;
    tb_prof_begin(ctx, "k_vo_match_carry");
    hipLaunchKernelGGL(k_vo_match_carry, dim3(nseq), dim3(256), 0, ctx->stream, d_orb, d_orb_counts, d_matches, d_match_counts, d_kf_mp,
                       d_kf_valid, d_kf_counts, pitch, sig, d_win, d_keys, d_key_counts, d_mp, d_valid, d_obs, d_obs_counts, d_outlier);
    tb_prof_end(ctx);
    TB_HIP(ctx, hipGetLastError());
    return TB_OK;
}
