/* Device-resident stereo VO loop (test/test_vo.cpp test_kitti, :674-850): the glue between the batched operators.
 *
 * One workgroup of 256 per sequence; ordered compaction with tb_block_ordered_slot (tb_device.h).
 * float32 arithmetic, one operation per statement (the library builds with -ffp-contract=off), left to right; the CPU
 * composition in tests/vo_reference.py does the same operations in the same order. */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_kfcopy.h"

/* Byte copy of nimg images into a tight [nimg][h][w] layout (the loop keeps the last left image for the next LK step). With an
 * index list (a ragged step's keyframe block) image j of the output is image idx[j] of the source: a gather. */
__global__ void __launch_bounds__(256)
k_vo_copy_image(const uint8_t* __restrict__ src, int w, int h, int stride, size_t pitch, const int32_t* __restrict__ idx,
                uint8_t* __restrict__ dst) {
    const int s = blockIdx.y;
    const size_t npx = (size_t)w * h;
    const uint8_t* S = src + (size_t)(idx ? idx[s] : s) * pitch;
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
    const int s = blockIdx.x, tid = threadIdx.x;
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
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) O[at] = r; /* at < n <= pitch */
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
    const int s = blockIdx.x, tid = threadIdx.x;
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
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) O[at] = r; /* at < n <= pitch */
    }
    if (tid == 0) { key_counts[s] = n; obs_counts[s] = base; }
}

/* Keyframe, first half: SetKeys(orb_keys) (test_vo.cpp:785). The ORB records become (x, y) pairs (what the stereo op reads)
 * and the map-point list is resized to m: mvpMapPoints.resize(m, nullptr) (Frame.cpp:114) KEEPS entries [0, min(n, m)) --
 * the map points step 2 attached to the previous key list at those indices -- and entries [n, m) are null. n = the key
 * count before the call (0 at frame 0: nothing was tracked). */
__global__ void __launch_bounds__(256)
k_vo_kf_pack(const tb_keypoint* __restrict__ orb, const int32_t* __restrict__ orb_counts, int orb_pitch, int pitch,
             float* __restrict__ keys, int32_t* __restrict__ key_counts, uint8_t* __restrict__ valid, const int32_t* __restrict__ idx) {
    const int r = blockIdx.x, s = idx ? idx[r] : r, tid = threadIdx.x;   /* row r of the extractor's batch is sequence s */
    const int m = min(max(orb_counts[r], 0), pitch);
    const int n = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    const tb_keypoint* K = orb + (size_t)r * orb_pitch;
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
              uint8_t* __restrict__ valid, const int32_t* __restrict__ idx) {
    const int r = blockIdx.x, s = idx ? idx[r] : r, tid = threadIdx.x;   /* depth row r belongs to sequence s */
    const int m = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch, od = (size_t)r * pitch;
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
        const float d = depth[od + j];
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

/* Projection trackers (test/test_projection.cpp test_projection, :512-517 with the commented lines enabled): the carry after
 * searchByProjection. As k_vo_match_carry -- a fresh frame, the last match in list order wins a key (the projection matchers
 * emit one match per map point, so several may name the same key: win[] decides by atomicMax over match indices), rows in key
 * order, invSigma2 by octave -- with two differences:
 *   - a map point's descriptor is the row of the frame that created it (MapPoint.cpp:35-36), so the 32 bytes travel with xyz;
 *   - MAP = false: trainIdx names a keyframe entry (src_mp / src_valid / src_desc at stride `pitch`, key aligned);
 *     MAP = true: trainIdx names a live map record (map_ptr->GetAllMapPoints().at(trainIdx), :527; records at stride
 *     src_pitch) and the match list is src_pitch long, one match per map point at most.
 * Keys without a map point get a zero descriptor. */
template <bool MAP>
__global__ void __launch_bounds__(256)
k_vo_proj_carry(const tb_keypoint* __restrict__ orb, const int32_t* __restrict__ orb_counts, const tb_match* __restrict__ matches,
                const int32_t* __restrict__ match_counts, int match_pitch, const float* __restrict__ src_mp,
                const uint8_t* __restrict__ src_valid, const tb_mappoint* __restrict__ src_rec, const uint8_t* __restrict__ src_desc,
                const int32_t* __restrict__ src_counts, int src_pitch, int pitch, tb_vo_sigma sig, int32_t* __restrict__ win,
                float* __restrict__ keys, int32_t* __restrict__ key_counts, float* __restrict__ mp, uint8_t* __restrict__ valid,
                uint8_t* __restrict__ mp_desc, tb_obs* __restrict__ obs, int32_t* __restrict__ obs_counts, uint8_t* __restrict__ outlier) {
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(orb_counts[s], 0), pitch);
    const int nm = min(max(match_counts[s], 0), match_pitch);   /* the matcher's count is not truncated, its list is */
    const int ns = min(max(src_counts[s], 0), src_pitch);
    const size_t o = (size_t)s * pitch, os = (size_t)s * src_pitch;
    const tb_keypoint* K = orb + o;
    const tb_match* M = matches + (size_t)s * match_pitch;
    int32_t* Wn = win + o;
    for (int i = tid; i < n; i += 256) atomicExch(&Wn[i], -1);
    __syncthreads();
    for (int k = tid; k < nm; k += 256) {
        const int q = M[k].queryIdx, tr = M[k].trainIdx;
        if (q >= 0 && q < n && tr >= 0 && tr < ns && (MAP || src_valid[os + tr])) atomicMax(&Wn[q], k);
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
            unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
            if (ok) {
                const size_t j = os + M[k].trainIdx;
                if (MAP) { X = src_rec[j].pos[0]; Y = src_rec[j].pos[1]; Z = src_rec[j].pos[2]; }
                else { X = src_mp[3 * j]; Y = src_mp[3 * j + 1]; Z = src_mp[3 * j + 2]; }
                const unsigned long long* D = reinterpret_cast<const unsigned long long*>(src_desc) + 4 * j;
                d0 = D[0]; d1 = D[1]; d2 = D[2]; d3 = D[3];
            }
            mp[3 * (o + i)] = X; mp[3 * (o + i) + 1] = Y; mp[3 * (o + i) + 2] = Z;
            unsigned long long* E = reinterpret_cast<unsigned long long*>(mp_desc) + 4 * (o + i);
            E[0] = d0; E[1] = d1; E[2] = d2; E[3] = d3;
            valid[o + i] = ok ? 1 : 0;
            outlier[o + i] = 0;
            const tb_keypoint kp = K[i];
            keys[2 * (o + i)] = kp.x; keys[2 * (o + i) + 1] = kp.y;
            r.u = kp.x; r.v = kp.y;
            r.X = X; r.Y = Y; r.Z = Z;
            r.inv_sigma2 = sig.v[min(max(kp.octave, 0), sig.n - 1)];
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) O[at] = r; /* at < n <= pitch */
    }
    if (tid == 0) { key_counts[s] = n; obs_counts[s] = base; }
}

/* Keyframe of a projection tracker, after k_vo_kf_spawn (test_projection.cpp:631-634): every key j that spawned a point
 * (the spawn's own test on depth[j]) gives the point its descriptor row; rec[j] (nullable) becomes the key-aligned tb_mappoint
 * searchByProjection(F1, F2) reads of the keyframe -- pos and bad = "no map point"; it reads nothing else of it. With a map
 * (map_rec != NULL) the spawned points are appended to the sequence's map tail in key order (ballot / prefix compaction as
 * k_vo_track): pos, normal = (pos - Ow) / |pos - Ow| (MapPoint.cpp:22-24; Ow = twc as the spawn computes it; float32, one
 * operation per statement, left to right), min_dist 1 and max_dist 1000 (the constants GetMin/MaxDistanceInvariance return,
 * MapPoint.cpp:207-217), bad 0, and the descriptor. map_n[s] grows by the block's size, which goes to map_blocks[s][slot].
 * A keyframe adds at most `pitch` points and the map holds nblk * pitch, so the tail never overflows; the store is guarded
 * all the same. */
__global__ void __launch_bounds__(256)
k_vo_kf_append(const int32_t* __restrict__ key_counts, const float* __restrict__ depth, const float* __restrict__ mp,
               const uint8_t* __restrict__ valid, const uint8_t* __restrict__ orb_desc, const float* __restrict__ Tcw, int pitch,
               uint8_t* __restrict__ mp_desc, tb_mappoint* __restrict__ rec, tb_mappoint* __restrict__ map_rec,
               uint8_t* __restrict__ map_desc, int32_t* __restrict__ map_n, int32_t* __restrict__ map_blocks, int nblk, int slot,
               int map_pitch, const int32_t* __restrict__ idx) {
    __shared__ int wsum[4];
    const int rw = blockIdx.x, s = idx ? idx[rw] : rw, tid = threadIdx.x;   /* depth row rw */
    const int m = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch, om = (size_t)s * map_pitch, od = (size_t)rw * pitch;
    const float* T = Tcw + 16 * s;
    float t[3];
    for (int i = 0; i < 3; i++) {
        float a = T[i] * T[3];
        const float b = T[4 + i] * T[7];
        a = a + b;
        const float c = T[8 + i] * T[11];
        a = a + c;
        t[i] = -a;
    }
    const int n0 = map_rec ? min(max(map_n[s], 0), map_pitch) : 0;
    int base = 0;
    for (int j0 = 0; j0 < m; j0 += 256) {
        const int j = j0 + tid;
        bool ok = false;
        tb_mappoint r = {{0, 0, 0}, {0, 0, 0}, 0, 0, 1};
        unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
        if (j < m) {
            const float d = depth[od + j];
            ok = d > 0.f && isfinite(d);
            if (ok) {
                const unsigned long long* D = reinterpret_cast<const unsigned long long*>(orb_desc) + 4 * (o + j);
                d0 = D[0]; d1 = D[1]; d2 = D[2]; d3 = D[3];
                unsigned long long* E = reinterpret_cast<unsigned long long*>(mp_desc) + 4 * (o + j);
                E[0] = d0; E[1] = d1; E[2] = d2; E[3] = d3;
            }
            if (valid[o + j]) {
                r.pos[0] = mp[3 * (o + j)]; r.pos[1] = mp[3 * (o + j) + 1]; r.pos[2] = mp[3 * (o + j) + 2];
                r.bad = 0;
            }
            if (rec) rec[o + j] = r;
        }
        if (!map_rec) continue;   /* uniform over the workgroup */
        const int at = n0 + tb_block_ordered_slot(ok, base, wsum);
        if (ok && at < map_pitch) {
            const float e0 = r.pos[0] - t[0], e1 = r.pos[1] - t[1], e2 = r.pos[2] - t[2];
            float q = e0 * e0;
            const float q1 = e1 * e1;
            q = q + q1;
            const float q2 = e2 * e2;
            q = q + q2;
            const float len = sqrtf(q);
            r.normal[0] = e0 / len; r.normal[1] = e1 / len; r.normal[2] = e2 / len;
            r.min_dist = 1.0f; r.max_dist = 1000.0f;
            map_rec[om + at] = r;
            unsigned long long* E = reinterpret_cast<unsigned long long*>(map_desc) + 4 * (om + at);
            E[0] = d0; E[1] = d1; E[2] = d2; E[3] = d3;
        }
    }
    if (map_rec && tid == 0) {
        map_n[s] = min(n0 + base, map_pitch);
        map_blocks[(size_t)s * nblk + slot] = min(n0 + base, map_pitch) - n0;
    }
}

/* The map holds the points of the last nblk keyframes. When one more arrives the oldest keyframe's points leave as a block and
 * the rest move down: records [blocks[0], n) of the source buffers become [0, n - blocks[0]) of the destination buffers (a
 * second set -- nothing is moved in place), the block counts move down one slot and the last slot is emptied for the append.
 * Records (9 words) and descriptors (8 words) are copied as 32-bit words; grid (tiles, nseq). */
__global__ void __launch_bounds__(256)
k_vo_map_evict(const tb_mappoint* __restrict__ src_rec, const uint8_t* __restrict__ src_desc, const int32_t* __restrict__ src_n,
               const int32_t* __restrict__ src_blocks, int nblk, int map_pitch, tb_mappoint* __restrict__ dst_rec,
               uint8_t* __restrict__ dst_desc, int32_t* __restrict__ dst_n, int32_t* __restrict__ dst_blocks) {
    const int s = blockIdx.y;
    const int n = min(max(src_n[s], 0), map_pitch);
    const int b0 = min(max(src_blocks[(size_t)s * nblk], 0), n);
    const int keep = n - b0;
    const size_t om = (size_t)s * map_pitch;
    const uint32_t* R = reinterpret_cast<const uint32_t*>(src_rec + om + b0);
    uint32_t* Rd = reinterpret_cast<uint32_t*>(dst_rec + om);
    const uint32_t* D = reinterpret_cast<const uint32_t*>(src_desc) + 8 * (om + b0);
    uint32_t* Dd = reinterpret_cast<uint32_t*>(dst_desc) + 8 * om;
    const size_t step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nr = (size_t)keep * (sizeof(tb_mappoint) / 4), nd = (size_t)keep * 8;
    for (size_t i = first; i < nr; i += step) Rd[i] = R[i];
    for (size_t i = first; i < nd; i += step) Dd[i] = D[i];
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < nblk; i += 256) dst_blocks[(size_t)s * nblk + i] = i + 1 < nblk ? src_blocks[(size_t)s * nblk + i + 1] : 0;
        if (threadIdx.x == 0) dst_n[s] = keep;
    }
}

/* ---- ragged batches (include/tb_capi.h, tb_vo_step_ragged_dev): per-sequence reset, hold of the idle sequences, the keyframe
 * block on a compacted batch. Every copy moves live entries only, through kf_copy's 16 / 4 / 1-byte lanes; which sequence a
 * workgroup serves, and whether it has anything to do, is one wave-uniform test per workgroup. */

/* tb_vo_reset_seq_dev: a selected sequence returns to the state tb_vo_reset_dev gives it -- pose Tcw0[s], no keys, no keyframe
 * (nullable arrays belong to the descriptor / BoW loops). cell_start (searchByViolence's keyframe grid, [nseq][ncell]) is
 * emptied as well: in ragged mode the matcher runs for a sequence that has no keyframe yet, and an all-zero table is an empty
 * grid. */
__global__ void __launch_bounds__(256)
k_vo_reset_seq(const int32_t* __restrict__ mask, const float* __restrict__ Tcw0, float* __restrict__ Tcw, int32_t* __restrict__ key_counts,
               int32_t* __restrict__ kf_counts, int32_t* __restrict__ kf_fv_counts, int32_t* __restrict__ kf_bv_counts,
               int32_t* __restrict__ cell_start, int ncell) {
    const int s = blockIdx.x, tid = threadIdx.x;
    if (!mask[s]) return;
    if (tid < 16) Tcw[16 * (size_t)s + tid] = Tcw0[16 * (size_t)s + tid];
    if (tid == 0) {
        key_counts[s] = 0;
        if (kf_counts) kf_counts[s] = 0;
        if (kf_fv_counts) kf_fv_counts[s] = 0;
        if (kf_bv_counts) kf_bv_counts[s] = 0;
    }
    if (cell_start)
        for (int i = tid; i < ncell; i += 256) cell_start[(size_t)s * ncell + i] = 0;
}

/* A table of row copies, the body of the two kernels below. Entry e moves sequence s's row of e.src to the same row of e.dst:
 * `count` entries of e.elem bytes, count = e.cnt[s] clamped to [0, e.lim] (e.cnt NULL: e.lim), rows e.stride entries apart. A
 * workgroup (sequence, group) walks the table and takes the entries of its group; the table lives in the kernel's argument
 * block, so the walk is scalar loads. */
#define VO_ROWS_MAX 30
struct VoRow { const uint8_t* src; uint8_t* dst; const int32_t* cnt; int lim, stride, elem, group; };
struct VoRows { VoRow r[VO_ROWS_MAX]; int n; };

__device__ __forceinline__ void vo_rows_copy(const VoRows& R, int s, int g, int tid) {
    for (int i = 0; i < R.n; i++) {
        if (R.r[i].group != g) continue;
        const size_t n = R.r[i].cnt ? (size_t)min(max(R.r[i].cnt[s], 0), R.r[i].lim) : (size_t)R.r[i].lim;
        const size_t o = (size_t)s * R.r[i].stride * R.r[i].elem;
        kf_copy(R.r[i].dst + o, R.r[i].src + o, n * R.r[i].elem, tid);
    }
}

/* The hold: after the tracking half ran over all sequences, an idle sequence (mask 0) gets back what it held -- side `a` of the
 * ping-pong and the previous step's outputs go into side `b` and this step's outputs, live entries only (the counts are the
 * held ones). Array groups (blockIdx.y): 0 keys, map points, validity, pose and every count; 1 the last left image; 2 rows and
 * outlier flags; 3 ORB records and the match list; 4 descriptors (the keys' and the ones carried with the map points); 5 the BoW
 * vectors. A sequence on its frame 0 (mask 2) matched against no keyframe: group 0 gives it what frame 0 of a lock-step loop
 * has -- no matches, no flags, no inliers, the reset pose. Mask 1: nothing. */
struct VoHoldFix { const float* a_Tcw; float* b_Tcw; int32_t *ninl, *mcnt, *mfl; };   /* mcnt / mfl: nullable */

__global__ void __launch_bounds__(256)
k_vo_hold(const int32_t* __restrict__ mask, VoHoldFix F, VoRows R) {
    const int s = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int m = mask[s];
    if (m == 1) return;
    if (m == 2) {
        if (g == 0) {
            if (tid < 16) F.b_Tcw[16 * (size_t)s + tid] = F.a_Tcw[16 * (size_t)s + tid];
            if (tid == 0) {
                F.ninl[s] = 0;
                if (F.mcnt) F.mcnt[s] = 0;
                if (F.mfl) F.mfl[s] = 0;
            }
        }
        return;
    }
    vo_rows_copy(R, s, g, tid);
}

/* The keyframe block's inputs on the compacted batch: row j gets the keys and the key count of sequence idx[j] (what the
 * stereo operator reads). */
__global__ void __launch_bounds__(256)
k_vo_kf_gather(const int32_t* __restrict__ idx, const float* __restrict__ keys, const int32_t* __restrict__ key_counts, int pitch,
               float* __restrict__ out_keys, int32_t* __restrict__ out_counts) {
    const int r = blockIdx.x, s = idx[r], tid = threadIdx.x;
    const size_t n = (size_t)min(max(key_counts[s], 0), pitch);
    kf_copy(out_keys + 2 * (size_t)r * pitch, keys + 2 * (size_t)s * pitch, n * 2 * sizeof(float), tid);
    if (tid == 0) out_counts[r] = key_counts[s];
}

/* key_frame = cur_frame_ptr for the sequences of the index list only: workgroup (j, g) copies array group g of sequence idx[j]
 * from the current frame into the keyframe snapshot, live entries only. 0 the ORB records, 1 their descriptors, 2 the map points,
 * their validity and the counts, 3 the descriptors carried with the map points (projection) or the FeatureVector keys (BoW), 4
 * the BowVector, 5 the word and node ids. */
__global__ void __launch_bounds__(256)
k_vo_kf_snapshot(const int32_t* __restrict__ idx, VoRows R) {
    vo_rows_copy(R, idx[blockIdx.x], blockIdx.y, threadIdx.x);
}

/* The two tables. Absent arrays (null destination) are left out; the returned value is the number of groups. */
static void vo_row(VoRows& R, int group, const void* src, void* dst, const int32_t* cnt, int lim, int stride, int elem) {
    if (!dst || R.n >= VO_ROWS_MAX) return;
    R.r[R.n++] = VoRow{static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), cnt, lim, stride, elem, group};
}
static void vo_row1(VoRows& R, int group, const int32_t* src, int32_t* dst) { vo_row(R, group, src, dst, nullptr, 1, 1, 4); }

static int vo_hold_rows(const tb_vo_hold_args* a, VoRows& R) {
    const tb_vo_frame_out &p = a->prev, &c = a->cur;
    const int P = a->pitch, M = a->match_pitch;
    const int32_t *kc = a->kcnt[0], *oc = p.orb_cnt;
    R.n = 0;
    vo_row(R, 0, a->keys[0], a->keys[1], kc, P, P, 8);
    vo_row(R, 0, a->mp[0], a->mp[1], kc, P, P, 12);
    vo_row(R, 0, a->valid[0], a->valid[1], kc, P, P, 1);
    vo_row(R, 0, a->Tcw[0], a->Tcw[1], nullptr, 16, 16, 4);
    vo_row1(R, 0, a->kcnt[0], a->kcnt[1]);
    vo_row1(R, 0, p.obs_counts, c.obs_counts);
    vo_row1(R, 0, p.n_inliers, c.n_inliers);
    vo_row1(R, 0, p.orb_cnt, c.orb_cnt);
    vo_row1(R, 0, p.mcounts, c.mcounts);
    vo_row1(R, 0, p.mflags, c.mflags);
    vo_row1(R, 0, p.fv_cnt, c.fv_cnt);
    vo_row1(R, 0, p.bv_cnt, c.bv_cnt);
    vo_row(R, 1, a->img[0], a->img[1], nullptr, (int)a->npx, (int)a->npx, 1);
    vo_row(R, 2, p.obs, c.obs, p.obs_counts, P, P, (int)sizeof(tb_obs));
    vo_row(R, 2, p.outlier, c.outlier, kc, P, P, 1);
    vo_row(R, 3, p.orb, c.orb, oc, P, P, (int)sizeof(tb_keypoint));
    vo_row(R, 3, p.matches, c.matches, p.mcounts, M, M, (int)sizeof(tb_match));
    vo_row(R, 4, p.orb_desc, c.orb_desc, oc, P, P, 32);
    vo_row(R, 4, p.mp_desc, c.mp_desc, kc, P, P, 32);
    vo_row(R, 5, p.bow_word, c.bow_word, oc, P, P, 4);
    vo_row(R, 5, p.bow_node, c.bow_node, oc, P, P, 4);
    vo_row(R, 5, p.fv_keys, c.fv_keys, p.fv_cnt, P, P, 8);
    vo_row(R, 5, p.bv_word, c.bv_word, p.bv_cnt, P, P, 4);
    vo_row(R, 5, p.bv_val, c.bv_val, p.bv_cnt, P, P, 8);
    return c.fv_keys ? 6 : (c.orb ? 5 : 3);
}

static int vo_snap_rows(int P, const tb_vo_frame_out* c, const float* mp, const uint8_t* valid, const tb_vo_kf_out* k, VoRows& R) {
    const int32_t* oc = c->orb_cnt;
    R.n = 0;
    vo_row(R, 0, c->orb, k->orb, oc, P, P, (int)sizeof(tb_keypoint));
    vo_row(R, 1, c->orb_desc, k->desc, oc, P, P, 32);
    vo_row(R, 2, mp, k->mp, oc, P, P, 12);
    vo_row(R, 2, valid, k->valid, oc, P, P, 1);
    vo_row1(R, 2, c->orb_cnt, k->cnt);
    vo_row1(R, 2, c->fv_cnt, k->fv_cnt);
    vo_row1(R, 2, c->bv_cnt, k->bv_cnt);
    vo_row(R, 3, c->mp_desc, k->mp_desc, oc, P, P, 32);
    vo_row(R, 3, c->fv_keys, k->fv_keys, c->fv_cnt, P, P, 8);
    vo_row(R, 4, c->bv_word, k->bv_word, c->bv_cnt, P, P, 4);
    vo_row(R, 4, c->bv_val, k->bv_val, c->bv_cnt, P, P, 8);
    vo_row(R, 5, c->bow_word, k->bow_word, oc, P, P, 4);
    vo_row(R, 5, c->bow_node, k->bow_node, oc, P, P, 4);
    return k->fv_keys ? 6 : (k->mp_desc ? 4 : 3);
}

int tbk_vo_copy_image(tb_ctx* ctx, int nimg, const uint8_t* d_src, int w, int h, int stride, size_t pitch, uint8_t* d_dst,
                      const int32_t* d_idx) {
    if (nimg <= 0) return TB_OK;
    const int bx = (int)std::min<size_t>(((size_t)w * h + 255) / 256, 512);
    return tb_launch(ctx, "k_vo_copy_image", k_vo_copy_image, dim3(bx, nimg), dim3(256), 0, d_src, w, h, stride, pitch, d_idx, d_dst);
}

int tbk_vo_track(tb_ctx* ctx, int nseq, const int32_t* d_prev_counts, const uint8_t* d_status, const float* d_keys, const float* d_prev_mp,
                 const uint8_t* d_prev_valid, int pitch, int32_t* d_key_counts, float* d_mp, uint8_t* d_valid, tb_obs* d_obs,
                 int32_t* d_obs_counts, uint8_t* d_outlier) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_track", k_vo_track, dim3(nseq), dim3(256), 0, d_prev_counts, d_status, d_keys, d_prev_mp, d_prev_valid,
                     pitch, d_key_counts, d_mp, d_valid, d_obs, d_obs_counts, d_outlier);
}

int tbk_vo_kf_pack(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, int orb_pitch, int pitch, float* d_keys,
                   int32_t* d_key_counts, uint8_t* d_valid, const int32_t* d_idx) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_kf_pack", k_vo_kf_pack, dim3(nseq), dim3(256), 0, d_orb, d_orb_counts, orb_pitch, pitch, d_keys,
                     d_key_counts, d_valid, d_idx);
}

int tbk_vo_kf_spawn(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const float* d_depth, const float* d_Tcw,
                    const double K[4], int pitch, float* d_mp, uint8_t* d_valid, const int32_t* d_idx) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_kf_spawn", k_vo_kf_spawn, dim3(nseq), dim3(256), 0, d_keys, d_key_counts, d_depth, d_Tcw, K[0], K[1], K[2],
                     K[3], pitch, d_mp, d_valid, d_idx);
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
    return tb_launch(ctx, "k_vo_match_carry", k_vo_match_carry, dim3(nseq), dim3(256), 0, d_orb, d_orb_counts, d_matches, d_match_counts,
                     d_kf_mp, d_kf_valid, d_kf_counts, pitch, sig, d_win, d_keys, d_key_counts, d_mp, d_valid, d_obs, d_obs_counts,
                     d_outlier);
}

int tbk_vo_proj_carry(tb_ctx* ctx, int nseq, int map_mode, const tb_keypoint* d_orb, const int32_t* d_orb_counts, const tb_match* d_matches,
                      const int32_t* d_match_counts, int match_pitch, const float* d_src_mp, const uint8_t* d_src_valid,
                      const tb_mappoint* d_src_rec, const uint8_t* d_src_desc, const int32_t* d_src_counts, int src_pitch, int pitch,
                      const float* inv_sigma2, int nlevels, int32_t* d_win, float* d_keys, int32_t* d_key_counts, float* d_mp,
                      uint8_t* d_valid, uint8_t* d_mp_desc, tb_obs* d_obs, int32_t* d_obs_counts, uint8_t* d_outlier) {
    if (nseq <= 0) return TB_OK;
    if (nlevels < 1 || nlevels > TB_MAX_LEVELS || match_pitch < 1 || src_pitch < 1) return TB_EINVAL;
    tb_vo_sigma sig = {};
    for (int l = 0; l < nlevels; l++) sig.v[l] = inv_sigma2[l];
    sig.n = nlevels;
    return tb_launch(ctx, map_mode ? "k_vo_proj_carry_map" : "k_vo_proj_carry_kf", map_mode ? k_vo_proj_carry<true> : k_vo_proj_carry<false>,
                     dim3(nseq), dim3(256), 0, d_orb, d_orb_counts, d_matches, d_match_counts, match_pitch, d_src_mp, d_src_valid, d_src_rec,
                     d_src_desc, d_src_counts, src_pitch, pitch, sig, d_win, d_keys, d_key_counts, d_mp, d_valid, d_mp_desc, d_obs, d_obs_counts,
                     d_outlier);
}

int tbk_vo_kf_append(tb_ctx* ctx, int nseq, const int32_t* d_key_counts, const float* d_depth, const float* d_mp, const uint8_t* d_valid,
                     const uint8_t* d_orb_desc, const float* d_Tcw, int pitch, uint8_t* d_mp_desc, tb_mappoint* d_rec,
                     tb_mappoint* d_map_rec, uint8_t* d_map_desc, int32_t* d_map_n, int32_t* d_map_blocks, int nblk, int slot,
                     int map_pitch, const int32_t* d_idx) {
    if (nseq <= 0) return TB_OK;
    if (d_map_rec && (nblk < 1 || slot < 0 || slot >= nblk || map_pitch < 1)) return TB_EINVAL;
    return tb_launch(ctx, "k_vo_kf_append", k_vo_kf_append, dim3(nseq), dim3(256), 0, d_key_counts, d_depth, d_mp, d_valid, d_orb_desc,
                     d_Tcw, pitch, d_mp_desc, d_rec, d_map_rec, d_map_desc, d_map_n, d_map_blocks, nblk, slot, map_pitch, d_idx);
}

int tbk_vo_map_evict(tb_ctx* ctx, int nseq, const tb_mappoint* d_src_rec, const uint8_t* d_src_desc, const int32_t* d_src_n,
                     const int32_t* d_src_blocks, int nblk, int map_pitch, tb_mappoint* d_dst_rec, uint8_t* d_dst_desc, int32_t* d_dst_n,
                     int32_t* d_dst_blocks) {
    if (nseq <= 0) return TB_OK;
    if (nblk < 1 || map_pitch < 1) return TB_EINVAL;
    return tb_launch(ctx, "k_vo_map_evict", k_vo_map_evict, dim3(8, nseq), dim3(256), 0, d_src_rec, d_src_desc, d_src_n, d_src_blocks, nblk,
                     map_pitch, d_dst_rec, d_dst_desc, d_dst_n, d_dst_blocks);
}

int tbk_vo_reset_seq(tb_ctx* ctx, int nseq, const int32_t* d_mask, const float* d_Tcw0, float* d_Tcw, int32_t* d_key_counts,
                     int32_t* d_kf_counts, int32_t* d_kf_fv_counts, int32_t* d_kf_bv_counts, int32_t* d_cell_start, int ncell) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_reset_seq", k_vo_reset_seq, dim3(nseq), dim3(256), 0, d_mask, d_Tcw0, d_Tcw, d_key_counts, d_kf_counts,
                     d_kf_fv_counts, d_kf_bv_counts, d_cell_start, ncell);
}

int tbk_vo_hold(tb_ctx* ctx, int nseq, const tb_vo_hold_args* a) {
    if (nseq <= 0) return TB_OK;
    if (a->npx > (size_t)INT32_MAX) return TB_EINVAL;
    VoRows R;
    const int groups = vo_hold_rows(a, R);
    const VoHoldFix F = {a->Tcw[0], a->Tcw[1], a->cur.n_inliers, a->cur.mcounts, a->cur.mflags};
    return tb_launch(ctx, "k_vo_hold", k_vo_hold, dim3(nseq, groups), dim3(256), 0, a->mask, F, R);
}

int tbk_vo_kf_gather(tb_ctx* ctx, int nkf, const int32_t* d_idx, const float* d_keys, const int32_t* d_key_counts, int pitch,
                     float* d_out_keys, int32_t* d_out_counts) {
    if (nkf <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_kf_gather", k_vo_kf_gather, dim3(nkf), dim3(256), 0, d_idx, d_keys, d_key_counts, pitch, d_out_keys,
                     d_out_counts);
}

int tbk_vo_kf_snapshot(tb_ctx* ctx, int nkf, const int32_t* d_idx, int pitch, const tb_vo_frame_out* cur, const float* d_mp,
                       const uint8_t* d_valid, const tb_vo_kf_out* kf) {
    if (nkf <= 0) return TB_OK;
    VoRows R;
    const int groups = vo_snap_rows(pitch, cur, d_mp, d_valid, kf, R);
    if (!d_idx) {   /* sequences [0, nkf): the same table, one copy of the whole slab per row */
        for (int i = 0; i < R.n; i++)
            TB_HIP(ctx, hipMemcpyAsync(R.r[i].dst, R.r[i].src, (size_t)nkf * R.r[i].stride * R.r[i].elem, hipMemcpyDeviceToDevice, ctx->stream));
        return TB_OK;
    }
    return tb_launch(ctx, "k_vo_kf_snapshot", k_vo_kf_snapshot, dim3(nkf, groups), dim3(256), 0, d_idx, R);
}

/* ---- window BA of the optical-flow loop (include/tb_capi.h, tb_vo_window_ba_enable): between two keyframes key i of every frame
 * is the same physical point, so the frames of a segment are a BA window over the keyframe's stereo points. The segment log is
 * [nseq][nslot] rows at the loop's key pitch, slot 0 = the keyframe, slot j = the frame j steps after it. Every ok / spawned row
 * is written over the whole pitch (zeros past the key count), so the window builder walks the pitch without a count. */

/* Segment start, at the end of a keyframe step's keyframe block: slot 0 takes the keyframe's keys (after SetKeys) and pose, the
 * segment takes the frame's map points (zeros where a key has none: those entries of the frame are never written), and spawned[i] says that the keyframe made a new stereo point at key i in this step --
 * k_vo_kf_spawn's own test on depth[i]. An entry that only survived SetKeys' resize is valid but not spawned. */
__global__ void __launch_bounds__(256)
k_vo_seg_start(const float* __restrict__ keys, const int32_t* __restrict__ key_counts, const float* __restrict__ depth,
               const float* __restrict__ mp, const uint8_t* __restrict__ valid, const float* __restrict__ Tcw, int pitch, int nslot,
               float* __restrict__ seg_keys,
               uint8_t* __restrict__ seg_ok, float* __restrict__ seg_pose, float* __restrict__ seg_pts,
               uint8_t* __restrict__ seg_spawned) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int m = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch, o0 = (size_t)s * nslot * pitch;
    for (int i = tid; i < pitch; i += 256) {
        uint8_t sp = 0;
        float X = 0.f, Y = 0.f, Z = 0.f;
        if (i < m) {
            const float d = depth[o + i];
            sp = (d > 0.f && isfinite(d)) ? 1 : 0;
            seg_keys[2 * (o0 + i)] = keys[2 * (o + i)]; seg_keys[2 * (o0 + i) + 1] = keys[2 * (o + i) + 1];
            if (valid[o + i]) { X = mp[3 * (o + i)]; Y = mp[3 * (o + i) + 1]; Z = mp[3 * (o + i) + 2]; }
        }
        seg_pts[3 * (o + i)] = X; seg_pts[3 * (o + i) + 1] = Y; seg_pts[3 * (o + i) + 2] = Z;
        seg_spawned[o + i] = sp;
        seg_ok[o0 + i] = sp;
    }
    if (tid < 16) seg_pose[16 * (size_t)s * nslot + tid] = Tcw[16 * (size_t)s + tid];
}

/* Frame t > 0 after its tracking half, into slot j = t - (the keyframe's frame): the tracked key list, the optimised pose, and
 * ok[i] = spawned[i] & valid[i] & !outlier[row(i)], where row(i) is key i's rank among the frame's valid keys -- the ballot /
 * prefix compaction in key order by which k_vo_track emitted the rows PoseOptimization flagged. With fewer than 3 rows the pose
 * was held and nothing is an inlier: ok is 0. valid chains from frame to frame, so a point lost once stays out. */
__global__ void __launch_bounds__(256)
k_vo_seg_log(const float* __restrict__ keys, const int32_t* __restrict__ key_counts, const uint8_t* __restrict__ valid,
             const uint8_t* __restrict__ outlier, const int32_t* __restrict__ obs_counts, const float* __restrict__ Tcw,
             const uint8_t* __restrict__ seg_spawned, int pitch, int nslot, int slot, float* __restrict__ seg_keys,
             uint8_t* __restrict__ seg_ok, float* __restrict__ seg_pose) {
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(key_counts[s], 0), pitch);
    const bool held = obs_counts[s] < 3;
    const size_t o = (size_t)s * pitch, oj = ((size_t)s * nslot + slot) * pitch;
    int base = 0;
    for (int i0 = 0; i0 < pitch; i0 += 256) {
        const int i = i0 + tid;
        const bool v = i < n && valid[o + i];
        const int row = tb_block_ordered_slot(v, base, wsum);   /* row < n <= pitch */
        if (i < n) { seg_keys[2 * (oj + i)] = keys[2 * (o + i)]; seg_keys[2 * (oj + i) + 1] = keys[2 * (o + i) + 1]; }
        if (i < pitch) seg_ok[oj + i] = (v && !held && seg_spawned[o + i] && !outlier[o + row]) ? 1 : 0;
    }
    if (tid < 16) seg_pose[16 * ((size_t)s * nslot + slot) + tid] = Tcw[16 * (size_t)s + tid];
}

/* The window of a segment, one workgroup per sequence: point i contributes its ok slots when there are at least min_obs of
 * them; an exclusive scan of those counts over the points (wave scans, the wave totals through LDS, a running base over the
 * 256-point slabs) places them, so the observations come out grouped by ascending point and, within a point, by ascending slot:
 * the order tb_local_ba_batch_dev requires. kf = the slot, pt = the key index, inv_sigma2 = 1 (octave 0, as the pose rows).
 * A point has at most nslot observations, so the list fits obs_pitch = nslot * pitch. */
__global__ void __launch_bounds__(256)
k_vo_seg_window(const float* __restrict__ seg_keys, const uint8_t* __restrict__ seg_ok, int pitch, int nslot, int min_obs,
                tb_ba_obs* __restrict__ obs, int32_t* __restrict__ obs_counts, int32_t* __restrict__ n_points) {
    __shared__ int wsum[4], wpts[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o0 = (size_t)s * nslot * pitch;
    tb_ba_obs* O = obs + o0;
    int base = 0, npts = 0;
    for (int i0 = 0; i0 < pitch; i0 += 256) {
        const int i = i0 + tid;
        int c = 0;
        if (i < pitch)
            for (int j = 0; j < nslot; j++) c += seg_ok[o0 + (size_t)j * pitch + i] ? 1 : 0;
        if (c < min_obs) c = 0;
        const int incl = tb_wave_incl_scan(c);
        const unsigned long long bm = __ballot(c > 0);
        if (lane == 63) wsum[wave] = incl;
        if (lane == 0) wpts[wave] = __popcll(bm);
        __syncthreads();
        int at = base + incl - c;
        for (int w = 0; w < wave; w++) at += wsum[w];
        if (c > 0)
            for (int j = 0; j < nslot; j++) {
                const size_t e = o0 + (size_t)j * pitch + i;
                if (!seg_ok[e]) continue;
                tb_ba_obs r;
                r.kf = j; r.pt = i; r.u = seg_keys[2 * e]; r.v = seg_keys[2 * e + 1]; r.inv_sigma2 = 1.0f;
                O[at++] = r;   /* at < sum of the counts <= nslot * pitch */
            }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        npts += wpts[0] + wpts[1] + wpts[2] + wpts[3];
        __syncthreads();
    }
    if (tid == 0) { obs_counts[s] = base; n_points[s] = npts; }
}

/* After the BA: the frame's pose, on the side the keyframe block reads, takes the refined pose of the window's last slot when
 * the window had at least min_points points, the BA accepted its observations (stats[7] != -1) and every entry of that pose is
 * finite. Otherwise the pose keeps every bit. One wavefront per sequence. */
__global__ void __launch_bounds__(64)
k_vo_seg_adopt(const float* __restrict__ win_pose, const int32_t* __restrict__ n_points, const double* __restrict__ stats, int nslot,
               int min_points, float* __restrict__ Tcw, uint8_t* __restrict__ adopted) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const float v = lane < 16 ? win_pose[16 * ((size_t)s * nslot + nslot - 1) + lane] : 0.f;
    const bool fin = __ballot(!isfinite(v)) == 0ull;
    const bool ok = fin && n_points[s] >= min_points && stats[8 * (size_t)s + 7] != -1.0;
    if (ok && lane < 16) Tcw[16 * (size_t)s + lane] = v;
    if (lane == 0) adopted[s] = ok ? 1 : 0;
}

int tbk_vo_seg_start(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const float* d_depth, const float* d_mp,
                     const uint8_t* d_valid, const float* d_Tcw, int pitch, int nslot, float* d_seg_keys, uint8_t* d_seg_ok, float* d_seg_pose, float* d_seg_pts,
                     uint8_t* d_seg_spawned) {
    if (nseq <= 0) return TB_OK;
    if (pitch < 1 || nslot < 2) return TB_EINVAL;
    return tb_launch(ctx, "k_vo_seg_start", k_vo_seg_start, dim3(nseq), dim3(256), 0, d_keys, d_key_counts, d_depth, d_mp, d_valid, d_Tcw,
                     pitch, nslot, d_seg_keys, d_seg_ok, d_seg_pose, d_seg_pts, d_seg_spawned);
}

int tbk_vo_seg_log(tb_ctx* ctx, int nseq, const float* d_keys, const int32_t* d_key_counts, const uint8_t* d_valid, const uint8_t* d_outlier,
                   const int32_t* d_obs_counts, const float* d_Tcw, const uint8_t* d_seg_spawned, int pitch, int nslot, int slot,
                   float* d_seg_keys, uint8_t* d_seg_ok, float* d_seg_pose) {
    if (nseq <= 0) return TB_OK;
    if (pitch < 1 || slot < 1 || slot >= nslot) return TB_EINVAL;
    return tb_launch(ctx, "k_vo_seg_log", k_vo_seg_log, dim3(nseq), dim3(256), 0, d_keys, d_key_counts, d_valid, d_outlier, d_obs_counts,
                     d_Tcw, d_seg_spawned, pitch, nslot, slot, d_seg_keys, d_seg_ok, d_seg_pose);
}

int tbk_vo_seg_window(tb_ctx* ctx, int nseq, const float* d_seg_keys, const uint8_t* d_seg_ok, int pitch, int nslot, int min_obs,
                      tb_ba_obs* d_obs, int32_t* d_obs_counts, int32_t* d_n_points) {
    if (nseq <= 0) return TB_OK;
    if (pitch < 1 || nslot < 2 || min_obs < 1) return TB_EINVAL;
    return tb_launch(ctx, "k_vo_seg_window", k_vo_seg_window, dim3(nseq), dim3(256), 0, d_seg_keys, d_seg_ok, pitch, nslot, min_obs, d_obs,
                     d_obs_counts, d_n_points);
}

int tbk_vo_seg_adopt(tb_ctx* ctx, int nseq, const float* d_win_pose, const int32_t* d_n_points, const double* d_stats, int nslot,
                     int min_points, float* d_Tcw, uint8_t* d_adopted) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_seg_adopt", k_vo_seg_adopt, dim3(nseq), dim3(64), 0, d_win_pose, d_n_points, d_stats, nslot, min_points,
                     d_Tcw, d_adopted);
}

/* ---- mono mode of the optical-flow loop (include/tb_capi.h, tb_vo_mono) */

/* After a tracking half: a key stays a triangulation candidate while LK has held it in every frame since the keyframe
 * (alive[i] &= status[i]); skip[i] = it has a map point already, or it was lost. */
__global__ void __launch_bounds__(256)
k_vo_mono_alive(const int32_t* __restrict__ key_counts, const uint8_t* __restrict__ status, const uint8_t* __restrict__ valid, int pitch,
                uint8_t* __restrict__ alive, uint8_t* __restrict__ skip) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(key_counts[s], 0), pitch);
    if (i >= n) return;
    const size_t o = (size_t)s * pitch + i;
    const uint8_t a = alive[o] && status[o] ? 1 : 0;
    alive[o] = a;
    skip[o] = valid[o] || !a ? 1 : 0;
}

/* ---- the mono loop without a right image (include/tb_capi.h, tb_vo_mono_init) */

/* Before a keyframe's triangulation: a sequence that is not initialised leaves the triangulation and is a two-view problem over
 * the keys LK still holds; an initialised one is no two-view problem and keeps the triangulation's skip bytes. */
__global__ void __launch_bounds__(256)
k_vo_init_prep(const uint8_t* __restrict__ initialised, const uint8_t* __restrict__ alive, int pitch, uint8_t* __restrict__ tri_skip,
               uint8_t* __restrict__ tv_skip) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pitch) return;
    const size_t o = (size_t)s * pitch + i;
    const bool ini = initialised[s] != 0;
    tv_skip[o] = ini || !alive[o] ? 1 : 0;
    if (!ini) tri_skip[o] = 1;
}

/* After the two-view call, one workgroup per sequence that is not initialised: the attempt's results (w_res, in planes: status, consensus,
 * winner[2], good[4], tri[4]; w_Tcw1) are kept; with status 0 and at least min_tracks alive keys the sequence takes the pose and,
 * through the triangulation's outputs the merge reads, the points. An initialised sequence keeps every byte. */
__global__ void __launch_bounds__(256)
k_vo_init_adopt(int t, int min_tracks, const int32_t* __restrict__ key_counts, const uint8_t* __restrict__ alive, int pitch,
                const int32_t* __restrict__ w_res, const float* __restrict__ w_Tcw1, const float* __restrict__ points,
                const uint8_t* __restrict__ pflags, uint8_t* __restrict__ initialised, int32_t* __restrict__ init_frame,
                int32_t* __restrict__ attempts, int32_t* __restrict__ res, float* __restrict__ Tcw1, float* __restrict__ Tcw,
                float* __restrict__ tri_points, uint8_t* __restrict__ tri_flags) {
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (initialised[s]) return;   /* block-uniform; written below only behind the barrier */
    const int n = min(max(key_counts[s], 0), pitch);
    const size_t o = (size_t)s * pitch;
    int cnt = 0;
    for (int i = tid; i < n; i += 256) cnt += alive[o + i] ? 1 : 0;
    cnt = tb_wave_sum(cnt);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    const int tracks = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const size_t S = gridDim.x;   /* planes: status [S], consensus [S], winner [S][2], good [S][4], tri [S][4] */
    const bool ok = w_res[s] == 0 && tracks >= min_tracks;
    if (tid < 12) {
        const size_t at = tid == 0 ? (size_t)s : tid == 1 ? S + s : tid < 4 ? 2 * S + 2 * (size_t)s + (tid - 2)
                        : tid < 8 ? 4 * S + 4 * (size_t)s + (tid - 4) : 8 * S + 4 * (size_t)s + (tid - 8);
        res[at] = w_res[at];
    }
    if (tid < 16) {
        const float v = w_Tcw1[16 * s + tid];
        Tcw1[16 * s + tid] = v;
        if (ok) Tcw[16 * s + tid] = v;
    }
    if (ok)
        for (int i = tid; i < n; i += 256)
            if (pflags[o + i] == 1) {
                tri_points[3 * (o + i)] = points[3 * (o + i)];
                tri_points[3 * (o + i) + 1] = points[3 * (o + i) + 1];
                tri_points[3 * (o + i) + 2] = points[3 * (o + i) + 2];
                tri_flags[o + i] = 1;
            }
    if (tid == 0) {
        attempts[s] += 1;
        if (ok) { initialised[s] = 1; init_frame[s] = t; }
    }
}

int tbk_vo_init_prep(tb_ctx* ctx, int nseq, const uint8_t* d_initialised, const uint8_t* d_alive, int pitch, uint8_t* d_tri_skip,
                     uint8_t* d_tv_skip) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_init_prep", k_vo_init_prep, dim3((pitch + 255) / 256, nseq), dim3(256), 0, d_initialised, d_alive, pitch,
                     d_tri_skip, d_tv_skip);
}

int tbk_vo_init_adopt(tb_ctx* ctx, int nseq, int t, int min_tracks, const int32_t* d_key_counts, const uint8_t* d_alive, int pitch,
                      const int32_t* d_w_res, const float* d_w_Tcw1, const float* d_points, const uint8_t* d_pflags,
                      uint8_t* d_initialised, int32_t* d_init_frame, int32_t* d_attempts, int32_t* d_res, float* d_Tcw1, float* d_Tcw,
                      float* d_tri_points, uint8_t* d_tri_flags) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_init_adopt", k_vo_init_adopt, dim3(nseq), dim3(256), 0, t, min_tracks, d_key_counts, d_alive, pitch, d_w_res,
                     d_w_Tcw1, d_points, d_pflags, d_initialised, d_init_frame, d_attempts, d_res, d_Tcw1, d_Tcw, d_tri_points, d_tri_flags);
}

/* The occupancy cell of a pixel, -1 outside the cw x ch grid (and for a coordinate no int holds) */
__device__ __forceinline__ int vo_merge_cell(float x, float y, int cell, int cw, int ch) {
    if (!(fabsf(x) < 1.0e9f) || !(fabsf(y) < 1.0e9f)) return -1;
    const int cx = (int)x / cell, cy = (int)y / cell;
    if (cx < 0 || cx >= cw || cy < 0 || cy >= ch) return -1;
    return cy * cw + cx;
}

/* Mono keyframe: the new key list of sequence s, from side src of the ping-pong into side dst (never in place).
 *   survivors  every key that has a map point -- valid[i], or triangulated in this step (tri_flags[i] == 1: its point is
 *              tri_points[i]) -- in index order, with its point; each marks its cell in the LDS bitmap (cw * ch bits)
 *   new keys   the ORB keys in extractor order, without a map point, except those whose cell holds a survivor, while the list
 *              has room (pitch keys)
 * kf_keys takes the new list and alive = 1: the next segment's keyframe. Both compactions are tb_block_ordered_slot's. */
__global__ void __launch_bounds__(256)
k_vo_kf_merge(const tb_keypoint* __restrict__ orb, const int32_t* __restrict__ orb_counts, int orb_pitch, int pitch, int cell, int cw, int ch,
              const float* __restrict__ src_keys, const int32_t* __restrict__ src_counts, const float* __restrict__ src_mp,
              const uint8_t* __restrict__ src_valid, const float* __restrict__ tri_points, const uint8_t* __restrict__ tri_flags,
              float* __restrict__ keys, int32_t* __restrict__ key_counts, float* __restrict__ mp, uint8_t* __restrict__ valid,
              float* __restrict__ kf_keys, uint8_t* __restrict__ alive, int32_t* __restrict__ survivors, int32_t* __restrict__ added) {
    extern __shared__ unsigned int vo_bitmap[];
    __shared__ int wsum[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int ncell = cw * ch, nword = (ncell + 31) >> 5;
    const int n = min(max(src_counts[s], 0), pitch);
    const int m = min(min(max(orb_counts[s], 0), orb_pitch), pitch);
    const size_t o = (size_t)s * pitch;
    const tb_keypoint* K = orb + (size_t)s * orb_pitch;
    for (int w = tid; w < nword; w += 256) vo_bitmap[w] = 0u;
    __syncthreads();
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false, tri = false;
        if (i < n) {
            tri = tri_flags[o + i] == 1;
            ok = tri || src_valid[o + i];
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) {   /* at <= i < pitch */
            const float x = src_keys[2 * (o + i)], y = src_keys[2 * (o + i) + 1];
            const float* X = tri ? tri_points + 3 * (o + i) : src_mp + 3 * (o + i);
            keys[2 * (o + at)] = x; keys[2 * (o + at) + 1] = y;
            kf_keys[2 * (o + at)] = x; kf_keys[2 * (o + at) + 1] = y;
            mp[3 * (o + at)] = X[0]; mp[3 * (o + at) + 1] = X[1]; mp[3 * (o + at) + 2] = X[2];
            valid[o + at] = 1;
            const int c = vo_merge_cell(x, y, cell, cw, ch);
            if (c >= 0 && c < ncell) atomicOr(&vo_bitmap[c >> 5], 1u << (c & 31));
        }
    }
    const int nsurv = base;
    __syncthreads();   /* the bitmap is complete */
    for (int j0 = 0; j0 < m && base < pitch; j0 += 256) {   /* base is the same in every thread */
        const int j = j0 + tid;
        bool ok = false;
        float x = 0.f, y = 0.f;
        if (j < m) {
            x = K[j].x; y = K[j].y;
            const int c = vo_merge_cell(x, y, cell, cw, ch);
            ok = !(c >= 0 && c < ncell && ((vo_bitmap[c >> 5] >> (c & 31)) & 1u));
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok && at < pitch) {
            keys[2 * (o + at)] = x; keys[2 * (o + at) + 1] = y;
            kf_keys[2 * (o + at)] = x; kf_keys[2 * (o + at) + 1] = y;
            mp[3 * (o + at)] = 0.f; mp[3 * (o + at) + 1] = 0.f; mp[3 * (o + at) + 2] = 0.f;
            valid[o + at] = 0;
        }
    }
    const int total = min(base, pitch);
    for (int k = tid; k < pitch; k += 256) {
        alive[o + k] = 1;
        if (k >= total) valid[o + k] = 0;
    }
    if (tid == 0) { key_counts[s] = total; survivors[s] = nsurv; added[s] = total - nsurv; }
}

size_t tbk_vo_merge_bitmap_bytes(int width, int height, int cell) {
    const size_t cw = ((size_t)width + cell - 1) / cell, ch = ((size_t)height + cell - 1) / cell;
    return (cw * ch + 31) / 32 * 4;
}

int tbk_vo_mono_alive(tb_ctx* ctx, int nseq, const int32_t* d_key_counts, const uint8_t* d_status, const uint8_t* d_valid, int pitch,
                      uint8_t* d_alive, uint8_t* d_skip) {
    if (nseq <= 0) return TB_OK;
    return tb_launch(ctx, "k_vo_mono_alive", k_vo_mono_alive, dim3((pitch + 255) / 256, nseq), dim3(256), 0, d_key_counts, d_status, d_valid,
                     pitch, d_alive, d_skip);
}

int tbk_vo_kf_merge(tb_ctx* ctx, int nseq, const tb_keypoint* d_orb, const int32_t* d_orb_counts, int orb_pitch, int pitch, int width,
                    int height, int cell, const float* d_src_keys, const int32_t* d_src_counts, const float* d_src_mp,
                    const uint8_t* d_src_valid, const float* d_tri_points, const uint8_t* d_tri_flags, float* d_keys,
                    int32_t* d_key_counts, float* d_mp, uint8_t* d_valid, float* d_kf_keys, uint8_t* d_alive, int32_t* d_survivors,
                    int32_t* d_added) {
    if (nseq <= 0) return TB_OK;
    if (cell < 1 || pitch < 1 || width < 1 || height < 1) return TB_EINVAL;
    const size_t lds = tbk_vo_merge_bitmap_bytes(width, height, cell);
    if (lds > TB_VO_MERGE_BITMAP_MAX) return tb_fail(ctx, TB_EINVAL, "k_vo_kf_merge: a bitmap of %zu bytes (cell %d)", lds, cell);
    return tb_launch(ctx, "k_vo_kf_merge", k_vo_kf_merge, dim3(nseq), dim3(256), lds, d_orb, d_orb_counts, orb_pitch, pitch, cell,
                     (width + cell - 1) / cell, (height + cell - 1) / cell, d_src_keys, d_src_counts, d_src_mp, d_src_valid, d_tri_points,
                     d_tri_flags, d_keys, d_key_counts, d_mp, d_valid, d_kf_keys, d_alive, d_survivors, d_added);
}
