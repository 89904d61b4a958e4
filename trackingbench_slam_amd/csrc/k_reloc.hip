/* The keyframe store and the verification of keyframe-database candidates (relocalisation pose): the copy and compaction
 * kernels around the batched searchByBow (k_match.hip, matcher.cpp:619-721) and PoseOptimization (k_pose.hip,
 * LocalBA.cpp:291-490). See include/tb_capi.h, tb_kf_store / tb_relocalize_batch_dev.
 *
 * A store array is [nseq][cap][pitch]: frame index s * cap + slot, so the matcher reads a stored keyframe in place. */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_kfcopy.h"

struct KfStoreArrays {
    tb_keypoint* keys;          /* [nseq][cap][pitch] */
    uint8_t* desc;              /* [nseq][cap][pitch][32] */
    unsigned long long* fv;     /* [nseq][cap][pitch] */
    float* mp;                  /* [nseq][cap][pitch][3] */
    uint8_t* valid;             /* [nseq][cap][pitch] */
    float* Tcw;                 /* [nseq][cap][16] */
    int32_t *counts, *fv_counts, *kf_ids;   /* [nseq][cap] */
};
struct KfStoreSrc {
    const tb_keypoint* keys;
    const uint8_t* desc;
    const unsigned long long* fv;
    const float* mp;
    const uint8_t* valid;
    const float* Tcw;
    const int32_t *counts, *fv_counts;
};

/* One add of the store: workgroup (s, g) copies array group g of sequence s's snapshot (src [nseq][src_pitch]) into ring slot
 * `slot`: 0 the key records, 1 the descriptors, 2 the FeatureVector keys, 3 the map points, their validity, the pose and the
 * slot's header. Only the live entries move (the counts, clamped to both pitches); what lies beyond them keeps what it held. */
__global__ void __launch_bounds__(256)
k_kf_store_add(KfStoreSrc A, int src_pitch, int cap, int pitch, int slot, int32_t kf_id, KfStoreArrays D) {
    const int s = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int lim = min(src_pitch, pitch);
    const size_t n = (size_t)min(max(A.counts[s], 0), lim), nf = (size_t)min(max(A.fv_counts[s], 0), lim);
    const size_t src = (size_t)s * src_pitch, f = (size_t)s * cap + slot, dst = f * pitch;
    if (g == 0) {
        kf_copy(D.keys + dst, A.keys + src, n * sizeof(tb_keypoint), tid);
    } else if (g == 1) {
        kf_copy(D.desc + 32 * dst, A.desc + 32 * src, n * 32, tid);
    } else if (g == 2) {
        kf_copy(D.fv + dst, A.fv + src, nf * sizeof(unsigned long long), tid);
    } else {
        kf_copy(D.mp + 3 * dst, A.mp + 3 * src, n * 3 * sizeof(float), tid);
        kf_copy(D.valid + dst, A.valid + src, n, tid);
        if (tid < 16) D.Tcw[16 * f + tid] = A.Tcw[16 * (size_t)s + tid];
        if (tid == 0) { D.counts[f] = (int32_t)n; D.fv_counts[f] = (int32_t)nf; D.kf_ids[f] = kf_id; }
    }
}

/* Pair c = s * ncand + r: the frame indices the matcher takes (side 1: the query frame s; side 2: the stored keyframe
 * s * cap + slot, or -1 where there is no candidate -- a slot of -1, one outside the ring, or an empty one), the pose
 * optimisation's seed (the keyframe's pose; the identity without a candidate) and the candidate's keyframe id. */
__global__ void __launch_bounds__(256)
k_reloc_pairs(int npairs, int ncand, int cap, const int32_t* __restrict__ cand_slot, const int32_t* __restrict__ kf_ids,
              const float* __restrict__ kf_Tcw, int32_t* __restrict__ ix1, int32_t* __restrict__ ix2, float* __restrict__ seed,
              int32_t* __restrict__ cand_kf) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= npairs) return;
    const int s = c / ncand, slot = cand_slot[c];
    int f = -1, kf = -1;
    if (slot >= 0 && slot < cap) {
        kf = kf_ids[(size_t)s * cap + slot];
        if (kf >= 0) f = s * cap + slot; else kf = -1;
    }
    ix1[c] = s; ix2[c] = f; cand_kf[c] = kf;
    for (int i = 0; i < 16; i++) seed[16 * (size_t)c + i] = f >= 0 ? kf_Tcw[16 * (size_t)f + i] : ((i & 3) == (i >> 2) ? 1.f : 0.f);
}

/* PoseOptimization's rows of pair c (one workgroup each), by k_vo_match_carry's rule without its side effects: for every match
 * whose stored entry trainIdx has a map point, key queryIdx gets that point, the last such match in list order winning a key
 * (win[], in LDS: one int per query key); then one row per key that has a point, IN KEY ORDER (LocalBA.cpp:333-363): px = the
 * query key, Xw = the stored map point, invSigma2 = invLevelSigma2[octave] (:349). The outlier flags of the query's keys are
 * cleared. Without a candidate: no rows. */
struct tb_reloc_sigma {
    float v[TB_MAX_LEVELS];
    int n;
};
__global__ void __launch_bounds__(256)
k_reloc_rows(const tb_keypoint* __restrict__ q_keys, const int32_t* __restrict__ q_counts, int q_pitch, const int32_t* __restrict__ ix1,
             const int32_t* __restrict__ ix2, const tb_match* __restrict__ matches, const int32_t* __restrict__ match_counts,
             const float* __restrict__ kf_mp, const uint8_t* __restrict__ kf_valid, const int32_t* __restrict__ kf_counts, int pitch,
             tb_reloc_sigma sig, tb_obs* __restrict__ obs, int32_t* __restrict__ obs_counts, uint8_t* __restrict__ outlier,
             int32_t* __restrict__ rows_out) {
    extern __shared__ int win[];   /* [q_pitch] */
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int s = ix1[c], f = ix2[c];
    if (f < 0 || s < 0) {
        if (tid == 0) { obs_counts[c] = 0; if (rows_out) rows_out[c] = 0; }
        return;
    }
    const int n = min(max(q_counts[s], 0), q_pitch);
    const int nm = min(max(match_counts[c], 0), pitch);
    const int nk = min(max(kf_counts[f], 0), pitch);
    const tb_keypoint* K = q_keys + (size_t)s * q_pitch;
    const tb_match* M = matches + (size_t)c * pitch;
    const float* MP = kf_mp + 3 * (size_t)f * pitch;
    const uint8_t* V = kf_valid + (size_t)f * pitch;
    tb_obs* O = obs + (size_t)c * pitch;
    uint8_t* OUT = outlier + (size_t)c * pitch;
    for (int i = tid; i < n; i += 256) win[i] = -1;
    __syncthreads();
    for (int k = tid; k < nm; k += 256) {
        const int q = M[k].queryIdx, tr = M[k].trainIdx;
        if (q >= 0 && q < n && tr >= 0 && tr < nk && V[tr]) atomicMax(&win[q], k);
    }
    __syncthreads();
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        tb_obs r = {0, 0, 0, 0, 0, 0};
        if (i < n) {
            const int k = win[i];
            ok = k >= 0;
            OUT[i] = 0;
            if (ok) {
                const int j = M[k].trainIdx;
                const tb_keypoint kp = K[i];
                r.u = kp.x; r.v = kp.y;
                r.X = MP[3 * j]; r.Y = MP[3 * j + 1]; r.Z = MP[3 * j + 2];
                r.inv_sigma2 = sig.v[min(max(kp.octave, 0), sig.n - 1)];
            }
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok) O[at] = r; /* at < n <= q_pitch <= pitch */
    }
    if (tid == 0) { obs_counts[c] = base; if (rows_out) rows_out[c] = base; }
}

/* Per sequence (one thread each): the candidate with the most inliers, ties to the lower rank, candidates that are absent left
 * out; it is the answer when its inliers reach min_inliers. best_rank -1: best_kf -1 and the identity pose. */
__global__ void __launch_bounds__(256)
k_reloc_select(int nseq, int ncand, int min_inliers, const int32_t* __restrict__ cand_kf, const int32_t* __restrict__ cand_inliers,
               const float* __restrict__ cand_Tcw, int32_t* __restrict__ best_rank, int32_t* __restrict__ best_kf,
               float* __restrict__ best_Tcw) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseq) return;
    int best = -1, most = -1;
    for (int r = 0; r < ncand; r++) {
        const size_t c = (size_t)s * ncand + r;
        if (cand_kf[c] < 0) continue;
        const int ni = cand_inliers[c];
        if (ni > most) { most = ni; best = r; }
    }
    if (best >= 0 && most < min_inliers) best = -1;
    if (best_rank) best_rank[s] = best;
    if (best_kf) best_kf[s] = best >= 0 ? cand_kf[(size_t)s * ncand + best] : -1;
    if (best_Tcw)
        for (int i = 0; i < 16; i++)
            best_Tcw[16 * (size_t)s + i] = best >= 0 ? cand_Tcw[16 * ((size_t)s * ncand + best) + i] : ((i & 3) == (i >> 2) ? 1.f : 0.f);
}

/* ---- recovery in the VO loop (tb_vo_recover_enable): a lost sequence adopts the verification's winner. All masking is by the
 * device predicates below; a sequence that does not adopt keeps every byte of its state. */

/* Entry i = s * topk + r: lost[s] = n_inliers[s] < lost_inliers and the tracker's own count (written once per sequence), and the
 * masked copy of the query's top_slot: a sequence that is not lost has no candidate, so its pairs read nothing. */
__global__ void __launch_bounds__(256)
k_vo_recover_mask(int nseq, int topk, int lost_inliers, const int32_t* __restrict__ n_inliers, const int32_t* __restrict__ top_slot,
                  uint8_t* __restrict__ lost, int32_t* __restrict__ track_inliers, int32_t* __restrict__ masked) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nseq * topk) return;
    const int s = i / topk, ni = n_inliers[s];
    const bool l = ni < lost_inliers;
    masked[i] = l ? top_slot[i] : -1;
    if (i == s * topk) { lost[s] = l ? 1 : 0; track_inliers[s] = ni; }
}

/* The pair sequence s adopts: c = s * topk + best_rank[s] where the sequence is lost and the selection has an answer, else -1
 * (wave-uniform: one sequence per workgroup). *f = the winner's frame index s * cap + slot in the store. */
struct VoRecoverPick {
    const uint8_t* lost;            /* [nseq] */
    const int32_t *best_rank, *ix2; /* [nseq], [nseq * topk] */
    int topk;
};
__device__ __forceinline__ int recover_pair(const VoRecoverPick& W, int s, int* f) {
    const int r = W.lost[s] ? W.best_rank[s] : -1;
    const int c = r >= 0 && r < W.topk ? s * W.topk + r : -1;
    *f = c >= 0 ? W.ix2[c] : -1;
    return *f >= 0 ? c : -1;
}

struct VoRecoverWork {   /* the store's work buffers after tb_relocalize_batch_dev, pair-major at the store's pitch */
    const tb_match* matches;
    const tb_obs* obs;
    const uint8_t* outlier;
    const int32_t *mcounts, *flags, *ocounts, *ninl;
    const float* kf_mp;         /* the store's rings: [nseq][cap][pitch][3] */
    const uint8_t* kf_valid;
    const int32_t* kf_counts;
    const int32_t* best_kf;     /* [nseq] */
    const float* best_Tcw;      /* [nseq][16] */
};
struct VoRecoverState {  /* the loop's state of the current frame, [nseq][pitch] */
    float* Tcw;
    float* mp;
    uint8_t* valid;
    tb_obs* obs;
    uint8_t* outlier;
    tb_match* matches;
    int32_t *obs_counts, *n_inliers, *mcounts, *mflags, *recovered_kf;
};

/* Adopt (one workgroup per sequence): the winner's pose; the carried map points by k_reloc_rows' rule, which is
 * k_vo_match_carry's -- every key loses its point, then every match whose stored entry has a map point gives its query key that
 * point, the last such match in list order winning a key (win[], in LDS: one int per query key), so the points of the failed
 * tracking step are dropped and outlier rows keep theirs --; the pair's rows, outlier flags, inlier count and match list.
 * Every other sequence: recovered_kf -1 and nothing else. The loop's arrays and the store's share one pitch. */
__global__ void __launch_bounds__(256)
k_vo_recover_adopt(VoRecoverPick W, VoRecoverWork A, const int32_t* __restrict__ q_counts, int pitch, VoRecoverState D) {
    extern __shared__ int win[];   /* [pitch] */
    const int s = blockIdx.x, tid = threadIdx.x;
    int f;
    const int c = recover_pair(W, s, &f);
    if (c < 0) {
        if (tid == 0) D.recovered_kf[s] = -1;
        return;
    }
    const int n = min(max(q_counts[s], 0), pitch);
    const int nm = min(max(A.mcounts[c], 0), pitch);
    const int nk = min(max(A.kf_counts[f], 0), pitch);
    const int nr = min(max(A.ocounts[c], 0), pitch);
    const size_t o = (size_t)s * pitch, oc = (size_t)c * pitch, of = (size_t)f * pitch;
    const tb_match* M = A.matches + oc;
    for (int i = tid; i < n; i += 256) win[i] = -1;
    __syncthreads();
    for (int k = tid; k < nm; k += 256) {
        const int q = M[k].queryIdx, tr = M[k].trainIdx;
        if (q >= 0 && q < n && tr >= 0 && tr < nk && A.kf_valid[of + tr]) atomicMax(&win[q], k);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int k = win[i];
        float X = 0.f, Y = 0.f, Z = 0.f;
        if (k >= 0) {
            const size_t j = of + M[k].trainIdx;
            X = A.kf_mp[3 * j]; Y = A.kf_mp[3 * j + 1]; Z = A.kf_mp[3 * j + 2];
        }
        D.mp[3 * (o + i)] = X; D.mp[3 * (o + i) + 1] = Y; D.mp[3 * (o + i) + 2] = Z;
        D.valid[o + i] = k >= 0 ? 1 : 0;
    }
    kf_copy(D.obs + o, A.obs + oc, (size_t)nr * sizeof(tb_obs), tid);
    kf_copy(D.outlier + o, A.outlier + oc, (size_t)n, tid);
    kf_copy(D.matches + o, M, (size_t)nm * sizeof(tb_match), tid);
    if (tid < 16) D.Tcw[16 * (size_t)s + tid] = A.best_Tcw[16 * (size_t)s + tid];
    if (tid == 0) {
        D.obs_counts[s] = nr; D.n_inliers[s] = A.ninl[c];
        D.mcounts[s] = nm; D.mflags[s] = A.flags[c];
        D.recovered_kf[s] = A.best_kf[s];
    }
}

struct VoRecoverRings {  /* what a ring slot holds: the store, the ring-aligned database slot, the loop's word / node rings */
    const tb_keypoint* keys;
    const uint8_t* desc;
    const unsigned long long* fv;
    const float* mp;
    const uint8_t* valid;
    const int32_t *counts, *fv_counts;
    const int32_t* bv_word;
    const double* bv_val;
    const int32_t* bv_counts;
    const int32_t *word, *node;
    const int32_t* best_kf;
};
struct VoRecoverSnap {   /* the loop's keyframe snapshot, [nseq][pitch] */
    tb_keypoint* keys;
    uint8_t* desc;
    unsigned long long* fv;
    float* mp;
    uint8_t* valid;
    int32_t *counts, *fv_counts;
    int32_t* bv_word;
    double* bv_val;
    int32_t* bv_counts;
    int32_t *word, *node;
    int32_t* kf_ids;
};

/* Switch the tracking keyframe: workgroup (s, g) of an adopting sequence copies array group g of the winning ring slot into the
 * sequence's rows of the snapshot -- 0 the key records, 1 the descriptors, 2 the FeatureVector keys, 3 the map points, their
 * validity and the counts, 4 the BowVector, 5 the word and node ids -- as k_kf_store_add moved them in: live entries only, by
 * kf_copy's 16 / 4 / 1-byte lanes. Every other sequence: nothing. */
__global__ void __launch_bounds__(256)
k_vo_recover_switch(VoRecoverPick W, VoRecoverRings A, int pitch, VoRecoverSnap D) {
    const int s = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    int f;
    if (recover_pair(W, s, &f) < 0) return;
    const size_t n = (size_t)min(max(A.counts[f], 0), pitch);
    const size_t src = (size_t)f * pitch, dst = (size_t)s * pitch;
    if (g == 0) {
        kf_copy(D.keys + dst, A.keys + src, n * sizeof(tb_keypoint), tid);
    } else if (g == 1) {
        kf_copy(D.desc + 32 * dst, A.desc + 32 * src, n * 32, tid);
    } else if (g == 2) {
        const size_t nf = (size_t)min(max(A.fv_counts[f], 0), pitch);
        kf_copy(D.fv + dst, A.fv + src, nf * sizeof(unsigned long long), tid);
        if (tid == 0) D.fv_counts[s] = (int32_t)nf;
    } else if (g == 3) {
        kf_copy(D.mp + 3 * dst, A.mp + 3 * src, n * 3 * sizeof(float), tid);
        kf_copy(D.valid + dst, A.valid + src, n, tid);
        if (tid == 0) { D.counts[s] = (int32_t)n; D.kf_ids[s] = A.best_kf[s]; }
    } else if (g == 4) {
        const size_t nb = (size_t)min(max(A.bv_counts[f], 0), pitch);
        kf_copy(D.bv_word + dst, A.bv_word + src, nb * sizeof(int32_t), tid);
        kf_copy(D.bv_val + dst, A.bv_val + src, nb * sizeof(double), tid);
        if (tid == 0) D.bv_counts[s] = (int32_t)nb;
    } else {
        kf_copy(D.word + dst, A.word + src, n * sizeof(int32_t), tid);
        kf_copy(D.node + dst, A.node + src, n * sizeof(int32_t), tid);
    }
}

/* The loop's word / node rings at a keyframe step, beside the store add: workgroup (s, g) copies the snapshot's live word
 * (g = 0) or node (g = 1) ids of sequence s into ring slot `slot`. */
__global__ void __launch_bounds__(256)
k_vo_recover_ring_add(const int32_t* __restrict__ word, const int32_t* __restrict__ node, const int32_t* __restrict__ counts, int cap,
                      int pitch, int slot, int32_t* __restrict__ word_ring, int32_t* __restrict__ node_ring) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t n = (size_t)min(max(counts[s], 0), pitch);
    const size_t src = (size_t)s * pitch, dst = ((size_t)s * cap + slot) * pitch;
    if (blockIdx.y == 0) kf_copy(word_ring + dst, word + src, n * sizeof(int32_t), tid);
    else kf_copy(node_ring + dst, node + src, n * sizeof(int32_t), tid);
}

int tbk_kf_store_add(tb_ctx* ctx, int nseq, const tb_keypoint* d_keys, const uint8_t* d_desc, const int32_t* d_counts,
                     const unsigned long long* d_fv, const int32_t* d_fv_counts, const float* d_mp, const uint8_t* d_valid, int src_pitch,
                     const float* d_Tcw, int32_t kf_id, int cap, int pitch, int slot, tb_keypoint* s_keys, uint8_t* s_desc,
                     unsigned long long* s_fv, float* s_mp, uint8_t* s_valid, float* s_Tcw, int32_t* s_counts, int32_t* s_fv_counts,
                     int32_t* s_kf_ids) {
    KfStoreSrc A = {d_keys, d_desc, d_fv, d_mp, d_valid, d_Tcw, d_counts, d_fv_counts};
    KfStoreArrays D = {s_keys, s_desc, s_fv, s_mp, s_valid, s_Tcw, s_counts, s_fv_counts, s_kf_ids};
    return tb_launch(ctx, "k_kf_store_add", k_kf_store_add, dim3(nseq, 4), dim3(256), 0, A, src_pitch, cap, pitch, slot, kf_id, D);
}

int tbk_reloc_pairs(tb_ctx* ctx, int nseq, int ncand, int cap, const int32_t* d_cand_slot, const int32_t* d_kf_ids, const float* d_kf_Tcw,
                    int32_t* d_ix1, int32_t* d_ix2, float* d_seed, int32_t* d_cand_kf) {
    const int npairs = nseq * ncand;
    return tb_launch(ctx, "k_reloc_pairs", k_reloc_pairs, dim3((npairs + 255) / 256), dim3(256), 0, npairs, ncand, cap, d_cand_slot,
                     d_kf_ids, d_kf_Tcw, d_ix1, d_ix2, d_seed, d_cand_kf);
}

int tbk_reloc_rows(tb_ctx* ctx, int npairs, const tb_keypoint* d_q_keys, const int32_t* d_q_counts, int q_pitch, const int32_t* d_ix1,
                   const int32_t* d_ix2, const tb_match* d_matches, const int32_t* d_match_counts, const float* d_kf_mp,
                   const uint8_t* d_kf_valid, const int32_t* d_kf_counts, int pitch, const float* inv_sigma2, int nlevels, tb_obs* d_obs,
                   int32_t* d_obs_counts, uint8_t* d_outlier, int32_t* d_rows_out) {
    tb_reloc_sigma sig;
    sig.n = std::min(std::max(nlevels, 1), TB_MAX_LEVELS);
    for (int l = 0; l < TB_MAX_LEVELS; l++) sig.v[l] = l < sig.n ? inv_sigma2[l] : 1.f;
    return tb_launch(ctx, "k_reloc_rows", k_reloc_rows, dim3(npairs), dim3(256), (size_t)q_pitch * sizeof(int), d_q_keys, d_q_counts,
                     q_pitch, d_ix1, d_ix2, d_matches, d_match_counts, d_kf_mp, d_kf_valid, d_kf_counts, pitch, sig, d_obs,
                     d_obs_counts, d_outlier, d_rows_out);
}

int tbk_reloc_select(tb_ctx* ctx, int nseq, int ncand, int min_inliers, const int32_t* d_cand_kf, const int32_t* d_cand_inliers,
                     const float* d_cand_Tcw, int32_t* d_best_rank, int32_t* d_best_kf, float* d_best_Tcw) {
    return tb_launch(ctx, "k_reloc_select", k_reloc_select, dim3((nseq + 255) / 256), dim3(256), 0, nseq, ncand, min_inliers, d_cand_kf,
                     d_cand_inliers, d_cand_Tcw, d_best_rank, d_best_kf, d_best_Tcw);
}

int tbk_vo_recover_mask(tb_ctx* ctx, int nseq, int topk, int lost_inliers, const int32_t* d_n_inliers, const int32_t* d_top_slot,
                        uint8_t* d_lost, int32_t* d_track_inliers, int32_t* d_masked) {
    return tb_launch(ctx, "k_vo_recover_mask", k_vo_recover_mask, dim3((nseq * topk + 255) / 256), dim3(256), 0, nseq, topk, lost_inliers,
                     d_n_inliers, d_top_slot, d_lost, d_track_inliers, d_masked);
}

int tbk_vo_recover_adopt(tb_ctx* ctx, int nseq, const tb_vo_recover_args* a) {
    VoRecoverPick W = {a->lost, a->best_rank, a->ix2, a->topk};
    VoRecoverWork A = {a->w_matches, a->w_obs, a->w_outlier, a->w_mcounts, a->w_flags, a->w_ocounts, a->w_ninl, a->s_mp, a->s_valid,
                       a->s_counts, a->best_kf, a->best_Tcw};
    VoRecoverState D = {a->Tcw, a->mp, a->valid, a->obs, a->outlier, a->matches, a->obs_counts, a->n_inliers, a->mcounts, a->mflags,
                        a->recovered_kf};
    return tb_launch(ctx, "k_vo_recover_adopt", k_vo_recover_adopt, dim3(nseq), dim3(256), (size_t)a->pitch * sizeof(int), W, A,
                     a->orb_counts, a->pitch, D);
}

int tbk_vo_recover_switch(tb_ctx* ctx, int nseq, const tb_vo_recover_args* a) {
    VoRecoverPick W = {a->lost, a->best_rank, a->ix2, a->topk};
    VoRecoverRings A = {a->s_keys, a->s_desc, a->s_fv, a->s_mp, a->s_valid, a->s_counts, a->s_fv_counts, a->db_words, a->db_values,
                        a->db_counts, a->word_ring, a->node_ring, a->best_kf};
    VoRecoverSnap D = {a->kf_orb, a->kf_desc, a->kf_fv, a->kf_mp, a->kf_valid, a->kf_cnt, a->kf_fv_cnt, a->kf_bv_word, a->kf_bv_val,
                       a->kf_bv_cnt, a->kf_word, a->kf_node, a->kf_ids};
    return tb_launch(ctx, "k_vo_recover_switch", k_vo_recover_switch, dim3(nseq, 6), dim3(256), 0, W, A, a->pitch, D);
}

int tbk_vo_recover_ring_add(tb_ctx* ctx, int nseq, const int32_t* d_word, const int32_t* d_node, const int32_t* d_counts, int cap, int pitch,
                            int slot, int32_t* d_word_ring, int32_t* d_node_ring) {
    return tb_launch(ctx, "k_vo_recover_ring_add", k_vo_recover_ring_add, dim3(nseq, 2), dim3(256), 0, d_word, d_node, d_counts, cap, pitch,
                     slot, d_word_ring, d_node_ring);
}
