/* Scoring BowVectors and the per-sequence keyframe database (see include/tb_capi.h, tb_bow_score_batch_dev / tb_bow_db_*).
 *
 * TemplatedVocabulary::score (third_part/DBoW2/DBoW2/TemplatedVocabulary.h:156-162, :1199-1203) forwards to the vocabulary's
 * scoring object, ScoringObject.cpp:23-311: a walk over two vectors sorted by word id that adds one term per common word (KL:
 * per word of v1) into ONE accumulator, in ascending word order, and a closing formula. The values are doubles and come out bit
 * for bit for the five scorings made of + - * / sqrt fabs (the library is built with -ffp-contract=off: one rounding per
 * statement), so the terms are computed in parallel and added serially, in word order -- never by a tree or per-lane partial
 * sums, which would reorder the sum. KL's log is the device library's; its order is the same. */
#include <algorithm>
#include <cmath>

#include "tb_device.h"

struct BowScoreArgs {
    const int32_t* aw; const double* av; const int32_t* ac; int a_pitch;   /* v1, the queries: [na][a_pitch], counts [na] */
    const int32_t* bw; const double* bv; const int32_t* bc; int b_pitch;   /* v2, the entries */
    int nj;          /* entries per query: query i meets entries i * bq + j, j in [0, nj), and writes out[i * nj + j] */
    int bq;          /* 1 with nj = 1: pairwise; 0: all pairs; nj: query i has its own ring of nj entries */
    int epb;         /* entries per workgroup (gridDim.y * epb >= nj) */
    int scoring;
    double log_eps;  /* GeneralScoring::LOG_EPS = log(DBL_EPSILON), ScoringObject.cpp:18, computed on the host */
    int ring;        /* != 0: the entries are ring slots; an empty or excluded slot is not scored, its out is a quiet NaN */
    int nfilled, newest, exclude;   /* slots in use, the slot of the last add, how many of the newest adds to leave out */
    double* out;
};

/* first index of w[0, n) that is >= key (std::map::lower_bound on the sorted list) */
template <typename P>
__device__ __forceinline__ int tb_lower_bound(P w, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (w[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* acc + the terms of the lanes in mask, one add per term, ascending lane = ascending word. mask is the wave's ballot, so the
 * loop is uniform and every lane carries the same accumulator. */
__device__ __forceinline__ double tb_add_in_lane_order(double acc, double term, unsigned long long mask) {
    while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        const int lo = __builtin_amdgcn_readlane(__double2loint(term), l), hi = __builtin_amdgcn_readlane(__double2hiint(term), l);
        acc = acc + __hiloint2double(hi, lo);
        mask &= mask - 1;
    }
    return acc;
}

/* is ring slot j of a ring with nfilled slots in use, whose last add went to slot newest, left out of a query? */
__device__ __forceinline__ bool tb_ring_skipped(int j, int cap, int nfilled, int newest, int exclude) {
    if (j >= nfilled) return true;
    const int age = (newest - j + cap) % cap;   /* 0 = the last add */
    return age < exclude;
}

/* One workgroup = one query vector (v1) staged in LDS, count entries of it, and up to epb entries (v2); each wavefront takes
 * entries in turn. For the five symmetric-walk scorings (ScoringObject.cpp:23-170, :226-311) a term exists per COMMON word, so
 * the lanes walk v2 in chunks of 64 (coalesced global loads) and binary-search v1 in LDS; KL (:175-221) adds a term per word of
 * v1, so there the lanes walk v1 in LDS and binary-search v2 in global memory. Either way the chunk's terms are in ascending
 * word order across the lanes and are added in that order. No barrier inside the per-entry loop, no atomics. */
__global__ void __launch_bounds__(256)
k_bow_score(BowScoreArgs A) {
    extern __shared__ __attribute__((aligned(16))) double s_val[];   /* [a_pitch] values, then [a_pitch] words */
    int32_t* s_word = reinterpret_cast<int32_t*>(s_val + A.a_pitch);
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = min(max(A.ac[i], 0), A.a_pitch);
    const size_t abase = (size_t)i * A.a_pitch;
    for (int t = tid; t < na; t += 256) { s_val[t] = A.av[abase + t]; s_word[t] = A.aw[abase + t]; }
    __syncthreads();
    const int j0 = blockIdx.y * A.epb, j1 = min(j0 + A.epb, A.nj);
    const int scoring = A.scoring;
    for (int j = j0 + wave; j < j1; j += 4) {
        const size_t o = (size_t)i * A.nj + j;
        if (A.ring && tb_ring_skipped(j, A.nj, A.nfilled, A.newest, A.exclude)) {
            if (lane == 0) A.out[o] = __longlong_as_double(0x7ff8000000000000ll);
            continue;
        }
        const size_t e = (size_t)i * A.bq + j;
        const int nb = min(max(A.bc[e], 0), A.b_pitch);
        const int32_t* __restrict__ bw = A.bw + e * A.b_pitch;
        const double* __restrict__ bv = A.bv + e * A.b_pitch;
        double score = 0.0;
        if (scoring == 3) {
            /* KLScoring::score: v1 is the query. A word of v1 that v2 has: vi * log(vi / wi) when both are non-zero (:195); one
             * that lies before some word of v2: vi * (log(vi) - LOG_EPS), unconditionally (:204); one past v2's last word, the
             * tail: the same when vi != 0 (:216-218) */
            for (int base = 0; base < na; base += 64) {
                const int q = base + lane;
                const bool have = q < na;
                const int w = have ? s_word[q] : 0;
                const double vi = have ? s_val[q] : 1.0;
                const int pos = have ? tb_lower_bound(bw, nb, w) : nb;
                const bool tail = pos >= nb;
                const bool common = !tail && bw[pos] == w;
                const double wi = common ? bv[pos] : 1.0;
                bool adds;
                double term;
                if (common) {
                    adds = vi != 0 && wi != 0;
                    const double r = vi / wi;
                    const double l = log(r);
                    term = vi * l;
                } else {
                    adds = !tail || vi != 0;
                    const double l = log(vi);
                    const double d = l - A.log_eps;
                    term = vi * d;
                }
                score = tb_add_in_lane_order(score, term, __ballot(have && adds));
            }
        } else {
            for (int base = 0; base < nb; base += 64) {
                const int q = base + lane;
                const bool have = q < nb;
                const int w = have ? bw[q] : 0;
                const double wi = have ? bv[q] : 0.0;
                const int pos = have ? tb_lower_bound(s_word, na, w) : na;
                const bool common = have && pos < na && s_word[pos] == w;
                const double vi = common ? s_val[pos] : 0.0;
                bool adds = common;
                double term;
                if (scoring == 0) {            /* L1Scoring :41 */
                    const double d = fabs(vi - wi);
                    const double d1 = d - fabs(vi);
                    term = d1 - fabs(wi);
                } else if (scoring == 2) {     /* ChiSquareScoring :148 */
                    const double sum = vi + wi;
                    adds = common && sum != 0.0;
                    const double p = vi * wi;
                    term = p / (adds ? sum : 1.0);
                } else if (scoring == 4) {     /* BhattacharyyaScoring :245 */
                    const double p = vi * wi;
                    term = sqrt(p);
                } else {                       /* L2Scoring :91, DotProductScoring :290 */
                    term = vi * wi;
                }
                score = tb_add_in_lane_order(score, term, __ballot(adds));
            }
            if (scoring == 0) {
                score = -score / 2.0;                                   /* :65 */
            } else if (scoring == 1) {
                if (score >= 1) score = 1.0;                            /* :114 */
                else { const double r = 1.0 - score; score = 1.0 - sqrt(r); }   /* :117 */
            } else if (scoring == 2) {
                score = 2. * score;                                     /* :167 */
            }
        }
        if (lane == 0) A.out[o] = score;
    }
}

/* One add of the database: sequence s's vector (src [nseq][src_pitch], its count clamped to the ring's pitch) into ring slot
 * `slot` of words / values [nseq][cap][pitch], with its count and keyframe id. */
__global__ void __launch_bounds__(256)
k_bow_db_add(const int32_t* __restrict__ src_w, const double* __restrict__ src_v, const int32_t* __restrict__ src_c, int src_pitch,
             int cap, int pitch, int slot, int32_t kf_id, int32_t* __restrict__ words, double* __restrict__ values,
             int32_t* __restrict__ counts, int32_t* __restrict__ kf_ids) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(src_c[s], 0), min(src_pitch, pitch));
    const size_t src = (size_t)s * src_pitch, dst = ((size_t)s * cap + slot) * pitch;
    for (int t = tid; t < n; t += 256) { words[dst + t] = src_w[src + t]; values[dst + t] = src_v[src + t]; }
    if (tid == 0) { counts[(size_t)s * cap + slot] = n; kf_ids[(size_t)s * cap + slot] = kf_id; }
}

/* Ranking by counting, one workgroup per sequence: the rank of a ranked slot is the number of ranked slots that are strictly
 * better -- a higher score (KL: a lower one), then the lower kf_id, then the lower slot; a NaN score is worse than any number.
 * The ranks are a permutation of 0 .. nranked - 1, so every top row is written exactly once; deterministic, no sort. */
__global__ void __launch_bounds__(256)
k_bow_db_rank(const double* __restrict__ scores, const int32_t* __restrict__ kf_ids, int cap, int nfilled, int newest, int exclude,
              int nranked, int ascending, int topk, int32_t* __restrict__ top_slot, int32_t* __restrict__ top_kf,
              double* __restrict__ top_score, int32_t* __restrict__ top_count) {
    __shared__ double s_sc[1024];
    __shared__ int32_t s_kf[1024];
    __shared__ uint8_t s_ok[1024];
    const int s = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)s * cap;
    for (int j = tid; j < cap; j += 256) {
        s_sc[j] = scores[base + j];
        s_kf[j] = kf_ids[base + j];
        s_ok[j] = tb_ring_skipped(j, cap, nfilled, newest, exclude) ? 0 : 1;
    }
    __syncthreads();
    for (int j = tid; j < cap; j += 256) {
        if (!s_ok[j]) continue;
        const double sj = s_sc[j];
        const int kj = s_kf[j];
        const bool nanj = sj != sj;
        int rank = 0;
        for (int k = 0; k < cap; k++) {
            if (!s_ok[k] || k == j) continue;
            const double sk = s_sc[k];
            const bool nank = sk != sk;
            bool better, tie;
            if (nank || nanj) { better = nanj && !nank; tie = nanj && nank; }
            else { better = ascending ? sk < sj : sk > sj; tie = sk == sj; }
            if (tie) better = s_kf[k] < kj || (s_kf[k] == kj && k < j);
            rank += better ? 1 : 0;
        }
        if (rank < topk) {
            const size_t r = (size_t)s * topk + rank;
            top_slot[r] = j; top_kf[r] = kj; top_score[r] = sj;
        }
    }
    for (int r = max(nranked, 0) + tid; r < topk; r += 256) {
        const size_t q = (size_t)s * topk + r;
        top_slot[q] = -1; top_kf[q] = -1; top_score[q] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (tid == 0 && top_count) top_count[s] = min(topk, max(nranked, 0));
}

/* ring != 0: nj is the ring's capacity and (nfilled, newest, exclude) say which slots are left out */
int tbk_bow_score(tb_ctx* ctx, int scoring, double log_eps, int na, const int32_t* d_aw, const double* d_av, const int32_t* d_ac, int a_pitch,
                  const int32_t* d_bw, const double* d_bv, const int32_t* d_bc, int b_pitch, int nj, int bq, int ring, int nfilled,
                  int newest, int exclude, double* d_out) {
    if (na <= 0 || nj <= 0) return TB_OK;
    BowScoreArgs A;
    A.aw = d_aw; A.av = d_av; A.ac = d_ac; A.a_pitch = a_pitch; A.bw = d_bw; A.bv = d_bv; A.bc = d_bc; A.b_pitch = b_pitch;
    A.nj = nj; A.bq = bq; A.scoring = scoring; A.log_eps = log_eps; A.ring = ring; A.nfilled = nfilled; A.newest = newest;
    A.exclude = exclude; A.out = d_out;
    /* a workgroup stages its query once and scores epb entries with 4 wavefronts: enough workgroups to fill the device twice
     * over where the batch allows it, at least one entry per wavefront, and a grid the launch accepts */
    const long long pairs = (long long)na * nj;
    long long per = (pairs + 2LL * ctx->num_cu - 1) / (2LL * ctx->num_cu);
    per = std::min<long long>(std::max<long long>((per + 3) / 4 * 4, 4), 64);
    per = std::max<long long>(per, ((long long)nj + 65534) / 65535);
    A.epb = (int)per;
    const size_t lds = (size_t)a_pitch * (sizeof(double) + sizeof(int32_t));
    TB_TRY(tb_lds_limit(ctx, (const void*)k_bow_score, lds));
    return tb_launch(ctx, "k_bow_score", k_bow_score, dim3(na, (nj + A.epb - 1) / A.epb), dim3(256), lds, A);
}

int tbk_bow_db_add(tb_ctx* ctx, int nseq, const int32_t* d_src_w, const double* d_src_v, const int32_t* d_src_c, int src_pitch, int cap,
                   int pitch, int slot, int32_t kf_id, int32_t* d_words, double* d_values, int32_t* d_counts, int32_t* d_kf_ids) {
    return tb_launch(ctx, "k_bow_db_add", k_bow_db_add, dim3(nseq), dim3(256), 0, d_src_w, d_src_v, d_src_c, src_pitch, cap, pitch, slot,
                     kf_id, d_words, d_values, d_counts, d_kf_ids);
}

int tbk_bow_db_rank(tb_ctx* ctx, int nseq, const double* d_scores, const int32_t* d_kf_ids, int cap, int nfilled, int newest, int exclude,
                    int ascending, int topk, int32_t* d_top_slot, int32_t* d_top_kf, double* d_top_score, int32_t* d_top_count) {
    const int nranked = nfilled - std::min(exclude, nfilled);
    return tb_launch(ctx, "k_bow_db_rank", k_bow_db_rank, dim3(nseq), dim3(256), 0, d_scores, d_kf_ids, cap, nfilled, newest, exclude,
                     nranked, ascending, topk, d_top_slot, d_top_kf, d_top_score, d_top_count);
}
