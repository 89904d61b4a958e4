/* a12 / a13 / a14 -- Hamming matchers.
 *
 * a12 Matcher::searchByBF (src/matchers/matcher.cpp:168-228) = cv::BFMatcher(NORM_HAMMING,
 *     crossCheck=true).match + "d < fmin(ratio*d_min, minTh)" filter.  OpenCV 3.3 cross-check semantics
 *     (batchDistance, restated): every TRAIN row takes its nearest query (first index on ties); a query
 *     keeps the train with the smallest such distance (first train on ties).  Both "first on ties"
 *     rules are an integer minimum over the packed word (distance << 32 | index), so the whole thing is
 *     two rounds of 64-bit atomicMin -- order independent, bit exact.
 * a13 Matcher::DescriptorDistance (:793-808): 256-bit Hamming = 4 x (xor64 + popcount64).
 * a14 Matcher::searchByViolence (:299-395): per F1 key, best / second-best over the 120x36 lookup grid
 *     window of F2 (Frame.cpp:202-255), traversal order (ix, iy, insertion) preserved per thread.
 *
 * Bound: not HBM -- a 2000 x 2000 pair is 4e6 Hamming-256 on 128 KB of descriptors that sit in LDS / L2. The
 * nearest-neighbour pass runs on the i8 matrix cores (k_bf_nn_mfma: the distances as an integer matrix product, 32 256
 * v_mfma_i32_32x32x32_i8 per 2000 x 2000 pair; beside them the vector ALU forms the keys, takes the minima and expands candidate bits to
 * bytes -- DESIGN.md 4e has the budget and what was measured). The scalar kernel (k_bf_nn: v_xor + v_bcnt, integer VALU
 * bound) serves sets narrower than a tile and index fields wider than 16 bits, and is the yardstick behind tb_debug_bf_scalar.
 */
#include "tb_internal.h"
#include "tb_device.h"

#define BF_T 256
#define BF_QC 512 /* queries staged per block */

struct Desc256 { unsigned long long w[4]; };

__device__ __forceinline__ int bf_dist(const Desc256& a, const unsigned long long* __restrict__ q) {
    return __popcll(a.w[0] ^ q[0]) + __popcll(a.w[1] ^ q[1]) + __popcll(a.w[2] ^ q[2]) + __popcll(a.w[3] ^ q[3]);
}

/* For every "row" descriptor (one per thread) the nearest "col" descriptor of a staged chunk:
 * rbest[pair][row] = min(dist << 32 | col). grid (row tiles, col chunks, pairs). */
__global__ void __launch_bounds__(BF_T)
k_bf_nn(const uint8_t* __restrict__ rows, const int32_t* __restrict__ rowCounts, const uint8_t* __restrict__ cols,
        const int32_t* __restrict__ colCounts, size_t set_pitch, int max_n, unsigned long long* __restrict__ rbest) {
    __shared__ __attribute__((aligned(16))) unsigned long long q[BF_QC * 4];
    const int p = blockIdx.z;
    const int nr = min(rowCounts[p], max_n), nc = min(colCounts[p], max_n);
    const int c0 = blockIdx.y * BF_QC;
    if (c0 >= nc || (int)(blockIdx.x * BF_T) >= nr) return;
    const int cn = min(BF_QC, nc - c0);
    const unsigned long long* csrc = reinterpret_cast<const unsigned long long*>(cols + (size_t)p * set_pitch) + (size_t)c0 * 4;
    for (int i = threadIdx.x; i < cn * 4; i += BF_T) q[i] = csrc[i];
    __syncthreads();
    const int r = blockIdx.x * BF_T + threadIdx.x;
    if (r >= nr) return;
    const unsigned long long* rsrc = reinterpret_cast<const unsigned long long*>(rows + (size_t)p * set_pitch) + (size_t)r * 4;
    Desc256 d;
    d.w[0] = rsrc[0]; d.w[1] = rsrc[1]; d.w[2] = rsrc[2]; d.w[3] = rsrc[3];
    int best = 0x7fffffff, bi = 0;
    for (int c = 0; c < cn; c++) {
        const int dist = bf_dist(d, q + 4 * c);
        if (dist < best) { best = dist; bi = c; }
    }
    atomicMin(&rbest[(size_t)p * max_n + r], ((unsigned long long)best << 32) | (unsigned)(c0 + bi));
}

/* The same nearest neighbour as an i8 matrix product. A candidate's bits as bytes {0, 1} and a row's bits as bytes
 * {+1 for a 0 bit, -1 for a 1 bit} give Hamming(row, cand) = popcount(row) + D, D = sum_k cand[k] * row[k]: popcount(row) is
 * constant per row, so the argmin is D's and the popcount is added once at the end.
 *
 * v_mfma_i32_32x32x32_i8, candidates = A (tile rows), rows = B (tile columns): the 32x32 C/D map puts the column on lane & 31
 * and the 16 results of a lane on tile rows (i & 3) + 8 (i >> 2) + 4 (lane >> 5), so a lane keeps the running minimum of ITS row
 * over its 16 registers and only the two lane halves of a row meet, once, at the end. A and B hold the same (lane >> 5, byte)
 * -> k assignment whatever it is, and a sum over k does not care about its order: k-step s takes 32-bit word s of the
 * descriptor, lane half h its 16-bit half h, byte j its bit j -- on both sides.
 *
 * key = (D << 16) + candidate, compared as signed: the smallest distance, the first index on ties -- the rule of the
 * (dist << 32 | index) atomicMin above. D is in [-256, 256] and the index field holds max_n <= 65535.
 *
 * A workgroup is 4 wavefronts x 64 rows: a wavefront keeps its rows' two B fragments (8 k-steps x 4 VGPRs each) in registers
 * for the whole sweep, and every ds_read_b128 of a candidate fragment feeds two MFMAs. The workgroup expands the candidates
 * from bits to bytes into LDS, BFM_CH at a time, as ex[k-step][candidate][32 bytes]: the 64 lanes of a fragment read are
 * 1 KB of consecutive bytes. Candidates past nc are zero bytes in LDS and take a key that never wins.
 *
 * grid (row blocks, candidate splits, pairs): with plain != 0 (one split) a row's result is stored, all ones where the row has
 * no candidate, and rbest needs no fill; otherwise the splits of a row meet in the atomicMin on a filled rbest. */
#define BFM_T 256
#define BFM_ROWS 256       /* rows per workgroup: 64 per wavefront */
#define BFM_CH 128         /* candidates per LDS chunk: 8 k-steps x 128 x 32 B = 32 KB */
#define BFM_MIN_N 32       /* below one tile of candidates the scalar kernel runs */
#define BFM_MAX_N 65535    /* the key's index field */

typedef int bfm_i4 __attribute__((ext_vector_type(4)));
typedef int bfm_i16 __attribute__((ext_vector_type(16)));

/* bits 4n .. 4n + 3 of w as four bytes {0, 1}: x + (x << 7) + (x << 14) + (x << 21) puts bit b of the nibble on bit 8b */
__device__ __forceinline__ unsigned bfm_expand4(unsigned w, int n) { return __umul24((w >> (4 * n)) & 0xfu, 0x204081u) & 0x01010101u; }

/* the smallest key of one tile's 16 results per lane; the tile's candidate base is not in it */
__device__ __forceinline__ int bfm_tile_min(const bfm_i16& acc) {
    int m = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 16; i++) m = min(m, (int)(((unsigned)acc[i] << 16) + (unsigned)((i & 3) + 8 * (i >> 2))));
    return m;
}
/* the same for a tile that reaches past nc: base = index of the lane's first candidate */
__device__ __forceinline__ int bfm_tile_min_edge(const bfm_i16& acc, int base, int nc) {
    int m = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int off = (i & 3) + 8 * (i >> 2);
        if (base + off < nc) m = min(m, (int)(((unsigned)acc[i] << 16) + (unsigned)off));
    }
    return m;
}

__global__ void __launch_bounds__(BFM_T, 2)   /* two wavefronts per SIMD: 256 registers, so the MFMAs take VGPR accumulators */
k_bf_nn_mfma(const uint8_t* __restrict__ rows, const int32_t* __restrict__ rowCounts, const uint8_t* __restrict__ cols,
             const int32_t* __restrict__ colCounts, size_t set_pitch, int max_n, unsigned long long* __restrict__ rbest, int plain) {
    __shared__ __attribute__((aligned(16))) unsigned ex[8 * BFM_CH * 8];
    const int p = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr = min(rowCounts[p], max_n), nc = min(colCounts[p], max_n);
    const int r0 = blockIdx.x * BFM_ROWS;
    if (r0 >= nr) return;   /* block-uniform */
    const int n = lane & 31, h = lane >> 5;
    const int wr0 = r0 + wave * 64;
    const bool wave_live = wr0 < nr;   /* a wavefront past the set still expands candidates */

    /* the rows' +-1 fragments: lane (n, h) holds bits 32 s + 16 h .. + 15 of row g * 32 + n in b[g][s] */
    bfm_i4 b[2][8];
    int pop[2];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const int r = wr0 + g * 32 + n;
        unsigned w[8];
#pragma unroll
        for (int s = 0; s < 8; s++) w[s] = 0;
        if (r < nr) {
            const unsigned long long* rsrc = reinterpret_cast<const unsigned long long*>(rows + (size_t)p * set_pitch) + (size_t)r * 4;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned long long v = rsrc[j];
                w[2 * j] = (unsigned)v; w[2 * j + 1] = (unsigned)(v >> 32);
            }
        }
        int pc = 0;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            pc += __popc(w[s]);
            const unsigned hw = (w[s] >> (16 * h)) & 0xffffu;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned e = bfm_expand4(hw, j);
                b[g][s][j] = (int)(((e << 8) - e) | 0x01010101u);   /* byte 1 -> 0xff, byte 0 -> 0x01 */
            }
        }
        pop[g] = pc;
    }

    int best0 = 0x7fffffff, best1 = 0x7fffffff;
    const unsigned long long* csrc = reinterpret_cast<const unsigned long long*>(cols + (size_t)p * set_pitch);
    const int nchunks = (nc + BFM_CH - 1) / BFM_CH;
    /* thread (ec, eq) expands words 4 eq .. 4 eq + 3 of candidate c0 + ec; the words of the next chunk are loaded a chunk ahead */
    const int ec = tid & (BFM_CH - 1), eq = tid >> 7;
    unsigned long long v0 = 0, v1 = 0;
    if ((int)blockIdx.y < nchunks && (int)blockIdx.y * BFM_CH + ec < nc) {
        const unsigned long long* src = csrc + (size_t)(blockIdx.y * BFM_CH + ec) * 4 + eq * 2;
        v0 = src[0]; v1 = src[1];
    }
    for (int ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
        const int c0 = ch * BFM_CH;
        __syncthreads();   /* the last chunk's readers are done */
        {
            const int c = ec, q = eq;
            const unsigned w4[4] = {(unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32)};
            v0 = v1 = 0;
            const int cnext = (ch + (int)gridDim.y) * BFM_CH + ec;   /* past nc after the last chunk */
            if (cnext < nc) {
                const unsigned long long* src = csrc + (size_t)cnext * 4 + eq * 2;
                v0 = src[0]; v1 = src[1];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4* dst = reinterpret_cast<uint4*>(&ex[((4 * q + j) * BFM_CH + c) * 8]);
                dst[0] = make_uint4(bfm_expand4(w4[j], 0), bfm_expand4(w4[j], 1), bfm_expand4(w4[j], 2), bfm_expand4(w4[j], 3));
                dst[1] = make_uint4(bfm_expand4(w4[j], 4), bfm_expand4(w4[j], 5), bfm_expand4(w4[j], 6), bfm_expand4(w4[j], 7));
            }
        }
        __syncthreads();
        if (!wave_live) continue;   /* wavefront-uniform; the barriers above are met by every wavefront */
        if (c0 + BFM_CH <= nc) {
            /* a full chunk, unrolled: the keys and minimum of tile t - 1 (vector ALU, two registers of each accumulator per
             * k-step) are issued under the MFMAs of tile t, which write the other pair of accumulators */
            bfm_i16 acc[2][2];
#pragma unroll
            for (int t = 0; t <= BFM_CH / 32; t++) {
                int m0 = 0x7fffffff, m1 = 0x7fffffff;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    if (t < BFM_CH / 32) {
                        const bfm_i4 a = *reinterpret_cast<const bfm_i4*>(&ex[(s * BFM_CH + t * 32 + n) * 8 + h * 4]);
                        if (s == 0) {
#pragma unroll
                            for (int i = 0; i < 16; i++) { acc[t & 1][0][i] = 0; acc[t & 1][1][i] = 0; }
                        }
                        acc[t & 1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[0][s], acc[t & 1][0], 0, 0, 0);
                        acc[t & 1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[1][s], acc[t & 1][1], 0, 0, 0);
                    }
                    if (t > 0) {
                        const bfm_i16 &p0 = acc[(t - 1) & 1][0], &p1 = acc[(t - 1) & 1][1];
                        const int i = 2 * s, j = 2 * s + 1;
                        const unsigned oi = (i & 3) + 8 * (i >> 2), oj = (j & 3) + 8 * (j >> 2);
                        m0 = min(m0, min((int)(((unsigned)p0[i] << 16) + oi), (int)(((unsigned)p0[j] << 16) + oj)));
                        m1 = min(m1, min((int)(((unsigned)p1[i] << 16) + oi), (int)(((unsigned)p1[j] << 16) + oj)));
                    }
                }
                if (t > 0) {
                    const int base = c0 + (t - 1) * 32 + 4 * h;
                    best0 = min(best0, m0 + base);
                    best1 = min(best1, m1 + base);
                }
            }
            continue;
        }
        const int ntile = min(BFM_CH / 32, (nc - c0 + 31) >> 5);
        for (int t = 0; t < ntile; t++) {
            bfm_i16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; i++) { acc0[i] = 0; acc1[i] = 0; }
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const bfm_i4 a = *reinterpret_cast<const bfm_i4*>(&ex[(s * BFM_CH + t * 32 + n) * 8 + h * 4]);
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[0][s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[1][s], acc1, 0, 0, 0);
            }
            const int base = c0 + t * 32 + 4 * h;
            if (c0 + t * 32 + 32 <= nc) {   /* wavefront-uniform */
                best0 = min(best0, bfm_tile_min(acc0) + base);
                best1 = min(best1, bfm_tile_min(acc1) + base);
            } else {
                const int m0 = bfm_tile_min_edge(acc0, base, nc), m1 = bfm_tile_min_edge(acc1, base, nc);
                if (m0 != 0x7fffffff) best0 = min(best0, m0 + base);
                if (m1 != 0x7fffffff) best1 = min(best1, m1 + base);
            }
        }
    }

    /* the two lane halves of a row saw different candidates */
    best0 = min(best0, __shfl_xor(best0, 32));
    best1 = min(best1, __shfl_xor(best1, 32));
    if (h == 0) {
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int r = wr0 + g * 32 + n, k = g ? best1 : best0;
            if (r >= nr) continue;
            unsigned long long v = ~0ull;
            if (k != 0x7fffffff) v = ((unsigned long long)(unsigned)((k >> 16) + pop[g]) << 32) | (unsigned)(k & 0xffff);
            if (plain) rbest[(size_t)p * max_n + r] = v;
            else if (k != 0x7fffffff) atomicMin(&rbest[(size_t)p * max_n + r], v);
        }
    }
}

/* cross-check: train t -> its nearest query q; qbest[q] = min(dist << 32 | t) */
__global__ void __launch_bounds__(BF_T)
k_bf_cross(const int32_t* __restrict__ trainCounts, int max_n, const unsigned long long* __restrict__ tbest,
           unsigned long long* __restrict__ qbest) {
    const int p = blockIdx.y, t = blockIdx.x * BF_T + threadIdx.x;
    if (t >= min(trainCounts[p], max_n)) return;
    const unsigned long long v = tbest[(size_t)p * max_n + t];
    if (v == ~0ull) return;
    const unsigned q = (unsigned)v;
    atomicMin(&qbest[(size_t)p * max_n + q], (v & 0xffffffff00000000ull) | (unsigned)t);
}

/* one block per pair: d_min, filter, compaction in query order (searchByBF :209-218) */
__global__ void __launch_bounds__(BF_T)
k_bf_finalize(const int32_t* __restrict__ queryCounts, int max_n, const unsigned long long* __restrict__ qbest, int filter,
              float ratio, float min_th, tb_match* __restrict__ out, int cap, int32_t* __restrict__ outCounts) {
    __shared__ int wsum[4];
    __shared__ int s_min;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int nq = min(queryCounts[p], max_n);
    const unsigned long long* qb = qbest + (size_t)p * max_n;
    if (tid == 0) s_min = 0x7fffffff;
    __syncthreads();
    int mn = 0x7fffffff;
    for (int qi = tid; qi < nq; qi += BF_T) {
        const unsigned long long v = qb[qi];
        if (v != ~0ull) mn = min(mn, (int)(v >> 32));
    }
    atomicMin(&s_min, mn);
    __syncthreads();
    float lim = 3.0e38f;
    if (filter) lim = fminf(TB_FMUL(ratio, (float)s_min), min_th);
    tb_match* o = out + (size_t)p * cap;
    int running = 0;
    for (int q0 = 0; q0 < nq; q0 += BF_T) {
        const int qi = q0 + tid;
        unsigned long long v = ~0ull;
        if (qi < nq) v = qb[qi];
        const float dist = (float)(int)(v >> 32);
        const bool f = v != ~0ull && (!filter || dist < lim);
        const int slot = tb_block_ordered_slot(f, running, wsum);
        if (f && slot < cap) {
            tb_match m;
            m.queryIdx = qi; m.trainIdx = (int)(unsigned)v; m.imgIdx = 0; m.distance = dist;
            o[slot] = m;
        }
    }
    if (tid == 0) outCounts[p] = running; /* may exceed cap: the host reports TB_ECAPACITY */
}

int tbk_bf_batch(tb_ctx* ctx, int npairs, const uint8_t* d1, const int32_t* c1, const uint8_t* d2, const int32_t* c2,
                 size_t set_pitch, int max_n, int crosscheck, int filter, float ratio, float min_th, tb_match* out, int cap,
                 int32_t* out_counts, unsigned long long* d_tbest, unsigned long long* d_qbest) {
    if (npairs <= 0 || max_n <= 0) return TB_OK;
    const size_t bytes = (size_t)npairs * max_n * sizeof(unsigned long long);
    /* the matrix-core kernel unless the sets are narrower than a tile, the key's index field is too narrow, or the test hook
     * (tb_debug_bf_scalar) asks for the scalar one. Candidate chunks side by side only while the row blocks alone leave
     * compute units idle; with one split the kernel stores and its output needs no fill. */
    const bool mfma = !ctx->dbg_bf_scalar && max_n >= BFM_MIN_N && max_n <= BFM_MAX_N;
    const int tiles = (max_n + BFM_ROWS - 1) / BFM_ROWS, chunks = (max_n + BFM_CH - 1) / BFM_CH;
    int split = 1;
    while (split * 2 <= chunks && (long long)tiles * npairs * split < 2ll * ctx->num_cu) split *= 2;
    const int plain = mfma && split == 1;
    const dim3 grid((max_n + BF_T - 1) / BF_T, (max_n + BF_QC - 1) / BF_QC, npairs), mgrid(tiles, split, npairs);
    /* rows = train (d2), cols = query (d1) with the cross-check; else rows = query, cols = train: qbest[q] = (dist, nearest
     * train) directly */
    const uint8_t *rows = crosscheck ? d2 : d1, *cols = crosscheck ? d1 : d2;
    const int32_t *rc = crosscheck ? c2 : c1, *cc = crosscheck ? c1 : c2;
    unsigned long long* rbest = crosscheck ? d_tbest : d_qbest;
    TB_HIP(ctx, hipMemsetAsync(d_qbest, 0xff, bytes, ctx->stream));
    if (crosscheck && !plain) TB_HIP(ctx, hipMemsetAsync(d_tbest, 0xff, bytes, ctx->stream));
    if (mfma) TB_TRY(tb_launch(ctx, "k_bf_nn", k_bf_nn_mfma, mgrid, dim3(BFM_T), 0, rows, rc, cols, cc, set_pitch, max_n, rbest, plain));
    else TB_TRY(tb_launch(ctx, "k_bf_nn", k_bf_nn, grid, dim3(BF_T), 0, rows, rc, cols, cc, set_pitch, max_n, rbest));
    if (crosscheck)
        TB_TRY(tb_launch(ctx, "k_bf_cross", k_bf_cross, dim3((max_n + BF_T - 1) / BF_T, npairs), dim3(BF_T), 0, c2, max_n, d_tbest,
                         d_qbest));
    TB_TRY(tb_launch(ctx, "k_bf_finalize", k_bf_finalize, dim3(npairs), dim3(BF_T), 0, c1, max_n, d_qbest, filter, ratio, min_th, out, cap,
                     out_counts));
    return TB_OK;
}

/* ------------------------------------------------------------------------------------------------
 * Matcher::searchByNN (matcher.cpp:35-95): the LSH nearest neighbour of include/tb_capi.h, stated per pair -- train j is a
 * candidate of query q iff some table's keys differ in at most L bits; the match is the candidate with the smallest
 * (Hamming, j). At the reference's (20, 10, 2) two unrelated descriptors are candidates with probability 0.675, so a bucket walk
 * would visit more entries than there are pairs: this is k_bf_nn's all-pairs tile loop with the predicate on top. The result is
 * a minimum over candidates, so the predicate is evaluated only for a pair whose distance beats the lane's best so far (strictly:
 * a block walks its train rows in ascending order, so the lower index wins a tie), which is rare after the first rows.
 *
 * One thread per query, LSH_T per block; the block walks the train chunks c0 = blockIdx.y * LSH_TC, step gridDim.y * LSH_TC, and
 * the blocks of one query tile meet in an atomicMin on (distance << 32 | train). LDS (dynamic, 16-byte aligned pieces):
 *   td  [LSH_TC][4] u64   the chunk's descriptors (read as a broadcast: every lane reads the same row)
 *   tk  [LSH_TC][T] u32   the chunk's keys, computed by the block from td (broadcast reads)
 *   qk  [T][LSH_T] u32    the block's query keys, table-major: lane-consecutive words, no bank conflict
 *   sb  [T * k] u8        the bit table
 * = 4 KB + (LSH_TC + LSH_T) * T * 4 + T * k bytes: 34.9 KB at (20, 10), 54 KB at (32, 32). */
#define LSH_T 256
#define LSH_TC 128

__device__ __forceinline__ unsigned lsh_key(const unsigned long long w0, const unsigned long long w1, const unsigned long long w2,
                                            const unsigned long long w3, const uint8_t* __restrict__ tb, int k) {
    unsigned key = 0;
    for (int b = 0; b < k; b++) {
        const unsigned bit = tb[b];   /* bit (bit % 8) of byte (bit / 8) = bit (bit % 64) of little-endian word (bit / 64) */
        const unsigned long long lo = (bit & 64) ? w1 : w0, hi = (bit & 64) ? w3 : w2;
        const unsigned long long w = (bit & 128) ? hi : lo;
        key |= (unsigned)((w >> (bit & 63)) & 1ull) << b;
    }
    return key;
}

__global__ void __launch_bounds__(LSH_T)
k_lsh_nn(const uint8_t* __restrict__ query, const int32_t* __restrict__ queryCounts, const uint8_t* __restrict__ train,
         const int32_t* __restrict__ trainCounts, size_t set_pitch, int max_n, const uint8_t* __restrict__ bits, int T, int k, int L,
         unsigned long long* __restrict__ qbest) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lsh_smem[];
    unsigned long long* td = lsh_smem;
    unsigned* tk = reinterpret_cast<unsigned*>(td + LSH_TC * 4);
    unsigned* qk = tk + LSH_TC * T;
    uint8_t* sb = reinterpret_cast<uint8_t*>(qk + LSH_T * T);
    const int p = blockIdx.z, tid = threadIdx.x;
    const int nq = min(queryCounts[p], max_n), nt = min(trainCounts[p], max_n);
    if ((int)(blockIdx.x * LSH_T) >= nq || (int)(blockIdx.y * LSH_TC) >= nt) return;   /* block-uniform */
    for (int i = tid; i < T * k; i += LSH_T) sb[i] = bits[i];
    const int r = blockIdx.x * LSH_T + tid;
    const bool live = r < nq;
    Desc256 d;
    d.w[0] = d.w[1] = d.w[2] = d.w[3] = 0;
    if (live) {
        const unsigned long long* rsrc = reinterpret_cast<const unsigned long long*>(query + (size_t)p * set_pitch) + (size_t)r * 4;
        d.w[0] = rsrc[0]; d.w[1] = rsrc[1]; d.w[2] = rsrc[2]; d.w[3] = rsrc[3];
    }
    __syncthreads();
    for (int t = 0; t < T; t++) qk[t * LSH_T + tid] = lsh_key(d.w[0], d.w[1], d.w[2], d.w[3], sb + t * k, k);
    int best = live ? 0x7fffffff : -1, bi = 0;   /* a lane past the set never takes a row */
    const unsigned long long* tsrc = reinterpret_cast<const unsigned long long*>(train + (size_t)p * set_pitch);
    for (int c0 = blockIdx.y * LSH_TC; c0 < nt; c0 += gridDim.y * LSH_TC) {
        const int cn = min(LSH_TC, nt - c0);
        __syncthreads();   /* the last chunk's readers are done (and, the first time, qk and sb are written) */
        for (int i = tid; i < cn * 4; i += LSH_T) td[i] = tsrc[(size_t)c0 * 4 + i];
        __syncthreads();
        for (int i = tid; i < cn * T; i += LSH_T) {
            const int c = i / T, t = i - c * T;
            tk[i] = lsh_key(td[4 * c], td[4 * c + 1], td[4 * c + 2], td[4 * c + 3], sb + t * k, k);
        }
        __syncthreads();
        for (int c = 0; c < cn; c++) {
            const int dist = bf_dist(d, td + 4 * c);
            if (dist < best) {
                bool cand = false;
                for (int t = 0; t < T; t++) cand |= __popc(qk[t * LSH_T + tid] ^ tk[c * T + t]) <= L;
                if (cand) { best = dist; bi = c0 + c; }
            }
        }
    }
    if (live && best != 0x7fffffff)
        atomicMin(&qbest[(size_t)p * max_n + r], ((unsigned long long)best << 32) | (unsigned)bi);
}

size_t tbk_lsh_lds_bytes(int T, int k) { return (size_t)LSH_TC * 32 + (size_t)(LSH_TC + LSH_T) * T * 4 + (size_t)T * k; }

/* the raw list (filter 0) or searchByNN's (filter 1) of npairs set pairs; d_qbest [npairs][max_n] */
int tbk_lsh_batch(tb_ctx* ctx, int npairs, const uint8_t* d1, const int32_t* c1, const uint8_t* d2, const int32_t* c2, size_t set_pitch,
                  int max_n, const uint8_t* d_bits, int T, int k, int L, int filter, float ratio, float min_th, tb_match* out, int cap,
                  int32_t* out_counts, unsigned long long* d_qbest) {
    if (npairs <= 0 || max_n <= 0) return TB_OK;
    TB_HIP(ctx, hipMemsetAsync(d_qbest, 0xff, (size_t)npairs * max_n * sizeof(unsigned long long), ctx->stream));
    /* train chunks side by side only while the query tiles alone leave compute units idle: every extra block of a query tile
     * starts its minimum afresh and pays the predicate for its first rows again */
    const int tiles = (max_n + LSH_T - 1) / LSH_T, chunks = (max_n + LSH_TC - 1) / LSH_TC;
    int split = 1;
    while (split < 4 && split * 2 <= chunks && (long long)tiles * npairs * split < 2ll * ctx->num_cu) split *= 2;
    TB_TRY(tb_launch(ctx, "k_lsh_nn", k_lsh_nn, dim3(tiles, split, npairs), dim3(LSH_T), tbk_lsh_lds_bytes(T, k), d1, c1, d2, c2, set_pitch,
                     max_n, d_bits, T, k, L, d_qbest));
    TB_TRY(tb_launch(ctx, "k_bf_finalize", k_bf_finalize, dim3(npairs), dim3(BF_T), 0, c1, max_n, d_qbest, filter, ratio, min_th, out, cap,
                     out_counts));
    return TB_OK;
}

/* ------------------------------------------------------------------------------------------------
 * SURVEY 8(f) row 1 -- Matcher::searchByProjection, both overloads (matcher.cpp:406-617): device helpers of
 * k_proj_search_batch, which projects one map point into F1 and derives its search window (matcher.cpp:431-458; the map
 * overload: Frame::IsInFrustum, Frame.cpp:370-412, and matcher.cpp:558-567). Float arithmetic: one rounding
 * per reference operation, fixed-size Eigen 3.3 reduction order c0 + (c1 + c2), no FMA contraction. */
#pragma clang fp contract(off)
struct ProjPose { float T[16]; };

__device__ __forceinline__ void pj_se3_map(const ProjPose& P, const float* X, float* Pc) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float c0 = P.T[4 * i] * X[0], c1 = P.T[4 * i + 1] * X[1], c2 = P.T[4 * i + 2] * X[2];
        Pc[i] = (c0 + (c1 + c2)) + P.T[4 * i + 3];
    }
}
__device__ __forceinline__ void pj_world2cam(const tb_camera& cam, const float* Pc, float* px) {
    const float x = Pc[0] / Pc[2], y = Pc[1] / Pc[2];
    if (!cam.has_distortion) {
        px[0] = cam.fx * x + cam.cx;
        px[1] = cam.fy * y + cam.cy;
    } else {
        const float r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const float a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
        const float cdist = 1 + cam.d[0] * r2 + cam.d[1] * r4 + cam.d[4] * r6;
        const float xd = x * cdist + cam.d[2] * a1 + cam.d[3] * a2;
        const float yd = y * cdist + cam.d[2] * a3 + cam.d[3] * a1;
        px[0] = xd * cam.fx + cam.cx;
        px[1] = yd * cam.fy + cam.cy;
    }
}
__device__ __forceinline__ bool pj_in_frame(const tb_camera& cam, const float* px) {
    if (!(fabsf(px[0]) < 2147483648.f) || !(fabsf(px[1]) < 2147483648.f)) return false; /* x86 cast -> INT_MIN */
    const int u = (int)px[0], v = (int)px[1];
    return u >= 0 && u < (int)((float)cam.width * 1.f) && v >= 0 && v < (int)((float)cam.height * 1.f);
}

/* ------------------------------------------------------------------------------------------------
 * SURVEY 8(f) row 3 -- Frame::AssignFeaturesToGrid (Frame.cpp:187-200, PosInGrid :257-265) on the device, and the
 * batched, device-resident form of searchByProjection(F1, F2) on top of it (no host round trip: projection,
 * window search, acceptance, rotation histogram and the ordered match list all stay in HBM).
 *
 * k_grid_build: one workgroup per frame. The 120x36 lookup grid as CSR: LDS histogram of the keys' cells, block
 * scan, scatter, then every cell's (short) item list is put back into key-index order -- the order
 * std::vector::push_back gives the reference, which decides ties in the matchers. */
#define GRID_CELLS (120 * 36)
__global__ void __launch_bounds__(256)
k_grid_build(const tb_keypoint* __restrict__ keys, const int32_t* __restrict__ counts, int key_pitch, float widthInv,
             float heightInv, int32_t* __restrict__ cellStart, int32_t* __restrict__ cellItems) {
    __shared__ int hist[GRID_CELLS];
    __shared__ int tmp[8];
    const int f = blockIdx.x, tid = threadIdx.x;
    const tb_keypoint* k = keys + (size_t)f * key_pitch;
    const int n = min(counts[f], key_pitch);
    int32_t* start = cellStart + (size_t)f * (GRID_CELLS + 1);
    int32_t* items = cellItems + (size_t)f * key_pitch;
    for (int c = tid; c < GRID_CELLS; c += 256) hist[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int posX = (int)roundf(k[i].x * widthInv), posY = (int)roundf(k[i].y * heightInv);
        if (posX >= 0 && posX < 120 && posY >= 0 && posY < 36) atomicAdd(&hist[posX * 36 + posY], 1);
    }
    __syncthreads();
    const int total = tb_block_excl_scan(hist, GRID_CELLS, tmp);
    for (int c = tid; c < GRID_CELLS; c += 256) start[c] = hist[c];
    if (tid == 0) start[GRID_CELLS] = total;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int posX = (int)roundf(k[i].x * widthInv), posY = (int)roundf(k[i].y * heightInv);
        if (posX >= 0 && posX < 120 && posY >= 0 && posY < 36) items[atomicAdd(&hist[posX * 36 + posY], 1)] = i;
    }
    __syncthreads(); /* hist[c] is now the END of cell c; the global writes below read what this block wrote */
    __threadfence_block();
    for (int c = tid; c < GRID_CELLS; c += 256) { /* insertion sort of the cell's items by key index */
        const int b = start[c], e = hist[c];
        for (int i = b + 1; i < e; i++) {
            const int v = items[i];
            int j = i - 1;
            while (j >= b && items[j] > v) { items[j + 1] = items[j]; j--; }
            items[j + 1] = v;
        }
    }
}

/* Frame::GetFeaturesInArea (Frame.cpp:202-255) as the matchers use it: every key of the lookup grid (cellStart / cellItems of
 * ONE frame, keys = that frame's) inside the box |kp - (x, y)| < r whose octave passes the level test, in the reference's
 * order (ix, iy, insertion); visit(j, kp) sees each one. */
template <class Visit>
__device__ __forceinline__ void grid_window_walk(const int32_t* __restrict__ cellStart, const int32_t* __restrict__ cellItems,
                                                 const tb_keypoint* __restrict__ keys, float x, float y, float r, float widthInv,
                                                 float heightInv, int minL, int maxL, Visit visit) {
    const int GRID_ROWS = 36, GRID_COLS = 120;
    const int nMinCellX = max(0, (int)floorf((x - r) * widthInv));
    const int nMaxCellX = min(GRID_COLS - 1, (int)ceilf((x + r) * widthInv));
    const int nMinCellY = max(0, (int)floorf((y - r) * heightInv));
    const int nMaxCellY = min(GRID_ROWS - 1, (int)ceilf((y + r) * heightInv));
    if (!(nMinCellX < GRID_COLS && nMaxCellX >= 0 && nMinCellY < GRID_ROWS && nMaxCellY >= 0)) return;
    const bool bCheckLevels = (minL > 0) || (maxL >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const int c = ix * GRID_ROWS + iy;
            for (int s = cellStart[c]; s < cellStart[c + 1]; s++) {
                const int j = cellItems[s];
                const tb_keypoint kp = keys[j];
                if (bCheckLevels) {
                    if (kp.octave < minL) continue;
                    if (maxL >= 0 && kp.octave > maxL) continue;
                }
                if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) continue;
                visit(j, kp);
            }
        }
}

/* The end of searchByProjection, searchByViolence and searchByBow (matcher.cpp:483-530, :352-395, :671-717): acceptance,
 * rotation histogram, ComputeThreeMaxima and the ordered match list of one pair, by one workgroup of 256. The reference's
 * output order -- kept bins ascending, inside a bin the order of acceptance -- is a stable partition: one ordered compaction
 * pass per kept bin (at most three). A matcher is a policy:
 *   int n                  candidates, in the reference's emission order
 *   bool accept(int i)     the matcher's thresholds on candidate i < n
 *   float rotation(int i)  the rotation of an accepted candidate, operands subtracted; asked for only when the orientation is
 *                          checked (searchByProjection's map overload never does, and has no F2 keys to read an angle from)
 *   tb_match make(int i)   the match of an accepted candidate
 * A bin outside the histogram (the reference asserts) sets *flag = 2 and drops the candidate. *out_count may exceed cap: the
 * list is truncated, the count is not. */
template <class Policy>
__device__ __forceinline__ void match_accept_stage(const Policy& P, int histo_len, int check_orientation, tb_match* __restrict__ out,
                                                   int cap, int32_t* out_count, int32_t* flag) {
    __shared__ int hist[1024];
    __shared__ int wsum[4];
    __shared__ int keep[3];
    const int tid = threadIdx.x;
    const float factor = 1.0f / (float)histo_len;
    auto accepted = [&](int i, int& bin) -> bool {
        if (i >= P.n || !P.accept(i)) return false;
        bin = 0;
        if (check_orientation) {
            float rot = P.rotation(i);
            if (rot < 0.0f) rot += 360.0f;
            bin = (int)roundf(rot * factor);
            if (bin == histo_len) bin = 0;
            if (bin < 0 || bin >= histo_len) { *flag = 2; return false; }
        }
        return true;
    };
    if (tid == 0) { keep[0] = check_orientation ? -1 : 0; keep[1] = keep[2] = -1; }
    for (int b = tid; b < histo_len; b += 256) hist[b] = 0;
    __syncthreads();
    if (check_orientation) {
        for (int i = tid; i < P.n; i += 256) { int bin; if (accepted(i, bin)) atomicAdd(&hist[bin], 1); }
        __syncthreads();
        if (tid == 0) {
            int i1 = -1, i2 = -1, i3 = -1;
            tbm::three_maxima(hist, histo_len, &i1, &i2, &i3);
            tbm::kept_bins_ascending(i1, i2, i3, keep);
        }
        __syncthreads();
    }
    int run = 0;
    for (int kb = 0; kb < 3; kb++) {
        const int want = keep[kb];
        if (want < 0) continue;
        for (int e0 = 0; e0 < P.n; e0 += 256) {
            const int i = e0 + tid;
            int bin = 0;
            const bool f = accepted(i, bin) && (!check_orientation || bin == want);
            const int slot = tb_block_ordered_slot(f, run, wsum);
            if (f && slot < cap) out[slot] = P.make(i);
        }
    }
    if (tid == 0) *out_count = run;
}

struct ProjBatch {
    const float* Tcw;                /* [npairs][16] */
    tb_camera cam;
    const tb_keypoint* k1; const uint8_t* d1; const uint8_t* taken1; const int32_t* n1; int pitch1;
    const int32_t* cellStart; const int32_t* cellItems;
    const tb_keypoint* k2; const tb_mappoint* mp2; const uint8_t* mp2d; const int32_t* n2; int pitch2;
    float sf[TB_MAX_LEVELS * 2]; int nlevels;
    float nratio, widthInv, heightInv, radio;
    int th_high, histo_len, check_orientation;
    int max_n2;   /* rows of `best` per pair = most map points any pair has; pitch2 may be 0 (one map shared by all pairs) */
    int map_mode; /* 0: searchByProjection(F1, F2); 1: searchByProjection(map, F1, radio) -- mp2 / mp2d are the map, k2 unused */
    int32_t* best;                   /* [npairs][pitch2][6] */
    tb_match* out; int cap; int32_t* out_counts; int32_t* flags; /* flags[p]: 1 = octave outside the table, 2 = bin outside the histogram */
};

/* projection + window search of one map point of pair blockIdx.y */
__global__ void __launch_bounds__(256)
k_proj_search_batch(ProjBatch B) {
    const int p = blockIdx.y, i2 = blockIdx.x * blockDim.x + threadIdx.x;
    const int n2 = min(B.n2[p], B.max_n2);
    if (i2 >= n2) return;
    ProjPose P;
#pragma unroll
    for (int i = 0; i < 16; i++) P.T[i] = B.Tcw[(size_t)p * 16 + i];
    const tb_mappoint mp = B.mp2[(size_t)p * B.pitch2 + i2];
    int bestDist = 256, bestDist2 = 256, bestIdx = -1, bestLevel = -1, bestLevel2 = -1, ncand = 0;
    bool search = false;
    float x = 0, y = 0, r = 0;
    int minL = 0, maxL = 0;
    if (!mp.bad && !B.map_mode) {
        float Pc[3], uv[2];
        pj_se3_map(P, mp.pos, Pc);
        const float invzc = 1.0f / Pc[2];
        if (!(invzc < 0)) {
            pj_world2cam(B.cam, Pc, uv);
            if (pj_in_frame(B.cam, uv)) {
                const int oct = B.k2[(size_t)p * B.pitch2 + i2].octave;
                if (oct < 0 || oct >= B.nlevels) B.flags[p] = 1; /* benign race */
                else { x = uv[0]; y = uv[1]; r = B.nratio * B.sf[oct]; minL = oct - 1; maxL = oct + 1; search = true; }
            }
        }
    } else if (!mp.bad) { /* Frame::IsInFrustum (Frame.cpp:370-412) + the window of matcher.cpp:558-567 */
        float Pc[3], uv[2], Ow[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float c0 = -P.T[i] * P.T[3], c1 = -P.T[4 + i] * P.T[7], c2 = -P.T[8 + i] * P.T[11];
            Ow[i] = c0 + (c1 + c2);
        }
        pj_se3_map(P, mp.pos, Pc);
        if (!(Pc[2] < 0.0f)) {
            pj_world2cam(B.cam, Pc, uv);
            if (pj_in_frame(B.cam, uv)) {
                const float PO[3] = {mp.pos[0] - Ow[0], mp.pos[1] - Ow[1], mp.pos[2] - Ow[2]};
                const float dist3 = sqrtf(PO[0] * PO[0] + (PO[1] * PO[1] + PO[2] * PO[2]));
                if (!(dist3 < mp.min_dist || dist3 > mp.max_dist)) {
                    const float viewCos = (PO[0] * mp.normal[0] + (PO[1] * mp.normal[1] + PO[2] * mp.normal[2])) / dist3;
                    if (!(viewCos < 0.5f)) {
                        float rr = 4.f;
                        if ((double)viewCos > 0.998) rr = 2.5f;
                        if ((double)B.nratio != 1.0) rr *= B.nratio;
                        x = uv[0]; y = uv[1]; r = rr * B.sf[0]; minL = -1; maxL = 0; search = true;
                    }
                }
            }
        }
    }
    if (search) {
        const uint8_t* d1 = B.d1 + (size_t)p * B.pitch1 * 32;
        const uint8_t* tk = B.taken1 + (size_t)p * B.pitch1;
        const unsigned long long* a = reinterpret_cast<const unsigned long long*>(B.mp2d) + ((size_t)p * B.pitch2 + i2) * 4;
        Desc256 da;
        da.w[0] = a[0]; da.w[1] = a[1]; da.w[2] = a[2]; da.w[3] = a[3];
        grid_window_walk(B.cellStart + (size_t)p * (GRID_CELLS + 1), B.cellItems + (size_t)p * B.pitch1, B.k1 + (size_t)p * B.pitch1,
                         x, y, r, B.widthInv, B.heightInv, minL, maxL, [&](int j, const tb_keypoint& kp) {
            ncand++;
            if (tk[j]) return;
            const int dist = bf_dist(da, reinterpret_cast<const unsigned long long*>(d1) + (size_t)j * 4);
            if (dist < bestDist) {
                bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = kp.octave; bestIdx = j;
            } else if (dist < bestDist2) {
                bestLevel2 = kp.octave; bestDist2 = dist;
            }
        });
    }
    int32_t* o = B.best + ((size_t)p * B.max_n2 + i2) * 6;
    o[0] = bestDist; o[1] = bestDist2; o[2] = bestIdx; o[3] = bestLevel; o[4] = bestLevel2; o[5] = ncand;
}

/* searchByProjection's acceptance (matcher.cpp:483-530; the map overload: :596-617), one workgroup per pair */
struct ProjAccept {
    int n, th_high, map_mode;
    float radio;
    const int32_t* best;
    const tb_keypoint *k1, *k2;
    __device__ bool accept(int i2) const {
        const int bd = best[6 * (size_t)i2], bi = best[6 * (size_t)i2 + 2];
        if (best[6 * (size_t)i2 + 5] == 0 || bi < 0 || bd > th_high) return false;
        return !(map_mode && best[6 * (size_t)i2 + 3] == best[6 * (size_t)i2 + 4] &&
                 (float)bd > radio * (float)best[6 * (size_t)i2 + 1]); /* matcher.cpp:608-609 */
    }
    __device__ float rotation(int i2) const { return k2[i2].angle - k1[best[6 * (size_t)i2 + 2]].angle; }
    __device__ tb_match make(int i2) const {
        tb_match m;
        m.queryIdx = best[6 * (size_t)i2 + 2]; m.trainIdx = i2; m.imgIdx = -1; m.distance = (float)best[6 * (size_t)i2];
        return m;
    }
};
__global__ void __launch_bounds__(256)
k_proj_accept_batch(ProjBatch B) {
    const int p = blockIdx.x;
    const ProjAccept P = {min(B.n2[p], B.max_n2), B.th_high, B.map_mode, B.radio, B.best + (size_t)p * B.max_n2 * 6,
                          B.k1 + (size_t)p * B.pitch1, B.k2 + (size_t)p * B.pitch2};
    match_accept_stage(P, B.histo_len, B.check_orientation, B.out + (size_t)p * B.cap, B.cap, B.out_counts + p, B.flags + p);
}

int tbk_grid_build_batch(tb_ctx* ctx, int nframes, const tb_keypoint* d_keys, const int32_t* d_counts, int key_pitch, int img_w,
                         int img_h, int32_t* d_cellStart, int32_t* d_cellItems) {
    if (nframes <= 0) return TB_OK;
    const float heightInv = 120.f / (float)img_w, widthInv = 36.f / (float)img_h; /* swapped in the reference; kept */
    TB_TRY(tb_launch(ctx, "k_grid_build", k_grid_build, dim3(nframes), dim3(256), 0, d_keys, d_counts, key_pitch, widthInv, heightInv,
                     d_cellStart, d_cellItems));
    return TB_OK;
}

int tbk_projection_batch(tb_ctx* ctx, int npairs, const float* d_Tcw, const tb_camera* cam, int img_w, int img_h,
                         const tb_keypoint* d_k1, const uint8_t* d_d1, const uint8_t* d_taken1, const int32_t* d_n1, int pitch1,
                         const int32_t* d_cellStart, const int32_t* d_cellItems, const tb_keypoint* d_k2, const tb_mappoint* d_mp2,
                         const uint8_t* d_mp2d, const int32_t* d_n2, int pitch2, const float* sf, int nlevels, float nratio,
                         int th_high, int histo_len, int check_orientation, int32_t* d_best, tb_match* d_out, int cap,
                         int32_t* d_out_counts, int32_t* d_flags, int map_mode, float radio, int max_n2) {
    if (npairs <= 0 || max_n2 <= 0) return TB_OK;
    ProjBatch B;
    B.map_mode = map_mode; B.radio = radio; B.max_n2 = max_n2;
    B.Tcw = d_Tcw; B.cam = *cam;
    B.k1 = d_k1; B.d1 = d_d1; B.taken1 = d_taken1; B.n1 = d_n1; B.pitch1 = pitch1;
    B.cellStart = d_cellStart; B.cellItems = d_cellItems;
    B.k2 = d_k2; B.mp2 = d_mp2; B.mp2d = d_mp2d; B.n2 = d_n2; B.pitch2 = pitch2;
    for (int i = 0; i < TB_MAX_LEVELS * 2; i++) B.sf[i] = i < nlevels ? sf[i] : 0.f;
    B.nlevels = nlevels; B.nratio = nratio;
    B.heightInv = 120.f / (float)img_w; B.widthInv = 36.f / (float)img_h;
    B.th_high = th_high; B.histo_len = histo_len; B.check_orientation = check_orientation;
    B.best = d_best; B.out = d_out; B.cap = cap; B.out_counts = d_out_counts; B.flags = d_flags;
    TB_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)npairs * sizeof(int32_t), ctx->stream));
    TB_TRY(tb_launch(ctx, "k_proj_search", k_proj_search_batch, dim3((max_n2 + 255) / 256, npairs), dim3(256), 0, B));
    TB_TRY(tb_launch(ctx, "k_proj_accept", k_proj_accept_batch, dim3(npairs), dim3(256), 0, B));
    return TB_OK;
}

/* ------------------------------------------------------------------------------------------------
 * Batched, device-resident Matcher::searchByViolence (matcher.cpp:299-395) on the device-built lookup grids: pair =
 * blockIdx.y; window search per F1 key, then acceptance (th_low, nratio), rotation histogram,
 * ComputeThreeMaxima and the reference's output order, one workgroup per pair. */
struct VioBatch {
    const tb_keypoint* k1; const uint8_t* d1; const int32_t* n1; int pitch1;
    const tb_keypoint* k2; const uint8_t* d2; const int32_t* n2; int pitch2;
    const int32_t* cellStart; const int32_t* cellItems; /* grids of the F2 frames */
    float widthInv, heightInv, r, nratio;
    int min_level, max_level, th_low, histo_len, check_orientation;
    int32_t* best;            /* [npairs][pitch1][4]: bestDist, bestDist2, bestIdx, candidates */
    tb_match* out; int cap; int32_t* out_counts; int32_t* flags;
};

__global__ void __launch_bounds__(256)
k_window_batch(VioBatch B) {
    const int p = blockIdx.y, i1 = blockIdx.x * blockDim.x + threadIdx.x;
    const int n1 = min(B.n1[p], B.pitch1);
    if (i1 >= n1) return;
    const tb_keypoint* k1 = B.k1 + (size_t)p * B.pitch1;
    const uint8_t* d2 = B.d2 + (size_t)p * B.pitch2 * 32;
    int bestDist = 0x7fffffff, bestDist2 = 0x7fffffff, bestIdx = -1, ncand = 0;
    const unsigned long long* a = reinterpret_cast<const unsigned long long*>(B.d1) + ((size_t)p * B.pitch1 + i1) * 4;
    Desc256 da;
    da.w[0] = a[0]; da.w[1] = a[1]; da.w[2] = a[2]; da.w[3] = a[3];
    grid_window_walk(B.cellStart + (size_t)p * (GRID_CELLS + 1), B.cellItems + (size_t)p * B.pitch2, B.k2 + (size_t)p * B.pitch2,
                     k1[i1].x, k1[i1].y, B.r, B.widthInv, B.heightInv, B.min_level, B.max_level, [&](int j, const tb_keypoint&) {
        ncand++;
        const int dist = bf_dist(da, reinterpret_cast<const unsigned long long*>(d2) + (size_t)j * 4);
        if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx = j; }
        else if (dist < bestDist2) bestDist2 = dist;
    });
    int32_t* o = B.best + ((size_t)p * B.pitch1 + i1) * 4;
    o[0] = bestDist; o[1] = bestDist2; o[2] = bestIdx; o[3] = ncand;
}

/* searchByViolence's acceptance (matcher.cpp:352-377), one workgroup per pair */
struct VioAccept {
    int n, th_low;
    float nratio;
    const int32_t* best;
    const tb_keypoint *k1, *k2;
    __device__ bool accept(int i1) const {
        const int bd = best[4 * (size_t)i1], bd2 = best[4 * (size_t)i1 + 1];
        return best[4 * (size_t)i1 + 3] != 0 && bd <= th_low && (float)bd < (float)bd2 * nratio;
    }
    __device__ float rotation(int i1) const { return k1[i1].angle - k2[best[4 * (size_t)i1 + 2]].angle; }
    __device__ tb_match make(int i1) const {
        tb_match m;
        m.queryIdx = i1; m.trainIdx = best[4 * (size_t)i1 + 2]; m.imgIdx = -1; m.distance = (float)best[4 * (size_t)i1];
        return m;
    }
};
__global__ void __launch_bounds__(256)
k_violence_accept_batch(VioBatch B) {
    const int p = blockIdx.x;
    const VioAccept P = {min(B.n1[p], B.pitch1), B.th_low, B.nratio, B.best + (size_t)p * B.pitch1 * 4, B.k1 + (size_t)p * B.pitch1,
                         B.k2 + (size_t)p * B.pitch2};
    match_accept_stage(P, B.histo_len, B.check_orientation, B.out + (size_t)p * B.cap, B.cap, B.out_counts + p, B.flags + p);
}

int tbk_violence_batch(tb_ctx* ctx, int npairs, const tb_keypoint* d_k1, const uint8_t* d_d1, const int32_t* d_n1, int pitch1,
                       const tb_keypoint* d_k2, const uint8_t* d_d2, const int32_t* d_n2, int pitch2, const int32_t* d_cellStart,
                       const int32_t* d_cellItems, int img2_w, int img2_h, int min_level, int max_level, float radius, int th_low,
                       float nratio, int histo_len, int check_orientation, int32_t* d_best, tb_match* d_out, int cap,
                       int32_t* d_out_counts, int32_t* d_flags) {
    if (npairs <= 0 || pitch1 <= 0) return TB_OK;
    VioBatch B;
    B.k1 = d_k1; B.d1 = d_d1; B.n1 = d_n1; B.pitch1 = pitch1;
    B.k2 = d_k2; B.d2 = d_d2; B.n2 = d_n2; B.pitch2 = pitch2;
    B.cellStart = d_cellStart; B.cellItems = d_cellItems;
    B.heightInv = 120.f / (float)img2_w; B.widthInv = 36.f / (float)img2_h; /* swapped in the reference; kept */
    B.r = radius; B.nratio = nratio; B.min_level = min_level; B.max_level = max_level;
    B.th_low = th_low; B.histo_len = histo_len; B.check_orientation = check_orientation;
    B.best = d_best; B.out = d_out; B.cap = cap; B.out_counts = d_out_counts; B.flags = d_flags;
    TB_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)npairs * sizeof(int32_t), ctx->stream));
    TB_TRY(tb_launch(ctx, "k_window_batch", k_window_batch, dim3((pitch1 + 255) / 256, npairs), dim3(256), 0, B));
    TB_TRY(tb_launch(ctx, "k_violence_accept", k_violence_accept_batch, dim3(npairs), dim3(256), 0, B));
    return TB_OK;
}

/* ---- stereo tracks -> pose-optimisation observations (round 3; SURVEY 3.5 / LocalBA.cpp:46-68, :333-363).
 * The reference's per-frame flow is stereo depth -> map points -> PoseOptimization (test/test_vo.cpp:716,761,800): a key of
 * the current frame gets Depth = bf / |x_other - x_key| (LocalBA.cpp:60-64), the test back-projects it through the pinhole
 * model (test_vo.cpp:257-267: norm = ((u - cx) / fx, (v - cy) / fy, 1), X = norm * depth), and PoseOptimization reads per
 * edge the pixel, the point and invSigma2[octave] (LocalBA.cpp:333-363). Here the two keys of a left <-> right match of
 * searchByBF play those roles: X from the LEFT key and the disparity, observed at the RIGHT key's pixel, so the pose that
 * PoseOptimization finds from the identity is the right camera's (a translation by the baseline bf / fx along x, plus whatever
 * the vertical mismatches of the matches ask for). One workgroup per frame; rows in match order; a match without
 * disparity (infinite depth) or with an octave outside the table is dropped by an ordered compaction. float32 arithmetic,
 * one operation per statement (no contraction), the same in oracle_match.cpp. */
__global__ void __launch_bounds__(256)
k_stereo_obs(const tb_keypoint* __restrict__ kl, const tb_keypoint* __restrict__ kr, int key_pitch, const tb_match* __restrict__ matches,
             const int32_t* __restrict__ match_counts, int match_pitch, float fx, float fy, float cx, float cy, float bf,
             const float* __restrict__ inv_sigma2, int nlevels, tb_obs* __restrict__ obs, int obs_pitch, int32_t* __restrict__ obs_counts) {
    __shared__ int wsum[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(match_counts[f], match_pitch);
    const tb_keypoint* L = kl + (size_t)f * key_pitch;
    const tb_keypoint* Rk = kr + (size_t)f * key_pitch;
    const tb_match* M = matches + (size_t)f * match_pitch;
    tb_obs* O = obs + (size_t)f * obs_pitch;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool ok = false;
        tb_obs o = {0, 0, 0, 0, 0, 0};
        if (i < n) {
            const tb_match m = M[i];
            const tb_keypoint a = L[m.queryIdx], b = Rk[m.trainIdx];
            const float depth = bf / fabsf(b.x - a.x);               /* LocalBA.cpp:64 */
            const float nx = (a.x - cx) / fx, ny = (a.y - cy) / fy;  /* test_vo.cpp:257-261 */
            o.u = b.x; o.v = b.y;
            o.X = nx * depth; o.Y = ny * depth; o.Z = depth;
            ok = isfinite(depth) && b.octave >= 0 && b.octave < nlevels;
            o.inv_sigma2 = ok ? inv_sigma2[b.octave] : 0.f;
        }
        const int at = tb_block_ordered_slot(ok, base, wsum);
        if (ok && at < obs_pitch) O[at] = o;
    }
    if (tid == 0) obs_counts[f] = min(base, obs_pitch);
}

int tbk_stereo_obs(tb_ctx* ctx, int nframes, const tb_keypoint* d_kl, const tb_keypoint* d_kr, int key_pitch, const tb_match* d_matches,
                   const int32_t* d_match_counts, int match_pitch, const float K[4], float bf, const float* d_inv_sigma2, int nlevels,
                   tb_obs* d_obs, int obs_pitch, int32_t* d_obs_counts) {
    if (nframes <= 0) return TB_OK;
    TB_TRY(tb_launch(ctx, "k_stereo_obs", k_stereo_obs, dim3(nframes), dim3(256), 0, d_kl, d_kr, key_pitch, d_matches, d_match_counts,
                     match_pitch, K[0], K[1], K[2], K[3], bf, d_inv_sigma2, nlevels, d_obs, obs_pitch, d_obs_counts));
    return TB_OK;
}

/* ---- SURVEY 8(f) row 4, second half: the DBoW2 transform (TemplatedVocabulary::transform, TemplatedVocabulary.h:1218-1260).
 * One thread per descriptor walks the tree: at every level the Hamming distance (FORB::distance, FORB.cpp:81-101) to each
 * child of the current node, the first child with the smallest distance wins (strict <, :1238). The children of a node are
 * consecutive 32-byte rows gathered through the L2 (a 10^6-node ORB vocabulary is 32 MB; the upper levels stay cached, the
 * leaves are one 320-byte gather per feature); ~k L = 60 distances per feature. Bound: gather latency; no SURVEY 8(d) row. */
struct BowVocab {
    int nnodes, L;
    const int32_t* child_start;
    const int32_t* child_items;
    const uint8_t* desc;
    const int32_t* word_id;
    const double* weight;
};
__global__ void __launch_bounds__(256)
k_bow_transform(BowVocab V, const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts, int desc_pitch, int levelsup,
                int32_t* __restrict__ word_ids, int32_t* __restrict__ node_ids, double* __restrict__ weights) {
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = counts ? min(counts[f], desc_pitch) : desc_pitch;
    if (i >= n) return;
    const size_t at = (size_t)f * desc_pitch + i;
    Desc256 a;
    const unsigned long long* pa = reinterpret_cast<const unsigned long long*>(desc + 32 * at);
    a.w[0] = pa[0]; a.w[1] = pa[1]; a.w[2] = pa[2]; a.w[3] = pa[3];
    const int nid_level = V.L - levelsup;
    int final_id = 0, level = 0, nid = 0;
    bool nid_set = nid_level <= 0;   /* root (TemplatedVocabulary.h:1227) */
    int c0 = V.child_start[0], c1 = V.child_start[1];
    while (c1 > c0) {
        level++;
        int best = V.child_items[c0];
        int best_d = bf_dist(a, reinterpret_cast<const unsigned long long*>(V.desc + 32 * (size_t)best));
        for (int c = c0 + 1; c < c1; c++) {
            const int id = V.child_items[c];
            const int dd = bf_dist(a, reinterpret_cast<const unsigned long long*>(V.desc + 32 * (size_t)id));
            if (dd < best_d) { best_d = dd; best = id; }
        }
        final_id = best;
        if (level == nid_level) { nid = final_id; nid_set = true; }
        c0 = V.child_start[final_id]; c1 = V.child_start[final_id + 1];
    }
    if (!nid_set) nid = final_id; /* the branch ended above level L - levelsup: the reference leaves *nid unset */
    if (word_ids) word_ids[at] = V.word_id[final_id];
    if (weights) weights[at] = V.weight[final_id];
    if (node_ids) node_ids[at] = nid;
}

/* The frame's FeatureVector as a sorted key list: (node id << 32 | feature index) of the features whose word is not
 * stopped (w > 0, TemplatedVocabulary.h:1159), ascending -- the std::map's node order, each node's features in insertion
 * order. One workgroup per frame: bow_sorted_keys, then the real keys out. */
#define BOW_MAXN 8192
#define BOW_T 1024 /* threads of k_bow_fv_sort and k_bow_vector */
/* (id << 32 | index) of the entries i < n with weight > 0 into sk (padded with all ones to a power of two), sorted ascending;
 * returns how many there are. The whole block of BOW_T calls it; wsum: one int per wave, read by every thread before it returns. */
__device__ __forceinline__ int bow_sorted_keys(const int32_t* __restrict__ ids, const double* __restrict__ weights, int n,
                                               unsigned long long* sk, int* wsum) {
    const int tid = threadIdx.x;
    int m = 1;
    while (m < n) m <<= 1;
    int mine = 0;
    for (int i = tid; i < m; i += BOW_T) {
        unsigned long long k = ~0ull;
        if (i < n && weights[i] > 0) { k = ((unsigned long long)(unsigned)ids[i] << 32) | (unsigned)i; mine++; }
        sk[i] = k;
    }
    mine = tb_wave_sum(mine);
    if ((tid & 63) == 0) wsum[tid >> 6] = mine;
    tb_block_bitonic_sort_u64(sk, m, BOW_T);
    int total = 0;
    for (int w = 0; w < BOW_T / 64; w++) total += wsum[w];
    return total;
}
__global__ void __launch_bounds__(1024)
k_bow_fv_sort(const int32_t* __restrict__ node_ids, const double* __restrict__ weights, const int32_t* __restrict__ counts,
              int desc_pitch, unsigned long long* __restrict__ keys_out, int32_t* __restrict__ fv_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
    __shared__ int wsum[16];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = counts ? min(counts[f], desc_pitch) : desc_pitch;
    const int total = bow_sorted_keys(node_ids + (size_t)f * desc_pitch, weights + (size_t)f * desc_pitch, n, sk, wsum);
    for (int i = tid; i < total; i += 1024) keys_out[(size_t)f * desc_pitch + i] = sk[i];
    if (tid == 0) fv_counts[f] = total;
}

/* The frame's BowVector (the other half of Frame::SetBow): TemplatedVocabulary::transform(features, v, fv, levelsup),
 * TemplatedVocabulary.h:1124-1188, and BowVector::normalize, BowVector.cpp:57-80, as a sorted list -- word ids ascending (the
 * std::map's order) and their values. One workgroup per frame:
 *   1. (word << 32 | feature) keys of the features whose word is not stopped, sorted in LDS (bow_sorted_keys);
 *   2. a word = a run of equal upper halves; the thread that owns the run's first entry adds the run's weights in list order =
 *      ascending feature index (TF, TF_IDF: addWeight) or keeps the first (IDF, BINARY: addIfNotExist); its slot in the output
 *      is the number of run heads before it;
 *   3. TF / TF_IDF with a scoring object that does not normalise: every value / (double)words. Otherwise the L1 or L2 norm, summed
 *      by ONE thread in ascending word order (the values are doubles and must come out bit for bit: a tree would reorder the
 *      sum), sqrt for L2, and every value / norm when norm > 0.
 * Every statement is one rounding (the library is built with -ffp-contract=off). The chain of step 3 is at most 8192 dependent
 * adds per frame; frames run in parallel. */
__global__ void __launch_bounds__(1024)
k_bow_vector(const int32_t* __restrict__ word_ids, const double* __restrict__ weights, const int32_t* __restrict__ counts, int desc_pitch,
             int weighting, int scoring, int32_t* __restrict__ bv_words, double* __restrict__ bv_values, int32_t* __restrict__ bv_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
    __shared__ int wsum[16];
    __shared__ double s_norm;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = counts ? min(max(counts[f], 0), desc_pitch) : desc_pitch;
    const size_t base = (size_t)f * desc_pitch;
    const int total = bow_sorted_keys(word_ids + base, weights + base, n, sk, wsum);
    __syncthreads();   /* wsum is reused below */
    /* run heads of this thread's contiguous chunk, their rank among all heads */
    const int per = (total + 1023) / 1024;
    const int beg = min(tid * per, total), end = min(beg + per, total);
    int heads = 0;
    for (int j = beg; j < end; j++) heads += (j == 0 || (unsigned)(sk[j] >> 32) != (unsigned)(sk[j - 1] >> 32)) ? 1 : 0;
    const int incl = tb_wave_incl_scan(heads);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    int slot = incl - heads, nwords = 0;
    for (int w = 0; w < 16; w++) {
        if (w < (tid >> 6)) slot += wsum[w];
        nwords += wsum[w];
    }
    const bool add = weighting == 0 || weighting == 1;   /* TF_IDF, TF */
    for (int j = beg; j < end; j++) {
        const unsigned word = (unsigned)(sk[j] >> 32);
        if (j != 0 && word == (unsigned)(sk[j - 1] >> 32)) continue;
        double v = weights[base + (unsigned)sk[j]];
        if (add)
            for (int q = j + 1; q < total && (unsigned)(sk[q] >> 32) == word; q++) v = v + weights[base + (unsigned)sk[q]];
        bv_words[base + slot] = (int32_t)word;
        bv_values[base + slot] = v;
        slot++;
    }
    __syncthreads();   /* the keys are dead; this block's bv_values are visible to it */
    double* vals = reinterpret_cast<double*>(sk);
    for (int i = tid; i < nwords; i += 1024) vals[i] = bv_values[base + i];
    __syncthreads();
    const bool must = scoring != 5, l2 = scoring == 1;   /* DOT_PRODUCT does not normalise; L2_NORM */
    double div = 0.0;
    if (!must) {
        if (add) div = (double)nwords;
    } else {
        if (tid == 0) {
            double norm = 0.0;
            if (l2)
                for (int i = 0; i < nwords; i++) { const double sq = vals[i] * vals[i]; norm = norm + sq; }
            else
                for (int i = 0; i < nwords; i++) norm = norm + fabs(vals[i]);
            if (l2) norm = sqrt(norm);
            s_norm = norm;
        }
        __syncthreads();
        div = s_norm;
    }
    if (div > 0.0)
        for (int i = tid; i < nwords; i += 1024) bv_values[base + i] = vals[i] / div;
    if (tid == 0) bv_counts[f] = nwords;
}

/* Batched searchByBow, search stage: one thread per entry of F1's feature vector (= the reference's emission order once the
 * entries of nodes F2 does not have are dropped): the node's entries of F2 by binary search, then best / second best Hamming
 * distance in list order (matcher.cpp:645-669). best[pos] = {bestDist1, bestDist2, bestIdx2, 1 if F2 has the node}.
 * ix1 / ix2 (NULL: pair p reads frame p of each side) give the frame of side 1 and side 2 that pair p reads, so a caller can
 * match frames where they lie (tb_relocalize_batch_dev: a query against several stored keyframes); best, out, out_counts and
 * flags stay per pair. A frame index < 0 is a pair without a partner: nothing is read, its count and flag are 0. */
struct BowBatch {
    const tb_keypoint *k1, *k2;
    const uint8_t *d1, *d2, *has_mp2;
    const unsigned long long *fv1, *fv2;
    const int32_t *n1, *n2;
    const int32_t *ix1, *ix2;
    int pitch1, pitch2, map_point_only, th_low, histo_len, check_orientation, cap;
    float nratio;
    int32_t* best;
    tb_match* out;
    int32_t *out_counts, *flags;
};
__global__ void __launch_bounds__(256)
k_bow_search_batch(BowBatch B) {
    const int p = blockIdx.y, pos = blockIdx.x * blockDim.x + threadIdx.x;
    const int f1 = B.ix1 ? B.ix1[p] : p, f2 = B.ix2 ? B.ix2[p] : p;
    if (f1 < 0 || f2 < 0) return;
    const int n1 = min(B.n1[f1], B.pitch1), n2 = min(B.n2[f2], B.pitch2);
    if (pos >= n1) return;
    const unsigned long long key = B.fv1[(size_t)f1 * B.pitch1 + pos];
    const unsigned node = (unsigned)(key >> 32), idx1 = (unsigned)key;
    const unsigned long long* F2 = B.fv2 + (size_t)f2 * B.pitch2;
    int lo = 0, hi = n2;
    const unsigned long long want = (unsigned long long)node << 32;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (F2[mid] < want) lo = mid + 1; else hi = mid; }
    int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256, found = 0;
    if (idx1 < (unsigned)B.pitch1) {
        Desc256 a;
        const unsigned long long* pa = reinterpret_cast<const unsigned long long*>(B.d1 + 32 * ((size_t)f1 * B.pitch1 + idx1));
        a.w[0] = pa[0]; a.w[1] = pa[1]; a.w[2] = pa[2]; a.w[3] = pa[3];
        for (int q = lo; q < n2 && (unsigned)(F2[q] >> 32) == node; q++) {
            found = 1;
            const unsigned idx2 = (unsigned)F2[q];
            if (idx2 >= (unsigned)B.pitch2) continue;
            if (B.map_point_only && !(B.has_mp2 && B.has_mp2[(size_t)f2 * B.pitch2 + idx2])) continue;
            const int dist = bf_dist(a, reinterpret_cast<const unsigned long long*>(B.d2 + 32 * ((size_t)f2 * B.pitch2 + idx2)));
            if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdx2 = (int)idx2; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
    }
    reinterpret_cast<int4*>(B.best)[(size_t)p * B.pitch1 + pos] = make_int4(bestDist1, bestDist2, bestIdx2, found);
}
/* searchByBow's acceptance (matcher.cpp:671-689; output order :703-717), one workgroup per pair */
struct BowAccept {
    int n, th_low;
    float nratio;
    const int32_t* best;
    const unsigned long long* F1;
    const tb_keypoint *k1, *k2;
    __device__ bool accept(int pos) const {
        const int bd = best[4 * (size_t)pos], bd2 = best[4 * (size_t)pos + 1];
        return best[4 * (size_t)pos + 3] != 0 && best[4 * (size_t)pos + 2] >= 0 && bd < th_low && (float)bd < nratio * (float)bd2;
    }
    __device__ float rotation(int pos) const { return k1[(unsigned)F1[pos]].angle - k2[best[4 * (size_t)pos + 2]].angle; }
    __device__ tb_match make(int pos) const {
        tb_match m;
        m.queryIdx = (int)(unsigned)F1[pos]; m.trainIdx = best[4 * (size_t)pos + 2]; m.imgIdx = -1; m.distance = (float)best[4 * (size_t)pos];
        return m;
    }
};
__global__ void __launch_bounds__(256)
k_bow_accept_batch(BowBatch B) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int f1 = B.ix1 ? B.ix1[p] : p, f2 = B.ix2 ? B.ix2[p] : p;
    if (tid == 0) B.flags[p] = 0;   /* ahead of the stage's first barrier, so of every flag it raises */
    if (f1 < 0 || f2 < 0) {   /* the whole workgroup: no barrier has been reached */
        if (tid == 0) B.out_counts[p] = 0;
        return;
    }
    const BowAccept P = {min(B.n1[f1], B.pitch1), B.th_low, B.nratio, B.best + (size_t)p * B.pitch1 * 4, B.fv1 + (size_t)f1 * B.pitch1,
                         B.k1 + (size_t)f1 * B.pitch1, B.k2 + (size_t)f2 * B.pitch2};
    match_accept_stage(P, B.histo_len, B.check_orientation, B.out + (size_t)p * B.cap, B.cap, B.out_counts + p, B.flags + p);
}

int tbk_bow_transform(tb_ctx* ctx, int nnodes, int L, const int32_t* d_child_start, const int32_t* d_child_items, const uint8_t* d_vdesc,
                      const int32_t* d_word_id, const double* d_weight, int nframes, const uint8_t* d_desc, const int32_t* d_counts,
                      int desc_pitch, int levelsup, int32_t* d_word_ids, int32_t* d_node_ids, double* d_weights,
                      unsigned long long* d_fv_keys, int32_t* d_fv_counts) {
    if (nframes <= 0 || desc_pitch <= 0) return TB_OK;
    BowVocab V = {nnodes, L, d_child_start, d_child_items, d_vdesc, d_word_id, d_weight};
    TB_TRY(tb_launch(ctx, "k_bow_transform", k_bow_transform, dim3((desc_pitch + 255) / 256, nframes), dim3(256), 0, V, d_desc, d_counts,
                     desc_pitch, levelsup, d_word_ids, d_node_ids, d_weights));
    if (d_fv_keys) {
        int m = 1;
        while (m < desc_pitch) m <<= 1;
        const size_t lds = (size_t)m * sizeof(unsigned long long);
        TB_TRY(tb_lds_limit(ctx, (const void*)k_bow_fv_sort, lds));
        TB_TRY(tb_launch(ctx, "k_bow_fv_sort", k_bow_fv_sort, dim3(nframes), dim3(1024), lds, d_node_ids, d_weights, d_counts, desc_pitch,
                         d_fv_keys, d_fv_counts));
    }
    return TB_OK;
}

int tbk_bow_vector(tb_ctx* ctx, int nframes, const int32_t* d_word_ids, const double* d_weights, const int32_t* d_counts, int desc_pitch,
                   int weighting, int scoring, int32_t* d_bv_words, double* d_bv_values, int32_t* d_bv_counts) {
    if (nframes <= 0 || desc_pitch <= 0) return TB_OK;
    int m = 1;
    while (m < desc_pitch) m <<= 1;
    const size_t lds = (size_t)m * sizeof(unsigned long long);
    TB_TRY(tb_lds_limit(ctx, (const void*)k_bow_vector, lds));
    TB_TRY(tb_launch(ctx, "k_bow_vector", k_bow_vector, dim3(nframes), dim3(1024), lds, d_word_ids, d_weights, d_counts, desc_pitch,
                     weighting, scoring, d_bv_words, d_bv_values, d_bv_counts));
    return TB_OK;
}

int tbk_bow_search_batch(tb_ctx* ctx, int npairs, const tb_keypoint* d_k1, const uint8_t* d_d1, int pitch1, const unsigned long long* d_fv1,
                         const int32_t* d_n1, const tb_keypoint* d_k2, const uint8_t* d_d2, int pitch2, const unsigned long long* d_fv2,
                         const int32_t* d_n2, const uint8_t* d_has_mp2, int map_point_only, int th_low, float nratio, int histo_len,
                         int check_orientation, tb_match* d_out, int cap, int32_t* d_out_counts, int32_t* d_flags, int32_t* d_best,
                         const int32_t* d_ix1, const int32_t* d_ix2) {
    if (npairs <= 0) return TB_OK;
    BowBatch B;
    B.ix1 = d_ix1; B.ix2 = d_ix2;
    B.k1 = d_k1; B.k2 = d_k2; B.d1 = d_d1; B.d2 = d_d2; B.has_mp2 = d_has_mp2; B.fv1 = d_fv1; B.fv2 = d_fv2; B.n1 = d_n1; B.n2 = d_n2;
    B.pitch1 = pitch1; B.pitch2 = pitch2; B.map_point_only = map_point_only; B.th_low = th_low; B.histo_len = histo_len;
    B.check_orientation = check_orientation; B.cap = cap; B.nratio = nratio; B.best = d_best; B.out = d_out; B.out_counts = d_out_counts;
    B.flags = d_flags;
    TB_TRY(tb_launch(ctx, "k_bow_search_batch", k_bow_search_batch, dim3((pitch1 + 255) / 256, npairs), dim3(256), 0, B));
    TB_TRY(tb_launch(ctx, "k_bow_accept_batch", k_bow_accept_batch, dim3(npairs), dim3(256), 0, B));
    return TB_OK;
}
