/* DBoW2 vocabulary training: TemplatedVocabulary<FORB::TDescriptor, FORB>::create (third_part/DBoW2/DBoW2/
 * TemplatedVocabulary.h:558-616; HKmeansStep :642-819, initiateClustersKMpp :833-913, createWords :918-938, setNodeWeights
 * :943-996; FORB::meanValue FORB.cpp:28-77, FORB::distance :81-101). See include/tb_capi.h (tb_vocab_train) for the
 * semantics and the three deviations (counter-based random numbers, an empty cluster keeps its centre, max_iters).
 *
 * The tree is built one level at a time. The descriptors of a level lie in one array in which every node of the previous
 * level owns a contiguous segment, in the order the recursion would hand them over (the partition is stable), so all nodes
 * of a level run their k-means together:
 *   k_voc_seed      one workgroup per segment: kmeans++ (D(x) weights, prefix threshold on integer sums, k - 1 rounds);
 *                   a segment of n <= k descriptors gets one cluster per descriptor; a segment of more than one tile
 *                   is seeded by one launch pair per centre instead (k_voc_seed_update on all its tiles, k_voc_seed_pick);
 *   k_voc_assoc     one thread per descriptor against its segment's <= k centres in LDS, first-min rule, "changed" flags;
 *   k_voc_means     per tile of VTILE descriptors the 256 bit counts of every cluster in LDS (thread b owns bit b, so no
 *                   conflicts); a segment of one tile takes the majority at once, a longer one adds its counts to global
 *                   integers (k_voc_means_fin takes the majority) -- integer sums, so any order gives the same bits;
 *   k_voc_hist / k_voc_offsets / k_voc_scatter   stable segmented partition of the descriptors by cluster.
 * A converged assignment is a fixed point, so a level iterates until no segment changes (one flag read per iteration) and
 * segments that have converged are skipped. The host keeps the per-level segment and tile tables (a few integers per node).
 * Final passes: k_voc_sub / k_voc_ids renumber the level-order nodes to create's id order, k_voc_place / k_voc_fill write the
 * tb_vocab arrays, k_voc_docmask / k_voc_docpop count Ni (documents per word) from k_bow_transform's walk.
 *
 * Bound: k_voc_assoc is integer VALU (k popcount-256 per descriptor, as the matchers); k_voc_means is LDS read-modify-write
 * (one counter update per descriptor and bit). */
#include <algorithm>
#include <math.h>

#include "tb_internal.h"
#include "tb_device.h"

#define VT 256      /* threads per workgroup: one per descriptor bit in k_voc_means */
#define VTILE 1024  /* descriptors per tile */
#define VKMAX 32    /* largest k */

struct D256 { unsigned long long w[4]; };
struct VSeg { int start, n, kidx, lidx, tile0, ntiles, j, pad; };  /* kidx: index among the k-means segments or -1 */
struct VTile { int seg, off, len, pad; };

__device__ __forceinline__ D256 ld256(const D256* p) {
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1];
    D256 d;
    d.w[0] = a.x; d.w[1] = a.y; d.w[2] = b.x; d.w[3] = b.y;
    return d;
}
__device__ __forceinline__ void st256(D256* p, const D256& d) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(d.w[0], d.w[1]);
    q[1] = make_ulonglong2(d.w[2], d.w[3]);
}
__device__ __forceinline__ int dist256(const D256& a, const D256& b) {
    return __popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1]) + __popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]);
}

/* output i of the splitmix64 stream of `seed` (synth.Stream) as a double in [0, 1) */
__device__ __forceinline__ double voc_uniform(unsigned long long seed, unsigned i) {
    unsigned long long z = seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

/* exclusive scan of one value per thread over the VT threads of the block; sh: LDS, 4 words. Ends with a barrier. */
__device__ __forceinline__ unsigned long long voc_block_scan(unsigned long long v, unsigned long long* total, unsigned long long* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) sh[w] = incl;
    __syncthreads();
    unsigned long long base = 0;
    for (int i = 0; i < w; i++) base += sh[i];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + incl - v;
}

/* [ndocs][pitch][32] with counts -> the documents concatenated */
__global__ void __launch_bounds__(VT)
k_voc_pack(const uint8_t* __restrict__ src, const int32_t* __restrict__ docoff, int pitch, D256* __restrict__ dst) {
    const int d = blockIdx.y, i = blockIdx.x * VT + threadIdx.x;
    const int o = docoff[d], n = docoff[d + 1] - o;
    if (i >= n) return;
    st256(dst + o + i, ld256(reinterpret_cast<const D256*>(src) + (size_t)d * pitch + i));
}

/* kmeans++ seeding of every segment of the level (initiateClustersKMpp), or the trivial clustering of a small one */
__global__ void __launch_bounds__(VT)
k_voc_seed(const VSeg* __restrict__ segs, const D256* __restrict__ D, int k, unsigned long long seedbase, int32_t* __restrict__ nclus,
           D256* __restrict__ centres, uint16_t* mind, uint8_t* __restrict__ assoc) {
    __shared__ unsigned long long sh[4];
    __shared__ D256 cen;
    __shared__ unsigned long long s_target;
    const VSeg sg = segs[blockIdx.x];
    const int tid = threadIdx.x, n = sg.n;
    if (sg.kidx < 0) {
        for (int i = tid; i < n; i += VT) assoc[sg.start + i] = (uint8_t)i;
        if (tid == 0) nclus[blockIdx.x] = n;
        return;
    }
    if (sg.lidx >= 0) return;   /* more than one tile: k_voc_seed_first / _update / _pick */
    const unsigned long long seed = seedbase + (unsigned long long)sg.j;
    const D256* Ds = D + sg.start;
    uint16_t* md = mind + sg.start;
    D256* cs = centres + (size_t)sg.kidx * k;
    unsigned draw = 0;   /* only thread 0 draws */
    if (tid == 0) {
        const double u = voc_uniform(seed, draw++);
        const int first = min((int)(u * (double)n), n - 1);
        cen = ld256(Ds + first);
        st256(cs, cen);
    }
    __syncthreads();
    const int per = (n + VT - 1) / VT;
    const int beg = min(tid * per, n), end = min(beg + per, n);
    int nc = 1;
    for (; nc < k; nc++) {
        const D256 c = cen;
        for (int i = tid; i < n; i += VT) {
            int m;
            if (nc == 1) m = dist256(ld256(Ds + i), c);
            else {
                m = md[i];
                if (m > 0) m = min(m, dist256(ld256(Ds + i), c));   /* a point at distance 0 is never updated (:875) */
            }
            md[i] = (uint16_t)m;
        }
        __syncthreads();   /* md[] of this block, written above, is read below by other threads of it */
        unsigned long long s = 0;
        for (int i = beg; i < end; i++) s += md[i];
        unsigned long long total;
        const unsigned long long excl = voc_block_scan(s, &total, sh);
        if (total == 0) break;   /* all descriptors equal a centre (:885, :909) */
        if (tid == 0) {
            double cut;
            do cut = voc_uniform(seed, draw++) * (double)total; while (cut == 0.0);
            /* the sums are integers: "running sum >= cut_d" is "running sum >= ceil(cut_d)" */
            s_target = min((unsigned long long)ceil(cut), total);
        }
        __syncthreads();
        const unsigned long long target = s_target;
        if (excl < target && target <= excl + s) {
            unsigned long long run = excl;
            int pick = end - 1;
            for (int i = beg; i < end; i++) {
                run += md[i];
                if (run >= target) { pick = i; break; }
            }
            cen = ld256(Ds + pick);
            st256(cs + nc, cen);
        }
        __syncthreads();
    }
    if (tid == 0) nclus[blockIdx.x] = nc;
}

/* The same seeding for a segment of more than one tile, one launch pair per centre so that the distance pass runs on all
 * tiles at once: k_voc_seed_first draws the first centre, k_voc_seed_update refreshes the distances of one tile against the
 * newest centre and sums them, k_voc_seed_pick (one workgroup per segment) walks the tile sums, then the tile the threshold
 * falls in. done[l] != 0: the distances of large segment l summed to 0, its seeding has ended. */
__global__ void __launch_bounds__(VT)
k_voc_seed_first(int nl, const int32_t* __restrict__ large, const VSeg* __restrict__ segs, const D256* __restrict__ D, int k,
                 unsigned long long seedbase, int32_t* __restrict__ nclus, D256* __restrict__ centres, int32_t* __restrict__ draws,
                 int32_t* __restrict__ done) {
    const int li = blockIdx.x * VT + threadIdx.x;
    if (li >= nl) return;
    const int s = large[li];
    const VSeg sg = segs[s];
    const double u = voc_uniform(seedbase + (unsigned long long)sg.j, 0);
    const int first = min((int)(u * (double)sg.n), sg.n - 1);
    st256(centres + (size_t)sg.kidx * k, ld256(D + sg.start + first));
    nclus[s] = 1;
    draws[li] = 1;
    done[li] = 0;
}

__global__ void __launch_bounds__(VT)
k_voc_seed_update(const VTile* __restrict__ tiles, const VSeg* __restrict__ segs, const D256* __restrict__ D, int k, int r,
                  const D256* __restrict__ centres, const int32_t* __restrict__ done, uint16_t* __restrict__ mind,
                  int32_t* __restrict__ tilesum) {
    __shared__ unsigned long long sh[4];
    const VTile t = tiles[blockIdx.x];
    const VSeg sg = segs[t.seg];
    if (done[sg.lidx]) return;
    const D256 c = ld256(centres + (size_t)sg.kidx * k + (r - 1));
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < t.len; i += VT) {
        int m;
        if (r == 1) m = dist256(ld256(D + t.off + i), c);
        else {
            m = mind[t.off + i];
            if (m > 0) m = min(m, dist256(ld256(D + t.off + i), c));
        }
        mind[t.off + i] = (uint16_t)m;
        s += m;
    }
    unsigned long long total;
    voc_block_scan(s, &total, sh);
    if (threadIdx.x == 0) tilesum[blockIdx.x] = (int)total;
}

__global__ void __launch_bounds__(VT)
k_voc_seed_pick(const int32_t* __restrict__ large, const VSeg* __restrict__ segs, const D256* __restrict__ D, int k, int r,
                unsigned long long seedbase, const int32_t* __restrict__ tilesum, const uint16_t* __restrict__ mind,
                int32_t* __restrict__ nclus, D256* __restrict__ centres, int32_t* __restrict__ draws, int32_t* __restrict__ done) {
    __shared__ unsigned long long sh[4];
    __shared__ unsigned long long s_target;
    const int li = blockIdx.x, s = large[li], tid = threadIdx.x;
    if (done[li]) return;
    const VSeg sg = segs[s];
    const int per = (sg.ntiles + VT - 1) / VT;
    const int beg = min(tid * per, sg.ntiles), end = min(beg + per, sg.ntiles);
    unsigned long long sum = 0;
    for (int t = beg; t < end; t++) sum += (unsigned long long)tilesum[sg.tile0 + t];
    unsigned long long total;
    const unsigned long long excl = voc_block_scan(sum, &total, sh);
    if (total == 0) {
        if (tid == 0) done[li] = 1;
        return;
    }
    if (tid == 0) {
        const unsigned long long seed = seedbase + (unsigned long long)sg.j;
        unsigned draw = (unsigned)draws[li];
        double cut;
        do cut = voc_uniform(seed, draw++) * (double)total; while (cut == 0.0);
        draws[li] = (int)draw;
        s_target = min((unsigned long long)ceil(cut), total);
    }
    __syncthreads();
    const unsigned long long target = s_target;
    if (excl < target && target <= excl + sum) {
        unsigned long long run = excl;
        int pick = sg.start + sg.n - 1;
        for (int t = beg; t < end; t++) {
            const unsigned long long ts = (unsigned long long)tilesum[sg.tile0 + t];
            if (run + ts >= target) {
                const int base = sg.start + t * VTILE, len = min(VTILE, sg.n - t * VTILE);
                for (int i = 0; i < len; i++) {
                    run += mind[base + i];
                    if (run >= target) { pick = base + i; break; }
                }
                break;
            }
            run += ts;
        }
        st256(centres + (size_t)sg.kidx * k + r, ld256(D + pick));
        nclus[s] = r + 1;
    }
}

/* every descriptor to the first centre of smallest distance (HKmeansStep :730-751) */
__global__ void __launch_bounds__(VT)
k_voc_assoc(const VTile* __restrict__ tiles, const VSeg* __restrict__ segs, const D256* __restrict__ D, const int32_t* __restrict__ nclus,
            const D256* __restrict__ centres, int k, uint8_t* __restrict__ assoc, int first, const int32_t* __restrict__ active,
            int32_t* __restrict__ chg, int32_t* __restrict__ flag) {
    __shared__ D256 c[VKMAX];
    const VTile t = tiles[blockIdx.x];
    const VSeg sg = segs[t.seg];
    if (sg.kidx < 0 || (active && !active[t.seg])) return;
    const int nc = nclus[t.seg], tid = threadIdx.x;
    if (tid < nc * 4)
        reinterpret_cast<unsigned long long*>(c)[tid] = reinterpret_cast<const unsigned long long*>(centres + (size_t)sg.kidx * k)[tid];
    __syncthreads();
    int changed = 0;
    for (int i = tid; i < t.len; i += VT) {
        const D256 d = ld256(D + t.off + i);
        int best = dist256(d, c[0]), bi = 0;
        for (int j = 1; j < nc; j++) {
            const int dd = dist256(d, c[j]);
            if (dd < best) { best = dd; bi = j; }
        }
        if (!first && assoc[t.off + i] != bi) changed = 1;
        assoc[t.off + i] = (uint8_t)bi;
    }
    if (__syncthreads_or(changed) && tid == 0) { chg[t.seg] = 1; *flag = 1; }
}

/* bit majority of one cluster: thread b holds the count of bit b; wave w's ballot is word w of the descriptor */
__device__ __forceinline__ void voc_majority(int count, int n_c, D256* centre) {
    if (n_c <= 0) return;   /* an empty cluster keeps its last centre */
    const unsigned long long m = __ballot(count >= n_c / 2 + n_c % 2);
    if ((threadIdx.x & 63) == 0) centre->w[threadIdx.x >> 6] = m;
}

/* FORB::meanValue of every cluster of the level */
__global__ void __launch_bounds__(VT)
k_voc_means(const VTile* __restrict__ tiles, const VSeg* __restrict__ segs, const D256* __restrict__ D, const uint8_t* __restrict__ assoc,
            const int32_t* __restrict__ nclus, int k, D256* __restrict__ centres, const int32_t* __restrict__ active,
            int32_t* __restrict__ bitcnt, int32_t* __restrict__ csize) {
    __shared__ int cnt[VKMAX * 256];
    __shared__ int csz[VKMAX];
    __shared__ D256 sd[VT];
    __shared__ uint8_t sl[VT];
    const VTile t = tiles[blockIdx.x];
    const VSeg sg = segs[t.seg];
    if (sg.kidx < 0 || (active && !active[t.seg])) return;
    const int nc = nclus[t.seg], tid = threadIdx.x, w = tid >> 6, b = tid & 63;
    for (int c = 0; c < nc; c++) cnt[c * 256 + tid] = 0;
    if (tid < VKMAX) csz[tid] = 0;
    for (int base = 0; base < t.len; base += VT) {
        __syncthreads();
        const int m = min(VT, t.len - base);
        if (tid < m) {
            sd[tid] = ld256(D + t.off + base + tid);
            const int lab = assoc[t.off + base + tid];
            sl[tid] = (uint8_t)lab;
            atomicAdd(&csz[lab], 1);
        }
        __syncthreads();
        for (int j = 0; j < m; j++) cnt[sl[j] * 256 + tid] += (int)((sd[j].w[w] >> b) & 1ull);
    }
    __syncthreads();
    if (sg.ntiles == 1) {
        for (int c = 0; c < nc; c++) voc_majority(cnt[c * 256 + tid], csz[c], centres + (size_t)sg.kidx * k + c);
    } else {
        for (int c = 0; c < nc; c++) {
            const int v = cnt[c * 256 + tid];
            if (v) atomicAdd(&bitcnt[((size_t)sg.lidx * k + c) * 256 + tid], v);
        }
        if (tid < nc && csz[tid]) atomicAdd(&csize[(size_t)sg.lidx * k + tid], csz[tid]);
    }
}

/* the segments of more than one tile: majority of the summed counts, which are cleared for the next iteration */
__global__ void __launch_bounds__(VT)
k_voc_means_fin(const int32_t* __restrict__ large, const VSeg* __restrict__ segs, const int32_t* __restrict__ nclus, int k,
                D256* __restrict__ centres, const int32_t* __restrict__ active, int32_t* __restrict__ bitcnt, int32_t* __restrict__ csize) {
    const int s = large[blockIdx.x];
    if (active && !active[s]) return;
    const VSeg sg = segs[s];
    const int nc = nclus[s], tid = threadIdx.x;
    for (int c = 0; c < nc; c++) {
        const size_t at = ((size_t)sg.lidx * k + c) * 256 + tid;
        const int v = bitcnt[at];
        bitcnt[at] = 0;
        voc_majority(v, csize[(size_t)sg.lidx * k + c], centres + (size_t)sg.kidx * k + c);
    }
    __syncthreads();
    if (tid < nc) csize[(size_t)sg.lidx * k + tid] = 0;
}

/* stable partition by cluster, step 1: descriptors per (tile, cluster) */
__global__ void __launch_bounds__(VT)
k_voc_hist(const VTile* __restrict__ tiles, const uint8_t* __restrict__ assoc, int k, int32_t* __restrict__ hist) {
    __shared__ int h[VKMAX];
    const VTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < VKMAX) h[tid] = 0;
    __syncthreads();
    for (int i = tid; i < t.len; i += VT) atomicAdd(&h[assoc[t.off + i]], 1);
    __syncthreads();
    if (tid < k) hist[(size_t)blockIdx.x * k + tid] = h[tid];
}

/* step 2, one wave per segment, lane c = cluster c: hist[tile][c] becomes the position of the first descriptor of cluster c
 * of that tile in the partitioned array; childn[seg][c] = size of cluster c */
__global__ void __launch_bounds__(64)
k_voc_offsets(const VSeg* __restrict__ segs, const int32_t* __restrict__ nclus, int k, int32_t* __restrict__ hist,
              int32_t* __restrict__ childn) {
    const VSeg sg = segs[blockIdx.x];
    const int c = threadIdx.x, nc = nclus[blockIdx.x];
    int run = 0;
    if (c < nc)
        for (int t = 0; t < sg.ntiles; t++) {
            int32_t* p = hist + (size_t)(sg.tile0 + t) * k + c;
            const int x = *p;
            *p = run;
            run += x;
        }
    const int off = sg.start + tb_wave_incl_scan(run) - run;
    if (c < nc)
        for (int t = 0; t < sg.ntiles; t++) hist[(size_t)(sg.tile0 + t) * k + c] += off;
    if (c < k) childn[(size_t)blockIdx.x * k + c] = run;
}

/* step 3: move the descriptors; within a cluster they keep their order */
__global__ void __launch_bounds__(VT)
k_voc_scatter(const VTile* __restrict__ tiles, const D256* __restrict__ D, const uint8_t* __restrict__ assoc, const int32_t* __restrict__ nclus,
              int k, const int32_t* __restrict__ tilebase, D256* __restrict__ out) {
    __shared__ int run[VKMAX];
    __shared__ int wcnt[4][VKMAX];
    const VTile t = tiles[blockIdx.x];
    const int nc = nclus[t.seg], tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (tid < nc) run[tid] = tilebase[(size_t)blockIdx.x * k + tid];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < t.len; base += VT) {
        const bool valid = base + tid < t.len;
        const int lab = valid ? assoc[t.off + base + tid] : -1;
        int rank = 0;
        for (int c = 0; c < nc; c++) {
            const unsigned long long m = __ballot(lab == c);
            if (lab == c) rank = __popcll(m & below);
            if (lane == 0) wcnt[w][c] = __popcll(m);
        }
        __syncthreads();
        if (valid) {
            int pos = run[lab] + rank;
            for (int i = 0; i < w; i++) pos += wcnt[i][lab];
            st256(out + pos, ld256(D + t.off + base + tid));
        }
        __syncthreads();
        if (tid < nc) run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads();
    }
}

/* the children of the level's segments into the level-order node array */
__global__ void __launch_bounds__(VT)
k_voc_emit(int nsegs, const VSeg* __restrict__ segs, const int32_t* __restrict__ nclus, const int32_t* __restrict__ child0, int k,
           const D256* __restrict__ centres, const D256* __restrict__ D, D256* __restrict__ node_desc) {
    const int i = blockIdx.x * VT + threadIdx.x, s = i / k, c = i % k;
    if (s >= nsegs || c >= nclus[s]) return;
    const VSeg sg = segs[s];
    st256(node_desc + child0[s] + c, ld256(sg.kidx >= 0 ? centres + (size_t)sg.kidx * k + c : D + sg.start + c));
}

/* ---- renumbering: level order -> create's order (children of a node consecutive, then the subtree of each in turn) */
__global__ void __launch_bounds__(VT)
k_voc_sub(int g0, int g1, const int32_t* __restrict__ nch, const int32_t* __restrict__ child0, int32_t* __restrict__ sub) {
    const int g = g0 + blockIdx.x * VT + threadIdx.x;
    if (g >= g1) return;
    int s = 0;
    for (int c = 0; c < nch[g]; c++) s += 1 + sub[child0[g] + c];
    sub[g] = s;
}
__global__ void __launch_bounds__(VT)
k_voc_ids(int g0, int g1, const int32_t* __restrict__ nch, const int32_t* __restrict__ child0, const int32_t* __restrict__ sub,
          int32_t* __restrict__ id, int32_t* __restrict__ base) {
    const int g = g0 + blockIdx.x * VT + threadIdx.x;
    if (g >= g1) return;
    if (g == 0) { id[0] = 0; base[0] = 1; }
    const int b = g == 0 ? 1 : base[g];
    int run = b + nch[g];
    for (int c = 0; c < nch[g]; c++) {
        const int ch = child0[g] + c;
        id[ch] = b + c;
        base[ch] = run;
        run += sub[ch];
    }
}
__global__ void __launch_bounds__(VT)
k_voc_place(int nn, const int32_t* __restrict__ nch, const int32_t* __restrict__ id, const int32_t* __restrict__ base,
            const D256* __restrict__ node_desc, int32_t* __restrict__ nch_id, int32_t* __restrict__ leaf_id, int32_t* __restrict__ first_id,
            D256* __restrict__ desc_out) {
    const int g = blockIdx.x * VT + threadIdx.x;
    if (g >= nn) return;
    const int i = id[g];
    nch_id[i] = nch[g];
    leaf_id[i] = (g != 0 && nch[g] == 0) ? 1 : 0;
    first_id[i] = base[g];
    st256(desc_out + i, ld256(node_desc + g));
}
__global__ void __launch_bounds__(VT)
k_voc_fill(int nn, const int32_t* __restrict__ child_start, const int32_t* __restrict__ first_id, const int32_t* __restrict__ wordnum,
           int32_t* __restrict__ child_items, int32_t* __restrict__ word_id) {
    const int i = blockIdx.x * VT + threadIdx.x;
    if (i >= nn) return;
    const int c0 = child_start[i], nc = child_start[i + 1] - c0;
    for (int c = 0; c < nc; c++) child_items[c0 + c] = first_id[i] + c;
    word_id[i] = (i != 0 && nc == 0) ? wordnum[i] : 0;
}
__global__ void __launch_bounds__(VT)
k_voc_weights(int nn, const int32_t* __restrict__ child_start, const int32_t* __restrict__ word_id, const double* __restrict__ by_word,
              double* __restrict__ weight) {
    const int i = blockIdx.x * VT + threadIdx.x;
    if (i >= nn) return;
    weight[i] = (i != 0 && child_start[i + 1] == child_start[i]) ? by_word[word_id[i]] : 0.0;
}

/* ---- Ni (setNodeWeights :962-983): documents [d0, d0 + 64) set their bit in the words their descriptors walk to */
__global__ void __launch_bounds__(VT)
k_voc_docmask(const int32_t* __restrict__ word_ids, const int32_t* __restrict__ docoff, int pitch, int d0,
              unsigned long long* __restrict__ mask) {
    const int d = d0 + blockIdx.y, i = blockIdx.x * VT + threadIdx.x;
    if (i >= docoff[d + 1] - docoff[d]) return;
    atomicOr(&mask[word_ids[(size_t)d * pitch + i]], 1ull << (d - d0));
}
__global__ void __launch_bounds__(VT)
k_voc_docpop(int nwords, unsigned long long* __restrict__ mask, int32_t* __restrict__ Ni) {
    const int i = blockIdx.x * VT + threadIdx.x;
    if (i >= nwords) return;
    Ni[i] += __popcll(mask[i]);
    mask[i] = 0;
}

/* ---- exclusive scan of n integers (out[n] = total): tiles of 1024, the tile sums by one workgroup, add back */
__global__ void __launch_bounds__(VT)
k_voc_scan_tile(int n, const int32_t* __restrict__ in, int32_t* __restrict__ out, int32_t* __restrict__ sums) {
    __shared__ unsigned long long sh[4];
    const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
    int v[4];
    unsigned long long s = 0;
    for (int j = 0; j < 4; j++) { v[j] = i0 + j < n ? in[i0 + j] : 0; s += v[j]; }
    unsigned long long total;
    int run = (int)voc_block_scan(s, &total, sh);
    for (int j = 0; j < 4; j++)
        if (i0 + j < n) { out[i0 + j] = run; run += v[j]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = (int)total;
}
__global__ void __launch_bounds__(VT)
k_voc_scan_sums(int ntiles, int32_t* __restrict__ sums) {
    __shared__ unsigned long long sh[4];
    int carry = 0;
    for (int b = 0; b < ntiles; b += VT) {
        const int i = b + threadIdx.x;
        const int v = i < ntiles ? sums[i] : 0;
        unsigned long long total;
        const int e = (int)voc_block_scan((unsigned long long)v, &total, sh);
        if (i < ntiles) sums[i] = carry + e;
        carry += (int)total;
    }
    if (threadIdx.x == 0) sums[ntiles] = carry;
}
__global__ void __launch_bounds__(VT)
k_voc_scan_add(int n, int32_t* __restrict__ out, const int32_t* __restrict__ sums, int ntiles) {
    const int i = blockIdx.x * VT + threadIdx.x;
    if (i < n) out[i] += sums[i >> 10];
    if (i == 0) out[n] = sums[ntiles];
}

/* ================================================================ host driver */
namespace {
struct Work {   /* device allocations of one training run */
    std::vector<void*> p;
    ~Work() { for (void* q : p) hipFree(q); }
    template <class T> hipError_t get(T** out, size_t count) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
    void release(void* q) {   /* hand an allocation over to the caller */
        p.erase(std::remove(p.begin(), p.end(), q), p.end());
    }
};
inline unsigned blocks(size_t n) { return (unsigned)((n + VT - 1) / VT); }
}  // namespace

#define VLAUNCH(name, grid, block, ...) TB_TRY(tb_launch(ctx, #name, name, grid, block, 0, __VA_ARGS__))

static int voc_scan(tb_ctx* ctx, int n, const int32_t* in, int32_t* out, int32_t* sums) {
    const int nt = (n + 1023) / 1024;
    if (nt) VLAUNCH(k_voc_scan_tile, dim3(nt), dim3(VT), n, in, out, sums);
    VLAUNCH(k_voc_scan_sums, dim3(1), dim3(VT), nt, sums);
    VLAUNCH(k_voc_scan_add, dim3(std::max(blocks(n), 1u)), dim3(VT), n, out, sums, nt);
    return TB_OK;
}

int tbk_vocab_train(tb_ctx* ctx, const tb_vocab_train_params* P, int ndocs, const uint8_t* d_desc, const int32_t* h_counts,
                    int desc_pitch, tb_vocab_arrays* out, tb_vocab_train_stats* stats) {
    const int k = P->k, L = P->L;
    Work W;
    std::vector<int32_t> docoff(ndocs + 1, 0);
    for (int d = 0; d < ndocs; d++) docoff[d + 1] = docoff[d] + h_counts[d];
    const int N = docoff[ndocs];
    *stats = tb_vocab_train_stats();

    int32_t *d_docoff, *d_flag;
    D256 *Dcur, *Dnext, *d_node_desc;
    uint8_t* d_assoc;
    uint16_t* d_mind;
    TB_HIP(ctx, W.get(&d_docoff, ndocs + 1));
    TB_HIP(ctx, W.get(&d_flag, 1));
    TB_HIP(ctx, W.get(&Dcur, N));
    TB_HIP(ctx, W.get(&Dnext, N));
    TB_HIP(ctx, W.get(&d_assoc, N));
    TB_HIP(ctx, W.get(&d_mind, N));
    TB_HIP(ctx, hipMemcpyAsync(d_docoff, docoff.data(), (size_t)(ndocs + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (N) VLAUNCH(k_voc_pack, dim3(blocks(desc_pitch), ndocs), dim3(VT), d_desc, d_docoff, desc_pitch, Dcur);

    /* the tree in level order: node g has nch[g] children child0[g] ...; the nodes of the level being expanded own ndesc
     * descriptors from position pos of Dcur */
    std::vector<int32_t> nch(1, 0), child0(1, 0), lvl_off(1, 0);
    std::vector<int32_t> ndesc(1, N), pos(1, 0);
    size_t node_cap = 1 + (size_t)N;   /* level-order descriptors: grown per level */
    TB_HIP(ctx, W.get(&d_node_desc, node_cap));
    TB_HIP(ctx, hipMemsetAsync(d_node_desc, 0, 32, ctx->stream));
    int nnodes = 1;

    for (int level = 1; level <= L; level++) {
        const int g0 = lvl_off[level - 1], np = (int)ndesc.size();
        /* segments: the parents that are expanded (HKmeansStep :645, :813), k-means ones first in the tile table */
        std::vector<VSeg> segs;
        std::vector<int> seg_parent;
        int nk = 0, nl = 0;
        for (int p = 0; p < np; p++) {
            if (ndesc[p] <= (level == 1 ? 0 : 1)) continue;
            VSeg s = {pos[p], ndesc[p], -1, -1, 0, (ndesc[p] + VTILE - 1) / VTILE, p, 0};
            if (s.n > k) { s.kidx = nk++; if (s.ntiles > 1) s.lidx = nl++; }
            segs.push_back(s);
            seg_parent.push_back(p);
        }
        const int S = (int)segs.size();
        if (!S) break;
        lvl_off.push_back(nnodes);   /* first node of the children's level */
        std::vector<VTile> tiles;
        std::vector<int32_t> large;
        for (int pass = 0; pass < 3; pass++)   /* tiles of the multi-tile k-means segments, of the other k-means ones, the rest */
            for (int s = 0; s < S; s++) {
                if ((segs[s].lidx >= 0 ? 0 : segs[s].kidx >= 0 ? 1 : 2) != pass) continue;
                segs[s].tile0 = (int)tiles.size();
                for (int t = 0; t < segs[s].ntiles; t++)
                    tiles.push_back(VTile{s, segs[s].start + t * VTILE, std::min(VTILE, segs[s].n - t * VTILE), 0});
                if (segs[s].lidx >= 0) large.push_back(s);
            }
        int nkt = 0, nlt = 0;   /* tiles of k-means segments; of the multi-tile ones among them */
        for (int s = 0; s < S; s++) {
            if (segs[s].kidx >= 0) nkt += segs[s].ntiles;
            if (segs[s].lidx >= 0) nlt += segs[s].ntiles;
        }
        const int NT = (int)tiles.size();

        Work LW;
        VSeg* d_segs; VTile* d_tiles;
        int32_t *d_large, *d_nclus, *d_chg, *d_bitcnt, *d_csize, *d_hist, *d_childn, *d_child0, *d_tilesum, *d_draws, *d_done;
        D256* d_centres;
        TB_HIP(ctx, LW.get(&d_segs, S));
        TB_HIP(ctx, LW.get(&d_tiles, NT));
        TB_HIP(ctx, LW.get(&d_large, nl));
        TB_HIP(ctx, LW.get(&d_nclus, S));
        TB_HIP(ctx, LW.get(&d_chg, 2 * (size_t)S));
        TB_HIP(ctx, LW.get(&d_bitcnt, (size_t)nl * k * 256));
        TB_HIP(ctx, LW.get(&d_csize, (size_t)nl * k));
        TB_HIP(ctx, LW.get(&d_hist, (size_t)NT * k));
        TB_HIP(ctx, LW.get(&d_childn, (size_t)S * k));
        TB_HIP(ctx, LW.get(&d_child0, S));
        TB_HIP(ctx, LW.get(&d_tilesum, nlt));
        TB_HIP(ctx, LW.get(&d_draws, nl));
        TB_HIP(ctx, LW.get(&d_done, nl));
        TB_HIP(ctx, LW.get(&d_centres, (size_t)nk * k));
        TB_HIP(ctx, hipMemcpyAsync(d_segs, segs.data(), (size_t)S * sizeof(VSeg), hipMemcpyHostToDevice, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(d_tiles, tiles.data(), (size_t)NT * sizeof(VTile), hipMemcpyHostToDevice, ctx->stream));
        if (nl) {
            TB_HIP(ctx, hipMemcpyAsync(d_large, large.data(), (size_t)nl * 4, hipMemcpyHostToDevice, ctx->stream));
            TB_HIP(ctx, hipMemsetAsync(d_bitcnt, 0, (size_t)nl * k * 256 * 4, ctx->stream));
            TB_HIP(ctx, hipMemsetAsync(d_csize, 0, (size_t)nl * k * 4, ctx->stream));
        }
        const unsigned long long seedbase = P->seed + ((unsigned long long)level << 40);
        VLAUNCH(k_voc_seed, dim3(S), dim3(VT), d_segs, Dcur, k, seedbase, d_nclus, d_centres, d_mind, d_assoc);
        if (nl) {
            VLAUNCH(k_voc_seed_first, dim3(blocks(nl)), dim3(VT), nl, d_large, d_segs, Dcur, k, seedbase, d_nclus, d_centres, d_draws, d_done);
            for (int r = 1; r < k; r++) {
                VLAUNCH(k_voc_seed_update, dim3(nlt), dim3(VT), d_tiles, d_segs, Dcur, k, r, d_centres, d_done, d_mind, d_tilesum);
                VLAUNCH(k_voc_seed_pick, dim3(nl), dim3(VT), d_large, d_segs, Dcur, k, r, seedbase, d_tilesum, d_mind, d_nclus, d_centres,
                        d_draws, d_done);
            }
        }

        int iters = 0;
        if (nk) {
            for (int it = 1;; it++) {
                int32_t* cur = d_chg + (size_t)(it & 1) * S;
                const int32_t* act = it >= 3 ? d_chg + (size_t)((it - 1) & 1) * S : nullptr;
                if (it > 1) {
                    VLAUNCH(k_voc_means, dim3(nkt), dim3(VT), d_tiles, d_segs, Dcur, d_assoc, d_nclus, k, d_centres, act, d_bitcnt, d_csize);
                    if (nl) VLAUNCH(k_voc_means_fin, dim3(nl), dim3(VT), d_large, d_segs, d_nclus, k, d_centres, act, d_bitcnt, d_csize);
                }
                TB_HIP(ctx, hipMemsetAsync(cur, 0, (size_t)S * 4, ctx->stream));
                TB_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
                VLAUNCH(k_voc_assoc, dim3(nkt), dim3(VT), d_tiles, d_segs, Dcur, d_nclus, d_centres, k, d_assoc, it == 1 ? 1 : 0, act, cur,
                        d_flag);
                iters = it;
                int32_t flag = 1;
                if (it > 1) {
                    TB_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
                    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
                }
                if (!flag) break;
                if (it == P->max_iters) {   /* the segments that still moved stop here with the centres just used */
                    if (it == 1) stats->capped_nodes += nk;
                    else {
                        std::vector<int32_t> chg(S);
                        TB_HIP(ctx, hipMemcpyAsync(chg.data(), cur, (size_t)S * 4, hipMemcpyDeviceToHost, ctx->stream));
                        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
                        for (int s = 0; s < S; s++) stats->capped_nodes += chg[s] ? 1 : 0;
                    }
                    break;
                }
            }
        }
        stats->iters_per_level[level - 1] = iters;

        VLAUNCH(k_voc_hist, dim3(NT), dim3(VT), d_tiles, d_assoc, k, d_hist);
        VLAUNCH(k_voc_offsets, dim3(S), dim3(64), d_segs, d_nclus, k, d_hist, d_childn);
        VLAUNCH(k_voc_scatter, dim3(NT), dim3(VT), d_tiles, Dcur, d_assoc, d_nclus, k, d_hist, Dnext);
        std::vector<int32_t> nclus(S), childn((size_t)S * k);
        TB_HIP(ctx, hipMemcpyAsync(nclus.data(), d_nclus, (size_t)S * 4, hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipMemcpyAsync(childn.data(), d_childn, (size_t)S * k * 4, hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));

        std::vector<int32_t> nd2, pos2, c0(S);
        for (int s = 0; s < S; s++) {
            const int g = g0 + seg_parent[s];
            if (nclus[s] < 1 || nclus[s] > k) return tb_fail(ctx, TB_EDEVICE, "vocabulary training: %d clusters in a node", nclus[s]);
            nch[g] = nclus[s];
            child0[g] = nnodes;
            c0[s] = nnodes;
            int at = segs[s].start;
            for (int c = 0; c < nclus[s]; c++) {
                const int m = childn[(size_t)s * k + c];
                nd2.push_back(m); pos2.push_back(at);
                at += m;
                if (m == 0) stats->empty_clusters++;
            }
            nnodes += nclus[s];
        }
        nch.resize(nnodes, 0); child0.resize(nnodes, 0);
        if ((size_t)nnodes > node_cap) {   /* grow the level-order descriptor array */
            const size_t cap2 = std::max(node_cap * 2, (size_t)nnodes);
            D256* bigger;
            TB_HIP(ctx, W.get(&bigger, cap2));
            TB_HIP(ctx, hipMemcpyAsync(bigger, d_node_desc, node_cap * 32, hipMemcpyDeviceToDevice, ctx->stream));
            d_node_desc = bigger;
            node_cap = cap2;
        }
        TB_HIP(ctx, hipMemcpyAsync(d_child0, c0.data(), (size_t)S * 4, hipMemcpyHostToDevice, ctx->stream));
        VLAUNCH(k_voc_emit, dim3(blocks((size_t)S * k)), dim3(VT), S, d_segs, d_nclus, d_child0, k, d_centres, Dcur, d_node_desc);
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));   /* c0 and the level's tables go out of scope */
        std::swap(Dcur, Dnext);
        ndesc.swap(nd2); pos.swap(pos2);
    }
    lvl_off.push_back(nnodes);
    const int nlev = (int)lvl_off.size() - 1;   /* levels 0 .. nlev - 1 hold nodes */

    /* ---- final passes: ids in create's order, the tb_vocab arrays, words, weights */
    const int nn = nnodes;
    int32_t *d_nch, *d_child0g, *d_sub, *d_id, *d_base, *d_nch_id, *d_leaf_id, *d_first_id, *d_wordnum, *d_sums;
    TB_HIP(ctx, W.get(&d_nch, nn));
    TB_HIP(ctx, W.get(&d_child0g, nn));
    TB_HIP(ctx, W.get(&d_sub, nn));
    TB_HIP(ctx, W.get(&d_id, nn));
    TB_HIP(ctx, W.get(&d_base, nn));
    TB_HIP(ctx, W.get(&d_nch_id, nn));
    TB_HIP(ctx, W.get(&d_leaf_id, nn));
    TB_HIP(ctx, W.get(&d_first_id, nn));
    TB_HIP(ctx, W.get(&d_wordnum, nn + 1));
    TB_HIP(ctx, W.get(&d_sums, nn / 1024 + 2));
    TB_HIP(ctx, W.get(&out->d_child_start, nn + 1));
    TB_HIP(ctx, W.get(&out->d_child_items, nn));
    TB_HIP(ctx, W.get(&out->d_word_id, nn));
    TB_HIP(ctx, W.get(&out->d_desc, (size_t)nn * 32));
    TB_HIP(ctx, W.get(&out->d_weight, nn));
    TB_HIP(ctx, hipMemcpyAsync(d_nch, nch.data(), (size_t)nn * 4, hipMemcpyHostToDevice, ctx->stream));
    TB_HIP(ctx, hipMemcpyAsync(d_child0g, child0.data(), (size_t)nn * 4, hipMemcpyHostToDevice, ctx->stream));
    TB_HIP(ctx, hipMemsetAsync(d_sub, 0, (size_t)nn * 4, ctx->stream));
    for (int l = nlev - 2; l >= 0; l--)
        VLAUNCH(k_voc_sub, dim3(blocks(lvl_off[l + 1] - lvl_off[l])), dim3(VT), lvl_off[l], lvl_off[l + 1], d_nch, d_child0g, d_sub);
    for (int l = 0; l < nlev; l++)
        VLAUNCH(k_voc_ids, dim3(blocks(lvl_off[l + 1] - lvl_off[l])), dim3(VT), lvl_off[l], lvl_off[l + 1], d_nch, d_child0g, d_sub, d_id,
                d_base);
    VLAUNCH(k_voc_place, dim3(blocks(nn)), dim3(VT), nn, d_nch, d_id, d_base, d_node_desc, d_nch_id, d_leaf_id, d_first_id,
            (D256*)out->d_desc);
    int rc;
    if ((rc = voc_scan(ctx, nn, d_nch_id, out->d_child_start, d_sums))) return rc;
    if ((rc = voc_scan(ctx, nn, d_leaf_id, d_wordnum, d_sums))) return rc;
    VLAUNCH(k_voc_fill, dim3(blocks(nn)), dim3(VT), nn, out->d_child_start, d_first_id, d_wordnum, out->d_child_items, out->d_word_id);
    int32_t nwords = 0;
    TB_HIP(ctx, hipMemcpyAsync(&nwords, d_wordnum + nn, 4, hipMemcpyDeviceToHost, ctx->stream));
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));

    std::vector<double> by_word(std::max(nwords, 1), 1.0);   /* TF, BINARY: 1 (:949-954) */
    if (nwords && (P->weighting == 0 || P->weighting == 2)) {   /* TF_IDF, IDF */
        int32_t *d_words, *d_Ni;
        unsigned long long* d_mask;
        TB_HIP(ctx, W.get(&d_words, (size_t)ndocs * desc_pitch));
        TB_HIP(ctx, W.get(&d_Ni, nwords));
        TB_HIP(ctx, W.get(&d_mask, nwords));
        TB_HIP(ctx, hipMemsetAsync(d_Ni, 0, (size_t)nwords * 4, ctx->stream));
        TB_HIP(ctx, hipMemsetAsync(d_mask, 0, (size_t)nwords * 8, ctx->stream));
        /* the walk of transform(): the counts clamp to the pitch there as here */
        std::vector<int32_t> cnt(h_counts, h_counts + ndocs);
        int32_t* d_cnt;
        TB_HIP(ctx, W.get(&d_cnt, ndocs));
        TB_HIP(ctx, hipMemcpyAsync(d_cnt, cnt.data(), (size_t)ndocs * 4, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = tbk_bow_transform(ctx, nn, L, out->d_child_start, out->d_child_items, out->d_desc, out->d_word_id, out->d_weight, ndocs,
                                    d_desc, d_cnt, desc_pitch, 0, d_words, nullptr, nullptr, nullptr, nullptr)))
            return rc;
        for (int d0 = 0; d0 < ndocs; d0 += 64) {
            VLAUNCH(k_voc_docmask, dim3(blocks(desc_pitch), std::min(64, ndocs - d0)), dim3(VT), d_words, d_docoff, desc_pitch, d0, d_mask);
            VLAUNCH(k_voc_docpop, dim3(blocks(nwords)), dim3(VT), nwords, d_mask, d_Ni);
        }
        std::vector<int32_t> Ni(nwords);
        TB_HIP(ctx, hipMemcpyAsync(Ni.data(), d_Ni, (size_t)nwords * 4, hipMemcpyDeviceToHost, ctx->stream));
        TB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < nwords; i++) by_word[i] = Ni[i] > 0 ? log((double)ndocs / (double)Ni[i]) : 0.0;   /* :986-992 */
    }
    double* d_by_word;
    TB_HIP(ctx, W.get(&d_by_word, by_word.size()));
    TB_HIP(ctx, hipMemcpyAsync(d_by_word, by_word.data(), by_word.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    VLAUNCH(k_voc_weights, dim3(blocks(nn)), dim3(VT), nn, out->d_child_start, out->d_word_id, d_by_word, out->d_weight);
    TB_HIP(ctx, hipStreamSynchronize(ctx->stream));

    out->nnodes = nn;
    stats->nnodes = nn;
    stats->nwords = nwords;
    W.release(out->d_child_start); W.release(out->d_child_items); W.release(out->d_word_id); W.release(out->d_desc); W.release(out->d_weight);
    return TB_OK;
}
