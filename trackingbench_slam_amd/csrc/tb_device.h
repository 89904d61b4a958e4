/* Device-side helpers shared by the kernels (gfx950: 64-lane wavefronts). */
#ifndef TB_DEVICE_H
#define TB_DEVICE_H

#include "tb_internal.h"
#include "tb_math.h"

#define TB_WAVE 64

__device__ __forceinline__ const uint8_t* tb_level_ptr(const PlanGeom& g, const uint8_t* slab, int b, int l,
                                                       int* stride) {
    if (l == 0 && g.img0 != nullptr) {
        *stride = g.img0_stride;
        return g.img0 + (size_t)b * g.img0_pitch;
    }
    *stride = g.lv[l].stride;
    return slab + (size_t)b * g.slabBytes + g.lv[l].off;
}

__device__ __forceinline__ int tb_lane() { return threadIdx.x & (TB_WAVE - 1); }

/* inclusive wave scan (sum) */
__device__ __forceinline__ int tb_wave_incl_scan(int v) {
    const int lane = tb_lane();
#pragma unroll
    for (int d = 1; d < TB_WAVE; d <<= 1) {
        int t = __shfl_up(v, d, TB_WAVE);
        if (lane >= d) v += t;
    }
    return v;
}

/* inclusive wave scan (sum) on the DPP path: Hillis-Steele inside every row of 16 lanes (row_shr 1, 2, 4, 8; lanes
 * shifted in from outside the row read 0), then the row totals travel down with row_bcast 15 / 31. Six vector adds, no
 * LDS round trips; lane 63 ends up with the wave total. */
__device__ __forceinline__ int tb_wave_incl_scan_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); /* row_shr:1 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); /* row_shr:2 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); /* row_shr:4 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); /* row_shr:8 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); /* row_bcast:15 into rows 1, 3 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); /* row_bcast:31 into rows 2, 3 */
    return v;
}
/* bitwise OR over the wave, result in lane 63 (same network) */
__device__ __forceinline__ int tb_wave_or_dpp(int v) {
    v |= __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}

__device__ __forceinline__ int tb_wave_sum(int v) {
#pragma unroll
    for (int d = TB_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, TB_WAVE);
    return v;
}

__device__ __forceinline__ int tb_wave_max_i(int v) {
#pragma unroll
    for (int d = TB_WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, TB_WAVE));
    return v;
}

/* In-place exclusive scan of arr[0..n) in LDS by the whole block; returns the total.
 * tmp: LDS, >= (blockDim.x/64 + 1) ints.  Deterministic (fixed chunking).  Ends with a barrier. */
__device__ inline int tb_block_excl_scan(int* arr, int n, int* tmp) {
    const int T = blockDim.x, tid = threadIdx.x;
    const int per = (n + T - 1) / T;
    const int beg = min(tid * per, n), end = min(beg + per, n);
    int s = 0;
    for (int i = beg; i < end; i++) s += arr[i];
    const int incl = tb_wave_incl_scan(s);
    const int wave = tid >> 6, lane = tid & 63, nw = T >> 6;
    if (lane == 63) tmp[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < nw; w++) { int t = tmp[w]; tmp[w] = acc; acc += t; }
        tmp[nw] = acc;
    }
    __syncthreads();
    int run = tmp[wave] + incl - s;
    for (int i = beg; i < end; i++) { int t = arr[i]; arr[i] = run; run += t; }
    const int total = tmp[nw];
    __syncthreads();
    return total;
}

/* Ordered compaction, one 256-thread chunk: the slot of this thread's element = base + the number of threads with a lower
 * index whose `ok` is set (__ballot prefix counts inside a wave, the wave totals through wsum); base advances by the block's
 * count. EVERY thread of a 256-thread block must call it (two barriers), with the same base; wsum: int[4] in LDS. The second
 * barrier only frees wsum for the next call: it does not order the caller's stores to the slots. */
__device__ __forceinline__ int tb_block_ordered_slot(bool ok, int& base, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bm = __ballot(ok);
    if (lane == 0) wsum[wave] = __popcll(bm);
    __syncthreads();
    int at = base;
    for (int w = 0; w < wave; w++) at += wsum[w];
    at += __popcll(bm & ((1ull << lane) - 1));
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return at;
}

/* Ascending bitonic sort of sk[0..m) in LDS by the whole block, any block size (T = blockDim.x; a caller that knows it passes
 * the constant, which keeps the strided loops' trip counts out of registers); m a power of two. A barrier in front (the caller
 * has just staged sk) and one after every step: it ends on a barrier. */
__device__ __forceinline__ void tb_block_bitonic_sort_u64(unsigned long long* sk, int m, const int T = blockDim.x) {
    __syncthreads();
    for (int k2 = 2; k2 <= m; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += T) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = sk[i], y = sk[l];
                    const bool up = (i & k2) == 0;
                    if ((x > y) == up) { sk[i] = y; sk[l] = x; }
                }
            }
            __syncthreads();
        }
}

#endif
