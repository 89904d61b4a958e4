/* a2 -- image pyramid: cv::resize 8UC1 INTER_LINEAR chain of Frame::ComputePyramid
 * (reference src/types/Frame.cpp:414-427), OpenCV 3.3 fixed-point arithmetic.
 *
 * Roofline: HBM-bound, algorithmic bytes = src px + dst px per level.
 * The source-index / 11-bit coefficient tables are built once per plan on the host with the same
 * double/float arithmetic as the CPU restatement, so the kernel is pure integer work:
 *   D = ((b0*((S0[sx]*a0+S0[sx1]*a1)>>4))>>16) + ((b1*((S1[sx]*a0+S1[sx1]*a1)>>4))>>16) + 2) >> 2.
 * One thread produces 4 consecutive destination pixels (one 32-bit store); consecutive lanes cover
 * consecutive 16-byte... 4-byte groups of a row, so stores are fully coalesced and the two source rows
 * are read as contiguous ~5*64-byte spans per wave (L1/L2 hits for the second tap).
 */
#include "tb_internal.h"
#include "tb_device.h"

__global__ void __launch_bounds__(256)
k_resize(PlanGeom g, uint8_t* __restrict__ slab, const ResizeX* __restrict__ rx, const ResizeY* __restrict__ ry,
         int level) {
    const int b = blockIdx.y;
    const LevelGeom& D = g.lv[level];
    const int groupsPerRow = D.stride >> 2;
    const int group = blockIdx.x * blockDim.x + threadIdx.x;
    if (group >= groupsPerRow * D.h) return;
    const int dy = group / groupsPerRow;
    const int dx0 = (group - dy * groupsPerRow) << 2;

    int sstride;
    const uint8_t* src = tb_level_ptr(g, slab, b, level - 1, &sstride);
    uint8_t* dst = slab + (size_t)b * g.slabBytes + D.off + (size_t)dy * D.stride;

    const ResizeY yy = ry[dy];
    const uint8_t* S0 = src + (size_t)yy.sy0 * sstride;
    const uint8_t* S1 = src + (size_t)yy.sy1 * sstride;
    const int b0 = yy.b0, b1 = yy.b1;
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int dx = dx0 + i;
        if (dx < D.w) {
            const ResizeX xx = rx[dx];
            const int r0 = S0[xx.sx] * xx.a0 + S0[xx.sx1] * xx.a1;
            const int r1 = S1[xx.sx] * xx.a0 + S1[xx.sx1] * xx.a1;
            int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
            v = min(max(v, 0), 255);
            packed |= (uint32_t)v << (8 * i);
        }
    }
    *reinterpret_cast<uint32_t*>(dst + dx0) = packed;
}

/* LDS-staged variant: one wavefront per tile of 256 x RS_ROWS destination pixels.
 *
 * Staging. Every source row the tile needs goes to LDS once, in units of U bytes (WIDE: 16, source base and stride 16-byte
 * aligned; else 4, caller-owned level 0 with a 4-byte aligned stride). One buffer resource per tile: base = (first source row,
 * first source column rounded down to U), bounded by the end of the last source row the tile needs, so units below that row read
 * as zero without touching memory; no exec-mask branches, no 64-bit addresses. An LDS row holds S = rowBytes / U units, the same
 * for every tile of a launch: unit idx of the tile is row idx / S (one multiply by the launcher's reciprocal), its LDS address is
 * U * idx and its source offset row * sstride + U * (idx - row * S). Units right of the tile's last source column get an offset
 * outside the bound (one select), so a narrow last tile fetches no more than it reads. Any number of rows takes rounds of RS_NLD
 * loads per lane, all of a round in flight before its first LDS store.
 *
 * Horizontal pass. The lane's four coefficient entries stay in registers across the tile's rows; the 8 taps of a row are LDS
 * byte reads, S[sx] a0 + S[sx1] a1 one 24-bit multiply and one 24-bit multiply-add. Ranges: pixels <= 255; a0, a1, b0, b1 <= 2049
 * with a0 + a1, b0 + b1 in 2047..2049 (each coefficient rounded on its own), so h <= 32 655 and b h < 2^27. (Fetching the taps as
 * three aligned dwords and picking them with v_alignbyte_b32 / v_perm_b32 / v_dot2_u32_u16 measured 7 % slower: DESIGN.md 8.)
 *
 * Vertical blend. (b h) >> 16 is v_mul_hi_u32 of h with b << 16 (b wave-uniform; the 32-bit multiplies issue at the rate of the
 * 24-bit ones, profiles/int_ops_mul.json, and this form needs no shift). No clamp: ((b0 h0) >> 16) + ((b1 h1) >> 16)
 * <= 1020, the result is 0..255 as it stands. All four pixels of a lane are computed (the coefficient loads clamp dx); the bytes
 * at columns >= w are cleared by one AND with a per-lane mask, so bytes in [w, stride) stay zero. The store is a buffer store
 * with a 32-bit offset from the tile's first byte; lanes right of the stride carry an offset outside the bound. */
#define RS_ROWS 8
#define RS_NLD 6 /* loads per lane and round: 6 x 64 units of 16 bytes hold the 14 x 21 units of a tile at scale 0.8 */

typedef unsigned int rs_u4 __attribute__((ext_vector_type(4)));

template <bool WIDE>
__global__ void __launch_bounds__(64)
k_resize_lds(PlanGeom g, uint8_t* __restrict__ slab, const ResizeX* __restrict__ rx, const ResizeY* __restrict__ ry,
             int level, int rowBytes, int srows, unsigned recip, int nImages, int by_image, int tilesX, int tilesY) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];
    /* workgroup -> (image, tile). by_image (batches): 1-D grid, XCD k (workgroup id mod 8) takes images k, k + 8, ... tile by
     * tile: vertically adjacent tiles share up to 5 of their 13 source rows, through ONE L2 this way. */
    int b, tx, ty;
    if (by_image) {
        const unsigned L = blockIdx.x, j = L >> 3, T = (unsigned)(tilesX * tilesY), grp = j / T, t = j - grp * T;
        b = (int)(grp * 8u + (L & 7u));
        if (b >= nImages) return;
        ty = (int)(t / (unsigned)tilesX); tx = (int)(t - (unsigned)ty * (unsigned)tilesX);
    } else {
        b = blockIdx.z; tx = blockIdx.x; ty = blockIdx.y;
    }
    constexpr int U = WIDE ? 16 : 4;
    const int dy0 = ty * RS_ROWS, lane = threadIdx.x;
    const LevelGeom& D = g.lv[level];
    const int X0 = tx * 256;
    int sstride;
    const uint8_t* src = tb_level_ptr(g, slab, b, level - 1, &sstride);
    const int dy1 = min(dy0 + RS_ROWS, D.h) - 1;
    const int xl = min(X0 + 255, D.w - 1);
    const int sxa = rx[min(X0, D.w - 1)].sx & ~(U - 1), sxb = rx[xl].sx1;
    /* the tile's ResizeY entries, once (wave-uniform: scalar loads) */
    ResizeY yy[RS_ROWS];
#pragma unroll
    for (int k = 0; k < RS_ROWS; k++) yy[k] = ry[min(dy0 + k, dy1)];
    const int sya = yy[0].sy0;
    const int S = rowBytes / U;
    const int nrows = min(yy[RS_ROWS - 1].sy1 - sya + 1, srows);     /* srows: what the launcher sized the LDS for */
    const int total = nrows * S;
    const int nseg = min((sxb - sxa) / U + 1, S);                    /* units of a row this tile reads */
    {
        const int rowEnd = (g.lv[level - 1].w + U - 1) & ~(U - 1);   /* <= sstride (launcher) */
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(src) + (size_t)sya * sstride + sxa, 0, (nrows - 1) * sstride + rowEnd - sxa, 0x00020000);
        for (int i0 = 0; i0 < total; i0 += 64 * RS_NLD) {
            if constexpr (WIDE) {
                rs_u4 v[RS_NLD];
#pragma unroll
                for (int k = 0; k < RS_NLD; k++) {
                    const unsigned idx = (unsigned)(i0 + 64 * k + lane), row = (idx * recip) >> 22, seg = idx - row * (unsigned)S;   /* idx / S */
                    v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, seg < (unsigned)nseg ? (int)row * sstride + U * (int)seg : 0x7ffffff0, 0, 0);
                }
#pragma unroll
                for (int k = 0; k < RS_NLD; k++) {
                    const int idx = i0 + 64 * k + lane;
                    if (idx < total) *reinterpret_cast<rs_u4*>(rows + U * idx) = v[k];
                }
            } else {
                uint32_t v[RS_NLD];
#pragma unroll
                for (int k = 0; k < RS_NLD; k++) {
                    const unsigned idx = (unsigned)(i0 + 64 * k + lane), row = (idx * recip) >> 22, seg = idx - row * (unsigned)S;
                    v[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, seg < (unsigned)nseg ? (int)row * sstride + U * (int)seg : 0x7ffffff0, 0, 0);
                }
#pragma unroll
                for (int k = 0; k < RS_NLD; k++) {
                    const int idx = i0 + 64 * k + lane;
                    if (idx < total) *reinterpret_cast<uint32_t*>(rows + U * idx) = v[k];
                }
            }
        }
    }
    const int dx0 = X0 + 4 * lane;
    /* the lane's four coefficient entries stay in registers across the tile's rows; tap offsets are relative to the LDS row */
    int o0[4], o1[4];
    uint32_t a0[4], a1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const ResizeX xx = rx[min(dx0 + i, D.w - 1)];
        o0[i] = xx.sx - sxa; o1[i] = xx.sx1 - sxa; a0[i] = (uint32_t)xx.a0; a1[i] = (uint32_t)xx.a1;
    }
    const int nkeep = min(max(D.w - dx0, 0), 4);
    const uint32_t keep = nkeep >= 4 ? 0xffffffffu : ((1u << (8 * nkeep)) - 1u);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
        slab + (size_t)b * g.slabBytes + D.off + (size_t)dy0 * D.stride + X0, 0, (dy1 - dy0 + 1) * D.stride - X0, 0x00020000);
    const uint32_t doff = dx0 < D.stride ? 4u * lane : 0x7ffffff0u;
    __syncthreads();
    /* horizontal interpolation of one source row at the lane's four columns: (S[sx] a0 + S[sx1] a1) >> 4 */
    auto hrow = [&](int sy, uint32_t (&hh)[4]) {
        const uint8_t* R = rows + (sy - sya) * rowBytes;
#pragma unroll
        for (int i = 0; i < 4; i++) hh[i] = (__umul24(R[o0[i]], a0[i]) + __umul24(R[o1[i]], a1[i])) >> 4;
    };
    /* vertical blend + store of destination row dy0 + k */
    auto emit = [&](int k, int b0, int b1, const uint32_t (&h0)[4], const uint32_t (&h1)[4]) {
        const uint32_t B0 = (uint32_t)b0 << 16, B1 = (uint32_t)b1 << 16;
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (__umulhi(h0[i], B0) + __umulhi(h1[i], B1) + 2u) >> 2;
        const uint32_t packed = (v[0] | (v[1] << 8)) | ((v[2] | (v[3] << 8)) << 16);
        __builtin_amdgcn_raw_buffer_store_b32(packed & keep, rd, (int)((uint32_t)(k * D.stride) + doff), 0, 0);
    };
    /* two destination rows per trip: at scale 0.8 the second one's upper source row is the first one's lower row four times
     * out of five (wave-uniform test) -- three horizontal passes instead of four */
#pragma unroll
    for (int k = 0; k < RS_ROWS; k += 2) {
        if (dy0 + k > dy1) break;
        const ResizeY ya = yy[k];
        uint32_t hA[4], hB[4];
        hrow(ya.sy0, hA);
        hrow(ya.sy1, hB);
        emit(k, ya.b0, ya.b1, hA, hB);
        if (dy0 + k + 1 <= dy1) {
            const ResizeY yb = yy[k + 1];
            uint32_t hC[4];
            if (yb.sy0 == ya.sy1) {
                hrow(yb.sy1, hC);
                emit(k + 1, yb.b0, yb.b1, hB, hC);
            } else {
                hrow(yb.sy0, hA);
                hrow(yb.sy1, hC);
                emit(k + 1, yb.b0, yb.b1, hA, hC);
            }
        }
    }
}

int tbk_resize_level(tb_extractor* ex, int level, int n) {
    tb_ctx* ctx = ex->ctx;
    const LevelGeom& D = ex->g.lv[level];
    const LevelGeom& Sg = ex->g.lv[level - 1];
    /* source alignment check for the LDS-staged kernel */
    const bool ext0 = (level - 1 == 0) && ex->g.img0 != nullptr;
    const int sstride = ext0 ? ex->g.img0_stride : Sg.stride;
    const uintptr_t sbase = ext0 ? reinterpret_cast<uintptr_t>(ex->g.img0) : 0;
    const unsigned long long spitch = ext0 ? ex->g.img0_pitch : 0;
    const bool aligned = (sstride % 4 == 0) && (sbase % 4 == 0) && (spitch % 4 == 0) && (sstride >= ((Sg.w + 3) & ~3));
    const bool wide = aligned && (sstride % 16 == 0) && (sbase % 16 == 0) && (spitch % 16 == 0) && (sstride >= ((Sg.w + 15) & ~15));
    const double rx_ratio = (double)Sg.w / (double)D.w, ry_ratio = (double)Sg.h / (double)D.h;
    /* an LDS row: the tile's source span, at most ceil(255 ratio) + 1 columns apart (+ 1: the table is rounded to float) and
     * the 15 bytes the first column is rounded down by, in whole 16-byte units */
    const int rowBytes = ((int)ceil(255.0 * rx_ratio) + 2 + 15 + 15) & ~15;
    const int srows = (int)(RS_ROWS * ry_ratio) + 3;
    const size_t lds = (size_t)rowBytes * srows;
    const long long S = rowBytes / (wide ? 16 : 4);
    /* idx / S as (idx * recip) >> 22 is exact while idx * S < 2^22, and idx < srows * S + 64 * RS_NLD */
    const bool divides = (srows * S + 64 * RS_NLD) * S < (1ll << 22) && srows < 512;
    if (aligned && lds <= 48 * 1024 && divides) {
        const int tilesX = (D.stride + 255) / 256, tilesY = (D.h + RS_ROWS - 1) / RS_ROWS;
        const int by_image = n >= 64 ? 1 : 0;
        const dim3 grid = by_image ? dim3((unsigned)(tilesX * tilesY) * 8u * (unsigned)((n + 7) / 8)) : dim3(tilesX, tilesY, n);
        const unsigned recip = (unsigned)((1u << 22) / (unsigned)S + 1u);
        return tb_launch(ctx, "k_resize", wide ? k_resize_lds<true> : k_resize_lds<false>, grid, dim3(64), lds, ex->g, ex->d_slab,
                         ex->d_rx[level], ex->d_ry[level], level, rowBytes, srows, recip, n, by_image, tilesX, tilesY);
    }
    const int groups = (D.stride >> 2) * D.h;
    dim3 grid((groups + 255) / 256, n);
    return tb_launch(ctx, "k_resize", k_resize, grid, dim3(256), 0, ex->g, ex->d_slab, ex->d_rx[level], ex->d_ry[level], level);
}

/* ---- measurement helper ("confirm on the box with a device-to-device copy microbench"): 16 bytes per lane, four
 * independent loads in flight per thread, one workgroup per 16 KB tile (no loop: the dispatcher keeps the CUs fed) -- the float4
 * copy the hardware guide quotes 6.29 TB/s for. A grid-stride loop over 8 workgroups per CU with one load in flight measured
 * 5.06 TB/s. bench.py reports what it measures with this next to the 8 TB/s spec peak. */
typedef unsigned int tb_u4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256)
k_copy16(const tb_u4* __restrict__ src, tb_u4* __restrict__ dst, size_t n16) {
    const size_t i0 = (size_t)blockIdx.x * 1024 + threadIdx.x;
    tb_u4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (i0 + 256 * k < n16) ? __builtin_nontemporal_load(src + i0 + 256 * k) : (tb_u4){0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (i0 + 256 * k < n16) __builtin_nontemporal_store(v[k], dst + i0 + 256 * k);
}

int tbk_copy16(tb_ctx* ctx, const void* d_src, void* d_dst, size_t bytes) {
    const size_t n16 = bytes / 16;
    if (n16 == 0) return TB_OK;
    const unsigned blocks = (unsigned)((n16 + 1023) / 1024);
    return tb_launch(ctx, nullptr, k_copy16, dim3(blocks), dim3(256), 0, (const tb_u4*)d_src, (tb_u4*)d_dst, n16);
}

/* ---- exchange helper: the live rows of a [F][cap] record array, frame after frame, to the front of a packed
 * array -- what a rank sends in the track gather instead of capacity-sized tensors. One workgroup per frame: its offset is
 * the sum of the counts before it (F is a few hundred: every workgroup adds them up itself), then 16 bytes per lane.
 * row_bytes is a multiple of 4 (28, 32, 16). total_out[0] = all live rows. */
__global__ void __launch_bounds__(256)
k_pack_rows(const uint8_t* __restrict__ src, int row_bytes, int cap, const int32_t* __restrict__ counts, int nframes,
            uint8_t* __restrict__ dst, long long* __restrict__ total_out) {
    __shared__ long long red[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    long long before = 0, all = 0;
    for (int i = tid; i < nframes; i += 256) {
        const long long c = min(max(counts[i], 0), cap);
        all += c;
        if (i < f) before += c;
    }
    for (int pass = 0; pass < 2; pass++) {
        long long v = pass == 0 ? before : all;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        v = red[0] + red[1] + red[2] + red[3];
        if (pass == 0) before = v; else all = v;
    }
    if (f == 0 && tid == 0 && total_out) total_out[0] = all;
    const int n = min(max(counts[f], 0), cap);
    const size_t nb = (size_t)n * row_bytes;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (size_t)f * cap * row_bytes);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + (size_t)before * row_bytes);
    for (size_t i = tid; i < nb / 4; i += 256) d4[i] = s4[i];
}

int tbk_pack_rows(tb_ctx* ctx, const void* d_src, int row_bytes, int cap, const int32_t* d_counts, int nframes, void* d_dst, long long* d_total) {
    if (nframes <= 0) return TB_OK;
    return tb_launch(ctx, nullptr, k_pack_rows, dim3(nframes), dim3(256), 0, (const uint8_t*)d_src, row_bytes, cap, d_counts, nframes,
                     (uint8_t*)d_dst, d_total);
}
