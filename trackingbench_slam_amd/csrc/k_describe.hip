/* a6 + a7 + a8 + a10 -- orientation, Gaussian blur and steered-BRIEF descriptor, fused per keypoint.
 *
 * Reference: IC_Angle (src/extractors/ORBextractor.cpp:17-44), GaussianBlur(7x7, sigma 2,
 * BORDER_REFLECT_101) on a clone of every level (:959-960), computeOrbDescriptor (:48-87) and the
 * coordinate rescale + level-major concatenation (:969-976).
 *
 * The reference blurs whole levels (2 x 2.48 MB of HBM traffic per 720p frame) and then gathers 512
 * taps per keypoint.  Every rotated, rounded tap lies within 18 px of the keypoint (the pattern's largest norm is
 * |(13, 13)| = 18.385, the rotation adds three float roundings, and cv_round of anything below 18.5 is at most 18:
 * tests/test_describe_reach_cpu.py), and the 8U blur is an exact integer
 * function of the 7x7 neighbourhood (kernel 18,34,49,55,49,34,18; (acc + 2^15) >> 16), so the blurred
 * 37x37 patch can be rebuilt bit-exactly from the 43x43 source patch, which also holds the orientation disc
 * (radius 15).  One wavefront per keypoint:
 *   stage 43x43 source patch in LDS (reflect-101 at level borders) -> integer moments (wave reduce) ->
 *   fastAtan2 -> separable blur in LDS (u16 intermediate is exact: 255*257 = 65535) -> 256 rotated tests,
 *   4 x 64-lane ballots = 32 descriptor bytes.
 * No blurred level is ever written to HBM.  Roofline: HBM/L2 gather of 2 KB per keypoint (SURVEY 8d
 * "orient + describe" row); VALU work ~370 multiply-adds per lane.
 */
#include "tb_internal.h"
#include "tb_device.h"

/* bit_pattern_31_ (ORBextractor.cpp:90-348) as floats, four per test (x0, y0, x1, y1): one 16-byte load per lane */
struct DsPattern { float v[1024]; };
constexpr DsPattern ds_make_pattern() {
    constexpr int8_t raw[1024] = {
#include "orb_pattern.inc"
    };
    DsPattern p{};
    for (int i = 0; i < 1024; i++) p.v[i] = (float)raw[i];
    return p;
}
__constant__ __attribute__((aligned(16))) DsPattern c_patternf = ds_make_pattern();

/* IC_Angle disc (umax[] of ORBextractor.cpp:389-404 = 15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3) as byte weights for
 * v_dot4_u32_u8: row |v| of the disc spans u in [-umax, umax]; byte i of the 32 bytes that start at u = -15 weighs
 * 1 (sum of intensities) and u + 16 (first moment, biased to stay unsigned) inside the disc, 0 outside. */
struct DsDisc { uint32_t w1[16][8], wu[16][8]; };
constexpr DsDisc ds_make_disc() {
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    DsDisc d{};
    for (int av = 0; av < 16; av++)
        for (int i = 0; i < 32; i++) {
            const int u = i - 15;
            const bool in = (u >= -umax[av]) && (u <= umax[av]);
            d.w1[av][i >> 2] |= (uint32_t)(in ? 1 : 0) << (8 * (i & 3));
            d.wu[av][i >> 2] |= (uint32_t)(in ? (u + 16) : 0) << (8 * (i & 3));
        }
    return d;
}
__constant__ __attribute__((aligned(16))) DsDisc c_disc = ds_make_disc();

#define DS_P 43      /* source patch edge: origin (kx - 21, ky - 21) */
#define DS_PS 52     /* source patch row stride: 13 dwords (odd) -> one-row-per-lane accesses hit distinct banks; 12 are used */
#define DS_B 37      /* blurred patch edge: centre (18, 18) */
#define DS_CS 46     /* h-pass COLUMN stride in u16 (23 dwords, odd): the sums are stored transposed, [column][row]; rows 43..45 are slack */
#define DS_BS 40     /* blurred patch row stride */
/* the patch buffer's three tenants: source rows (46: the staging rounds store up to three rows past the patch), h-pass columns, blurred rows
 * (40: the v-pass pieces store up to three rows past the patch) */
#define DS_BUF 3408
static_assert(DS_BUF >= 46 * DS_PS && DS_BUF >= DS_B * DS_CS * 2 && DS_BUF >= 40 * DS_BS && DS_BUF % 16 == 0, "patch buffer tenants");

typedef unsigned short ds_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int ds_reflect(int i, int n) {
    /* BORDER_REFLECT_101; n >= 2 and |overshoot| < n for every level that can hold a keypoint */
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

/* four bytes of a register array starting at byte o (compile-time o) */
__device__ __forceinline__ uint32_t ds_window(const uint32_t* w, int o) {
    return (o & 3) ? __builtin_amdgcn_alignbyte(w[(o >> 2) + 1], w[o >> 2], o & 3) : w[o >> 2];
}

__device__ __forceinline__ uint32_t ds_udot2(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(ds_u16x2, a), __builtin_bit_cast(ds_u16x2, b), c, false);
}

/* offset r * DS_BS + c of a steered tap from the patch centre: (r, c) = (rn(x b + y a), rn(x a - y b)), un-contracted
 * (ORBextractor.cpp:57-62). cv_round of a coordinate (|v| < 19) is one float add: v + 1.5 * 2^23 is rounded to nearest-even at unit
 * spacing and the sum's bit pattern is 0x4B400000 + rn(v) -- the integer v_rndne_f32 + v_cvt_i32_f32 give, from the fast issue
 * class; the low 24 bits go into the multiply-add as they are and the constants come off once */
__device__ __forceinline__ int ds_tap(float x, float y, float a, float b) {
    const float r = TB_FADD(TB_FMUL(x, b), TB_FMUL(y, a)), c = TB_FSUB(TB_FMUL(x, a), TB_FMUL(y, b));
    constexpr uint32_t M = 0x4B400000u;
    const uint32_t br = __builtin_bit_cast(uint32_t, TB_FADD(r, 12582912.0f)), bc = __builtin_bit_cast(uint32_t, TB_FADD(c, 12582912.0f));
    return (int)((uint32_t)__mul24((int)br, DS_BS) + bc - ((M & 0xffffffu) * DS_BS + M));
}

/* horizontal 7-tap pass of one patch row held in 12 dwords, patch column 0 at byte SH: 37 exact u16 sums
 * (18,34,49,55,49,34,18; at most 255 * 257 = 65535) as two v_dot4_u32_u8 each, stored down the row's place in every column
 * (out[c * DS_CS]). The K1 products of a group of outputs are issued before their K2 accumulations: a dependent v_dot4 pair
 * back to back costs a wait state. */
template <int SH>
__device__ __forceinline__ void ds_hrow(const uint32_t* w, unsigned short* out) {
    constexpr uint32_t K1 = 18u | (34u << 8) | (49u << 16) | (55u << 24), K2 = 49u | (34u << 8) | (18u << 16);
    constexpr int GRP = 8;
#pragma unroll
    for (int c0 = 0; c0 < DS_B; c0 += GRP) {
        uint32_t a[GRP];
#pragma unroll
        for (int i = 0; i < GRP; i++)
            if (c0 + i < DS_B) a[i] = __builtin_amdgcn_udot4(ds_window(w, c0 + i + SH), K1, 0u, false);
#pragma unroll
        for (int i = 0; i < GRP; i++)
            if (c0 + i < DS_B) a[i] = __builtin_amdgcn_udot4(ds_window(w, c0 + i + SH + 4), K2, a[i], false);
#pragma unroll
        for (int i = 0; i < GRP; i++)
            if (c0 + i < DS_B) out[(c0 + i) * DS_CS] = (unsigned short)a[i];
    }
}

/* vertical 7-tap pass of N outputs of one column whose first h-pass row is even: P[k] = the column's u16 sums of rows
 * (r0 + 2k, r0 + 2k + 1) as they lie in LDS, ((N - 1) >> 1) + 4 of them. The kernel is symmetric, so both output parities are
 * four v_dot2_u32_u16 on these even-aligned pairs (exact 32-bit accumulation), (acc + 2^15) >> 16 saturated (the kernel sums
 * to 257):
 *   j = 2m:     P[m].(18,34) + P[m+1].(49,55) + P[m+2].(49,34) + P[m+3].(18, 0)
 *   j = 2m + 1: P[m].( 0,18) + P[m+1].(34,49) + P[m+2].(55,49) + P[m+3].(34,18) */
template <int N>
__device__ __forceinline__ void ds_vcol(const uint32_t* P, uint8_t* out) {
    constexpr uint32_t KE[4] = {18u | (34u << 16), 49u | (55u << 16), 49u | (34u << 16), 18u};
    constexpr uint32_t KO[4] = {18u << 16, 34u | (49u << 16), 55u | (49u << 16), 34u | (18u << 16)};
    constexpr int GRP = 8;     /* outputs whose four dependent dots are issued stage by stage: no wait state between them */
#pragma unroll
    for (int j0 = 0; j0 < N; j0 += GRP) {
        uint32_t acc[GRP];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int i = 0; i < GRP; i++) {
                const int j = j0 + i;
                if (j < N) acc[i] = ds_udot2(P[(j >> 1) + k], (j & 1) ? KO[k] : KE[k], k ? acc[i] : (1u << 15));
            }
#pragma unroll
        for (int i = 0; i < GRP; i++)
            if (j0 + i < N) acc[i] = min(acc[i] >> 16, 255u);
#pragma unroll
        for (int i = 0; i < GRP; i++)
            if (j0 + i < N) out[(j0 + i) * DS_BS] = (uint8_t)acc[i];   /* rows past the patch land in the spare rows of bl[] */
    }
}

/* Instruction budget per keypoint (one wavefront), the quantity this kernel is bound by (~1080 vector instructions in
 * round 1, blur passes 51 % of them):
 *   staging   interior keypoints copy the patch rows as 12 aligned dwords each through a buffer resource (32-bit offsets,
 *             out-of-range rows read zero; the sub-dword phase of the patch is kept as a column shift), border keypoints
 *             take the per-byte reflect-101 path;
 *   moments   one lane per disc row: eight 4-byte windows against the disc's weight table, 16 v_dot4_u32_u8;
 *   h-pass    one lane per patch ROW: 12 dword reads, 37 outputs of two v_dot4_u32_u8 each (4 multiply-adds per
 *             instruction on the packed bytes), fully unrolled, stored transposed;
 *   v-pass    the 37 x 37 outputs over ALL lanes: columns 0-31 as two column segments of 19 rows per lane (row 18 twice),
 *             then columns 32-36 as ten 4-row pieces on 50 lanes; the operands are dword reads of row pairs, four
 *             v_dot2_u32_u16 per output and no pairing instruction;
 *   tests     4 x 64 rotated comparisons -> 4 ballots. */
#define DS_KPB 4     /* keypoints (wavefronts) per workgroup */

__device__ __forceinline__ void ds_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__global__ void __launch_bounds__(64 * DS_KPB)
k_describe(PlanGeom g, const uint8_t* __restrict__ slab, const uint32_t* __restrict__ sel,
           const int32_t* __restrict__ selCount, tb_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
           int32_t* __restrict__ counts, int nImages, int by_image, int slotGroups) {
    /* ONE patch buffer per keypoint, three tenants in turn: the source patch (rows of 52 bytes, 48 used), the h-pass sums (u16,
     * transposed: columns of 92 bytes), the blurred patch (40-byte rows). All of a wavefront's loads of one tenant complete before
     * its first store of the next (ds_wave_fence). 3.4 KB per keypoint instead of 7.7 as three arrays: the kernel's occupancy was
     * bound by LDS (20 -> 32 wavefronts per CU, now the register limit). */
    __shared__ __attribute__((aligned(16))) uint8_t buf_[DS_KPB][DS_BUF];
    __shared__ int mom[DS_KPB][2];
    __shared__ float rot[DS_KPB][4];
    /* A workgroup = DS_KPB wavefronts = DS_KPB consecutive slots of one image, one keypoint per wavefront with its own patch
     * buffers. The wavefronts meet twice: the orientation of a keypoint (fastAtan2, then sinf / cosf in the double-precision form
     * that matches glibc bit for bit: ~100 wave-uniform vector instructions, an eighth of the kernel when every wavefront ran
     * them on 64 identical lanes) is computed for all DS_KPB keypoints at once on DS_KPB lanes of wavefront 0, while the others are in
     * their blur passes.
     * workgroup -> (image, slot group). by_image (batches): a 1-D grid in which XCD k (workgroup id mod 8) takes images k, k + 8,
     * ... group by group, so that all patch gathers of an image go through ONE L2 (its pyramid, 2.5 MB at 1280x720, fits the
     * 4 MB); otherwise (group, image) order, every XCD works on every image. */
    int b, sg;
    if (by_image) {
        const unsigned L = blockIdx.x, j = L >> 3, grp = j / (unsigned)slotGroups;
        sg = (int)(j - grp * (unsigned)slotGroups);
        b = (int)(grp * 8u + (L & 7u));
        if (b >= nImages) return;
    } else {
        b = blockIdx.y; sg = blockIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = sg * DS_KPB + wave;
    uint8_t* const src = buf_[wave];
    unsigned short* const hp = reinterpret_cast<unsigned short*>(buf_[wave]);
    uint8_t* const bl = buf_[wave];
    const int32_t* sc = selCount + b * TB_MAX_LEVELS;
    /* slot -> (level, index), level-major output base */
    int level = 0, base = 0;
    for (int l = 0; l < g.nlevels; l++) {
        if (slot >= g.lv[l].selBase) level = l;
    }
    for (int l = 0; l < level; l++) base += sc[l];
    if (slot == 0 && lane == 0) {
        int tot = 0;
        for (int l = 0; l < g.nlevels; l++) tot += sc[l];
        counts[b] = tot;
    }
    const LevelGeom& G = g.lv[level];
    const int idx = slot - G.selBase;
    const bool active = slot < g.selCap && idx < sc[level];      /* wave-uniform; idle wavefronts still meet the barriers */
    uint32_t rec = 0;
    int kx = 0, ky = 0, sh = 0;
    if (active) {
        rec = sel[(size_t)b * g.selCap + slot];
        kx = (int)(rec & 0xfff) + TB_BORDER; ky = (int)((rec >> 12) & 0xfff) + TB_BORDER;
        int stride;
        const uint8_t* img = tb_level_ptr(g, slab, b, level, &stride);

        /* 1. stage the source patch: patch column c lives at LDS column c + sh */
        const int x0 = kx - 21, y0 = ky - 21;
        const bool interior = x0 >= 0 && y0 >= 0 && kx + 21 < G.w && ky + 21 < G.h && ((stride & 3) == 0) &&
                              ((reinterpret_cast<uintptr_t>(img) & 3) == 0) && ((x0 & ~3) + 48 <= stride);
        sh = interior ? (x0 & 3) : 0;
        if (interior) {
            /* 9 rounds of 5 rows x 12 dwords. One buffer resource per keypoint, base = the patch's first aligned dword, bounded by
             * the end of the 12th dword of patch row 42: rows 43..45 of the last round read zero without touching memory, and
             * the offsets are 32 bits wide. Lanes 60..63 (row 5 of a round) repeat the first dwords of the next round's first row;
             * every lane stores what it loaded (rows 43..45 go to the buffer's slack), so neither loads nor stores need a predicate. */
            const int rr = (lane * 5462) >> 16, dd = lane - rr * 12;     /* lane / 12 */
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(img) + (size_t)y0 * stride + (x0 & ~3), 0, (DS_P - 1) * stride + 48, 0x00020000);
            const int off = rr * stride + 4 * dd;
            uint32_t v[9];
#pragma unroll
            for (int j = 0; j < 9; j++) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 5 * j * stride, 0, 0);
#pragma unroll
            for (int j = 0; j < 9; j++) *reinterpret_cast<uint32_t*>(src + (5 * j + rr) * DS_PS + 4 * dd) = v[j];
        } else {
            for (int e = lane; e < DS_P * DS_P; e += 64) {
                const int r = e / DS_P, c = e - r * DS_P;
                const int yy = ds_reflect(y0 + r, G.h), xx = ds_reflect(x0 + c, G.w);
                src[r * DS_PS + c] = img[(size_t)yy * stride + xx];
            }
        }
        ds_wave_fence();

        /* 2. IC_Angle: integer moments over the radius-15 disc, lane = disc row v = lane - 15 */
        int m10 = 0, m01 = 0;
        if (lane < 31) {
            const int v = lane - 15, av = v < 0 ? -v : v;
            const int o = 6 + sh;                                  /* byte of u = -15 in the row (patch column 21 - 15) */
            const uint32_t* rw = reinterpret_cast<const uint32_t*>(src + (21 + v) * DS_PS) + (o >> 2);
            const uint4* t1 = reinterpret_cast<const uint4*>(c_disc.w1[av]);
            const uint4* tu = reinterpret_cast<const uint4*>(c_disc.wu[av]);
            const uint4 a0 = t1[0], a1 = t1[1], u0 = tu[0], u1 = tu[1];
            const uint32_t w1[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const uint32_t wu[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
            uint32_t w[9];
#pragma unroll
            for (int k = 0; k < 9; k++) w[k] = rw[k];
            uint32_t sI = 0, sW = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t X = __builtin_amdgcn_alignbyte(w[k + 1], w[k], (uint32_t)(o & 3));
                sI = __builtin_amdgcn_udot4(X, w1[k], sI, false);
                sW = __builtin_amdgcn_udot4(X, wu[k], sW, false);
            }
            m10 = (int)sW - 16 * (int)sI;    /* sum u I = sum (u + 16) I - 16 sum I */
            m01 = v * (int)sI;
        }
        m10 = tb_wave_incl_scan_dpp(m10);
        m01 = tb_wave_incl_scan_dpp(m01);
        if (lane == 63) { mom[wave][0] = m10; mom[wave][1] = m01; }
    }
    __syncthreads();

    /* 2b. orientations of the workgroup's keypoints, one lane each (ORBextractor.cpp:43, :52-55) */
    if (wave == 0 && lane < DS_KPB) {
        const float angle = tbm::fast_atan2((float)mom[lane][1], (float)mom[lane][0]);
        const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
        float a, bsin;
        tbm::sincosf_rn(TB_FMUL(angle, factorPI), &bsin, &a);
        rot[lane][0] = angle; rot[lane][1] = a; rot[lane][2] = bsin;
    }

    /* the lane's four tests (x0, y0, x1, y1): in flight across the blur passes */
    float4 pt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pt[j] = reinterpret_cast<const float4*>(c_patternf.v)[j * 64 + lane];
    if (active) {
        /* 3a. horizontal 7-tap pass, one lane per patch row (exact integers, u16 result); the sums overwrite other lanes' source
         * rows, so every lane has its row in registers first */
        {
            const uint32_t* rw = reinterpret_cast<const uint32_t*>(src + min(lane, DS_P - 1) * DS_PS);
            uint32_t w[12];
#pragma unroll
            for (int j = 0; j < 12; j++) w[j] = rw[j];
            ds_wave_fence();
            if (lane < DS_P) {
                unsigned short* out = hp + lane;
                /* the sub-dword phase of the patch: four code paths with compile-time byte offsets */
                if (sh == 0) ds_hrow<0>(w, out); else if (sh == 1) ds_hrow<1>(w, out); else if (sh == 2) ds_hrow<2>(w, out); else ds_hrow<3>(w, out);
            }
        }
        ds_wave_fence();
        /* 3b. vertical pass over all 64 lanes: all operands first (the outputs overwrite them) */
        {
            /* columns 0..31: lane = (column, upper / lower segment): rows [0, 19) and [18, 37), 25 h-pass rows = 13 pairs each
             * (the 26th row is weighed with 0) */
            const int c = lane & 31, r0 = 18 * (lane >> 5);
            /* columns 32..36: lane = (column, one of ten 4-row pieces): 10 h-pass rows = 5 pairs; lanes 50..63 repeat lane 49 */
            const int l2 = min(lane, 49), pc = (l2 * 205) >> 10, c2 = 32 + l2 - 5 * pc, q0 = 4 * pc;     /* l2 / 5 */
            const uint32_t* p1 = reinterpret_cast<const uint32_t*>(hp + c * DS_CS + r0);
            const uint32_t* p2 = reinterpret_cast<const uint32_t*>(hp + c2 * DS_CS + q0);
            uint32_t P[13], P2[5];
#pragma unroll
            for (int i = 0; i < 13; i++) P[i] = p1[i];
#pragma unroll
            for (int i = 0; i < 5; i++) P2[i] = p2[i];
            ds_wave_fence();
            ds_vcol<19>(P, bl + r0 * DS_BS + c);
            ds_vcol<4>(P2, bl + q0 * DS_BS + c2);         /* the last piece's rows 37..39 are the spare rows */
        }
    }
    __syncthreads();
    if (!active) return;

    /* 4. steered BRIEF, ORBextractor.cpp:52-84 */
    const float angle = rot[wave][0], a = rot[wave][1], bsin = rot[wave][2];
    const uint8_t* center = bl + 18 * DS_BS + 18;
    const size_t out = (size_t)b * g.selCap + base + idx;
    unsigned long long* d64 = reinterpret_cast<unsigned long long*>(desc + out * 32);
    unsigned long long bits[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int t0 = center[ds_tap(pt[j].x, pt[j].y, a, bsin)], t1 = center[ds_tap(pt[j].z, pt[j].w, a, bsin)];
        bits[j] = __ballot(t0 < t1);
    }

    /* 5. descriptor and keypoint record; coordinates scaled by sf[level] for level != 0 (ORBextractor.cpp:969-974) */
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) d64[j] = bits[j];
        tb_keypoint kp;
        kp.x = (float)kx;
        kp.y = (float)ky;
        if (level != 0) {
            kp.x = TB_FMUL(kp.x, G.sf);
            kp.y = TB_FMUL(kp.y, G.sf);
        }
        kp.size = G.patchSize;
        kp.angle = angle;
        kp.response = (float)(rec >> 24);
        kp.octave = level;
        kp.class_id = -1;
        kps[out] = kp;
    }
}

int tbk_describe(tb_extractor* ex, int n) {
    tb_ctx* ctx = ex->ctx;
    const int by_image = n >= 64 ? 1 : 0;
    const int slotGroups = (ex->g.selCap + DS_KPB - 1) / DS_KPB;
    const dim3 grid = by_image ? dim3((unsigned)slotGroups * 8u * (unsigned)((n + 7) / 8)) : dim3(slotGroups, n);
    return tb_launch(ctx, "k_describe", k_describe, grid, dim3(64 * DS_KPB), 0, ex->g, ex->d_slab, ex->d_sel, ex->d_selCount, ex->d_kps,
                     ex->d_desc, ex->d_counts, n, by_image, slotGroups);
}
