/* Two-view linear triangulation with known poses (LocalBA::LinearTriangle, LocalBA.cpp:24-43), batched, with the acceptance
 * gates of include/tb_capi.h (tb_linear_triangle_batch_dev).
 *
 * One lane per point pair (the per-point code is tb_triangulate.h's tri_point, which k_two_view.hip shares), everything in
 * registers: the 4 x 4 matrices are C arrays whose every index is a compile-time constant after unrolling (tri_rotate's P, Q are
 * template arguments), so they are promoted to registers and the kernel has no scratch and no LDS. A pair's poses and K are
 * wave-uniform. float64, one operation per statement, only + - * / sqrt, in the order tests/triangulate_reference.py writes down
 * (the library builds with -ffp-contract=off). The Jacobi iteration runs a fixed number of sweeps without a convergence test: the
 * lanes of a wave stay converged and the result does not depend on a threshold. */
#include "tb_internal.h"
#include "tb_device.h"
#include "tb_triangulate.h"

#define TRI_T 256

__global__ void __launch_bounds__(TRI_T)
k_linear_triangle(const float* __restrict__ xy0, const float* __restrict__ xy1, const int32_t* __restrict__ counts, int pitch,
                  const float* __restrict__ Tcw0, const float* __restrict__ Tcw1, double fx, double fy, double cx, double cy,
                  const float* __restrict__ inv_sigma2_0, const float* __restrict__ inv_sigma2_1, const uint8_t* __restrict__ skip,
                  double cos_parallax_max, double chi2_max, float* __restrict__ points, uint8_t* __restrict__ flags,
                  int32_t* __restrict__ tally) {
    const int p = blockIdx.y, i = blockIdx.x * TRI_T + threadIdx.x;
    const int n = counts ? min(max(counts[p], 0), pitch) : pitch;
    const size_t o = (size_t)p * pitch + i;
    const bool in_row = i < pitch;
    int flag = 0;
    if (in_row && i < n && !(skip && skip[o])) {
        double T0[16], T1[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { T0[k] = (double)Tcw0[16 * p + k]; T1[k] = (double)Tcw1[16 * p + k]; }
        const double u0 = (double)xy0[2 * o], v0 = (double)xy0[2 * o + 1], u1 = (double)xy1[2 * o], v1 = (double)xy1[2 * o + 1];
        const double s0 = inv_sigma2_0 ? (double)inv_sigma2_0[o] : 1.0, s1 = inv_sigma2_1 ? (double)inv_sigma2_1[o] : 1.0;
        float Xf, Yf, Zf;
        flag = tri_point(T0, T1, u0, v0, u1, v1, s0, s1, fx, fy, cx, cy, cos_parallax_max, chi2_max, Xf, Yf, Zf);
        if (flag == 1) { points[3 * o] = Xf; points[3 * o + 1] = Yf; points[3 * o + 2] = Zf; }
    }
    if (in_row) flags[o] = (uint8_t)flag;
    /* one atomic per wavefront and code; integer sums do not depend on the order */
#pragma unroll
    for (int code = 0; code < 6; code++) {
        const int cnt = __popcll(__ballot(in_row && flag == code));
        if (tb_lane() == 0 && cnt) atomicAdd(&tally[6 * p + code], cnt);
    }
}

int tbk_linear_triangle(tb_ctx* ctx, int npairs, const float* d_xy0, const float* d_xy1, const int32_t* d_counts, int pitch,
                        const float* d_Tcw0, const float* d_Tcw1, const double K[4], const float* d_inv_sigma2_0,
                        const float* d_inv_sigma2_1, const uint8_t* d_skip, double cos_parallax_max, double chi2_max, float* d_points,
                        uint8_t* d_flags, int32_t* d_tally) {
    if (npairs <= 0) return TB_OK;
    TB_HIP(ctx, hipMemsetAsync(d_tally, 0, (size_t)npairs * 6 * sizeof(int32_t), ctx->stream));
    return tb_launch(ctx, "k_linear_triangle", k_linear_triangle, dim3((pitch + TRI_T - 1) / TRI_T, npairs), dim3(TRI_T), 0, d_xy0, d_xy1,
                     d_counts, pitch, d_Tcw0, d_Tcw1, K[0], K[1], K[2], K[3], d_inv_sigma2_0, d_inv_sigma2_1, d_skip, cos_parallax_max,
                     chi2_max, d_points, d_flags, d_tally);
}
