/* The depth filter (tb_depth_filter_*, include/tb_capi.h): epipolar ZMSSD search, 1-D alignment and the Gaussian x Beta seed
 * update, held statement for statement to tests/depth_filter_reference.py. FP64, one rounding per statement (the library is built
 * with -ffp-contract=off), sums left to right.
 *
 * k_df_update  one wavefront per entry, lane = pixel (ly, lx) = (lane / 8, lane % 8) of the 8 x 8 patch, four entries per
 *              256-thread workgroup, grid (ceil(pitch / 4), sequences of the launch). The entry index is read through
 *              readfirstlane, so the seed, both poses and every decision are wave-uniform: an entry that is not active leaves
 *              after one load, and the four waves of a group never meet (no barrier, no LDS, no atomics). Steps 1, 2, 6, 7, 8 are
 *              computed by every lane redundantly; lane 0 stores. A lane samples its own pixel of the warped patch and its
 *              four neighbours (the border is only ever read as a neighbour), so the patch is not exchanged. The search's
 *              score is 64 sum(D^2) - (sum D)^2 with D = A - B per pixel: the definition's 64 (sum AA - 2 sum AB + sum BB) -
 *              (sum A - sum B)^2 as integers, with two wave sums a sample in place of three. Align1D's three float64 sums an
 *              iteration take the definition's butterfly p[t] = p[t] + p[t ^ d], d = 1 .. 32.
 * k_df_add     one workgroup per sequence: the seeds bound to the slot the ring takes next are dropped, the entries that are
 *              free or dropped are listed in ascending order and the offered keys that are not skipped take them in key order
 *              (two ordered compactions, tb_block_ordered_slot).
 * k_df_copy    the keyframe's image into the ring slot k_df_add chose.
 * k_df_points  world points and flags of the converged entries; release frees them.
 */
#include "tb_device.h"

struct DfGeom {
    int pitch, R, W, H;
    int max_steps, zmssd_max, align_iters, pad_;
    double fx, fy, cx, cy, conv_div, px_err;
};

#define DF_HALF 5.0

__device__ __forceinline__ double df_wave_sum_d(double v) {
#pragma unroll
    for (int d = 1; d < TB_WAVE; d <<= 1) v = v + __shfl_xor(v, d, TB_WAVE);
    return v;
}

/* pixel (x, y) of the warped 10 x 10 patch: floor of the bilinear sample, 0 outside (step 3) */
__device__ __forceinline__ int df_patch(const uint8_t* ref, int W, int H, double u, double v, double I00, double I01, double I10,
                                        double I11, int x, int y) {
    const double dx = (double)(x - 5), dy = (double)(y - 5);
    const double px = I00 * dx + I01 * dy + u;
    const double py = I10 * dx + I11 * dy + v;
    if (!(px >= 0.0 && py >= 0.0 && px < (double)W - 1.0 && py < (double)H - 1.0)) return 0;
    const double fu = floor(px), fv = floor(py);
    const int iu = (int)fu, iv = (int)fv;
    const double su = px - fu, sv = py - fv;
    const double w00 = (1.0 - su) * (1.0 - sv);
    const double w01 = (1.0 - su) * sv;
    const double w10 = su * (1.0 - sv);
    const double w11 = 1.0 - w00 - w01 - w10;
    const uint8_t* p = ref + (size_t)iv * W + iu;
    const double val = w00 * (double)p[0] + w01 * (double)p[W] + w10 * (double)p[1] + w11 * (double)p[W + 1];
    return (int)fmin(floor(val), 255.0);
}

struct DfRay { double x, y, z; };
__device__ __forceinline__ DfRay df_unit_ray(double u, double v, const DfGeom& g) {
    const double x = (u - g.cx) / g.fx;
    const double y = (v - g.cy) / g.fy;
    const double nrm = sqrt(x * x + y * y + 1.0);
    DfRay f;
    f.x = x / nrm; f.y = y / nrm; f.z = 1.0 / nrm;
    return f;
}

__device__ __forceinline__ double df_acos(double x) { return acos(fmin(1.0, fmax(-1.0, x))); }

enum { DF_IDLE = -1, DF_UPDATED = 0, DF_BEHIND = 1, DF_OUTSIDE = 2, DF_WARP = 3, DF_DEGENERATE = 4, DF_NO_MATCH = 5, DF_CONVERGED = 6,
       DF_NONFINITE = 7 };

__global__ __launch_bounds__(256) void k_df_update(DfGeom g, int seq0, tb_df_seed* seeds, tb_df_trace* traces, const uint8_t* ring,
                                                   const float* ring_Tcw, const uint8_t* images, int stride, size_t image_pitch,
                                                   const float* Tcw) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = seq0 + blockIdx.y;
    if (e >= g.pitch) return;
    tb_df_seed* sp = seeds + (size_t)s * g.pitch + e;
    tb_df_trace* tp = traces + (size_t)s * g.pitch + e;
    const int slot = sp->slot;
    tb_df_trace tr;
    tr.score = -1; tr.px = 0.0; tr.py = 0.0; tr.z = 0.0; tr.tau = 0.0; tr.flag = DF_IDLE; tr.n = 0; tr.win = -1; tr.reserved = 0;
    if (sp->state != 1 || (unsigned)slot >= (unsigned)g.R) {
        if (lane == 0) *tp = tr;
        return;
    }
    const double mu = sp->mu, sigma2 = sp->sigma2, a = sp->a, b = sp->b, z_range = sp->z_range;
    const double u = (double)sp->u, v = (double)sp->v;
    const int updates = sp->updates;
    const int W = g.W, H = g.H;
    const double fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy;
    const uint8_t* ref = ring + ((size_t)s * g.R + slot) * ((size_t)W * H);
    const uint8_t* cur = images + (size_t)s * image_pitch;
    const int lx = lane & 7, ly = lane >> 3;

    /* T_cr = Tcw Tcw_ref^-1: R = Rc Rr', t = tc - R tr */
    double R[3][3], t[3];
    {
        const float* Tr = ring_Tcw + ((size_t)s * g.R + slot) * 16;
        const float* Tc = Tcw + (size_t)s * 16;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                R[i][j] = (double)Tc[i * 4 + 0] * (double)Tr[j * 4 + 0] + (double)Tc[i * 4 + 1] * (double)Tr[j * 4 + 1] +
                          (double)Tc[i * 4 + 2] * (double)Tr[j * 4 + 2];
            t[i] = (double)Tc[i * 4 + 3] - (R[i][0] * (double)Tr[3] + R[i][1] * (double)Tr[7] + R[i][2] * (double)Tr[11]);
        }
    }
    const DfRay f = df_unit_ray(u, v, g);
    double Rf[3];
#pragma unroll
    for (int i = 0; i < 3; i++) Rf[i] = R[i][0] * f.x + R[i][1] * f.y + R[i][2] * f.z;

    int flag = DF_UPDATED;
    double n_mu = mu, n_sigma2 = sigma2, n_a = a, n_b = b;
    int n_state = 1;
    bool changed = false;
    do {
        /* 1. range ends */
        const double sd = sqrt(sigma2);
        const double d = 1.0 / mu;
        const double d_min = 1.0 / (mu + sd);
        const double d_max = 1.0 / fmax(mu - sd, 1e-8);
        double P0[3], P1[3], P2[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            P0[i] = Rf[i] * d + t[i];
            P1[i] = Rf[i] * d_min + t[i];
            P2[i] = Rf[i] * d_max + t[i];
        }
        if (!(P0[2] > 0.0 && P1[2] > 0.0 && P2[2] > 0.0)) { flag = DF_BEHIND; break; }
        const double Ax = P1[0] / P1[2], Ay = P1[1] / P1[2];
        const double Bx = P2[0] / P2[2], By = P2[1] / P2[2];
        const double uc = fx * (P0[0] / P0[2]) + cx;
        const double vc = fy * (P0[1] / P0[2]) + cy;
        if (!(uc >= 5.0 && vc >= 5.0 && uc < (double)W - 5.0 && vc < (double)H - 5.0)) { flag = DF_OUTSIDE; break; }
        /* 2. affine warp at d */
        double A00, A01, A10, A11;
        {
            const double X[3] = {f.x * d, f.y * d, f.z * d};
            const double zr = X[2];
            const double xu = (u + DF_HALF - cx) / fx, yu = (v - cy) / fy;
            const double xv = (u - cx) / fx, yv = (v + DF_HALF - cy) / fy;
            const double Xu[3] = {xu * zr, yu * zr, zr};
            const double Xv[3] = {xv * zr, yv * zr, zr};
            double pu[3], pv[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double* Pk = k == 0 ? X : (k == 1 ? Xu : Xv);
                double Q[3];
#pragma unroll
                for (int i = 0; i < 3; i++) Q[i] = R[i][0] * Pk[0] + R[i][1] * Pk[1] + R[i][2] * Pk[2];
#pragma unroll
                for (int i = 0; i < 3; i++) Q[i] = Q[i] + t[i];
                pu[k] = fx * (Q[0] / Q[2]) + cx;
                pv[k] = fy * (Q[1] / Q[2]) + cy;
            }
            A00 = (pu[1] - pu[0]) / DF_HALF;
            A01 = (pu[2] - pu[0]) / DF_HALF;
            A10 = (pv[1] - pv[0]) / DF_HALF;
            A11 = (pv[2] - pv[0]) / DF_HALF;
        }
        const double det = A00 * A11 - A01 * A10;
        if (!(det > 1.0 / 3.0 && det < 3.0)) { flag = DF_WARP; break; }
        const double I00 = A11 / det, I01 = -A01 / det, I10 = -A10 / det, I11 = A00 / det;
        /* 3. this lane's pixel of the warped patch and its four neighbours */
        const int pc = df_patch(ref, W, H, u, v, I00, I01, I10, I11, lx + 1, ly + 1);
        const int pl = df_patch(ref, W, H, u, v, I00, I01, I10, I11, lx, ly + 1);
        const int pr = df_patch(ref, W, H, u, v, I00, I01, I10, I11, lx + 2, ly + 1);
        const int pt = df_patch(ref, W, H, u, v, I00, I01, I10, I11, lx + 1, ly);
        const int pb = df_patch(ref, W, H, u, v, I00, I01, I10, I11, lx + 1, ly + 2);
        /* 4. epipolar search */
        const double ax = fx * Ax + cx, ay = fy * Ay + cy;
        const double bx = fx * Bx + cx, by = fy * By + cy;
        const double ex = ax - bx, ey = ay - by;
        const double epi_len = sqrt(ex * ex + ey * ey);
        if (!(epi_len >= 1e-6)) { flag = DF_DEGENERATE; break; }
        const double nd = fmax(1.0, floor(epi_len / 0.7));
        tr.n = (int)fmin(nd, 2147483647.0);
        if (nd > (double)g.max_steps) { flag = DF_NO_MATCH; break; }
        const int n = (int)nd;
        int win = -1, wu = 0, wv = 0;
        long long best = -1;
        {
            const double dAx = Ax - Bx, dAy = Ay - By;
            double ppu = -1.0, ppv = -1.0;   /* the previous sample's pixel; no pixel that is scored has a negative coordinate */
            for (int i = 0; i <= n; i++) {
                const double tt = (double)i / nd;
                const double x = Bx + tt * dAx;
                const double y = By + tt * dAy;
                const double pu = floor(fx * x + cx + 0.5);
                const double pv = floor(fy * y + cy + 0.5);
                const bool same = i > 0 && pu == ppu && pv == ppv;
                ppu = pu; ppv = pv;
                if (same) continue;
                if (!(pu >= 4.0 && pv >= 4.0 && pu <= (double)W - 1.0 - 4.0 && pv <= (double)H - 1.0 - 4.0)) continue;
                const int iu = (int)pu, iv = (int)pv;
                const int D = pc - (int)cur[(size_t)(iv - 4 + ly) * stride + (iu - 4 + lx)];
                const int sD = tb_wave_sum(D), sDD = tb_wave_sum(D * D);
                const long long sc = 64LL * sDD - (long long)sD * sD;
                if (win < 0 || sc < best) { win = i; best = sc; wu = iu; wv = iv; }
            }
        }
        tr.win = win;
        tr.score = best;
        if (win < 0 || best >= 64LL * g.zmssd_max) { flag = DF_NO_MATCH; break; }
        /* 5. Align1D along the line's unit pixel direction */
        const double dirx = ex / epi_len, diry = ey / epi_len;
        double au = (double)wu, av = (double)wv;
        bool conv = false;
        {
            const double refv = (double)pc;
            const double dv = 0.5 * (dirx * ((double)pr - (double)pl) + diry * ((double)pb - (double)pt));
            const double H00 = df_wave_sum_d(dv * dv);
            const double H01 = df_wave_sum_d(dv);
            const double H11 = 64.0;
            const double detH = H00 * H11 - H01 * H01;
            const double Hi00 = H11 / detH, Hi01 = -H01 / detH, Hi11 = H00 / detH;
            double mean_diff = 0.0, chi2 = 0.0, up0 = 0.0, up1 = 0.0;
            for (int it = 0; it < g.align_iters; it++) {
                const double fu = floor(au), fv = floor(av);
                if (!(fu >= 4.0 && fv >= 4.0 && fu < (double)W - 4.0 && fv < (double)H - 4.0)) break;
                const int iu = (int)fu, iv = (int)fv;
                const double sx = au - fu, sy = av - fv;
                const double wTL = (1.0 - sx) * (1.0 - sy);
                const double wTR = sx * (1.0 - sy);
                const double wBL = (1.0 - sx) * sy;
                const double wBR = sx * sy;
                const uint8_t* p = cur + (size_t)(iv - 4 + ly) * stride + (iu - 4 + lx);
                const double sp_ = wTL * (double)p[0] + wTR * (double)p[1] + wBL * (double)p[stride] + wBR * (double)p[stride + 1];
                const double res = sp_ - refv + mean_diff;
                const double J0 = -df_wave_sum_d(res * dv);
                const double J1 = -df_wave_sum_d(res);
                const double new_chi2 = df_wave_sum_d(res * res);
                if (it > 0 && new_chi2 > chi2) {
                    au = au - up0;
                    av = av - up1;
                    break;
                }
                chi2 = new_chi2;
                up0 = Hi00 * J0 + Hi01 * J1;
                up1 = Hi01 * J0 + Hi11 * J1;
                au = au + up0 * dirx;
                av = av + up0 * diry;
                mean_diff = mean_diff + up1;
                if (up0 * up0 + up1 * up1 < 0.03 * 0.03) { conv = true; break; }
            }
        }
        tr.px = au;
        tr.py = av;
        if (!conv) { flag = DF_NO_MATCH; break; }
        /* 6. depth */
        const DfRay c = df_unit_ray(au, av, g);
        const double aa = Rf[0] * Rf[0] + Rf[1] * Rf[1] + Rf[2] * Rf[2];
        const double ac = Rf[0] * c.x + Rf[1] * c.y + Rf[2] * c.z;
        const double cc = c.x * c.x + c.y * c.y + c.z * c.z;
        const double detA = aa * cc - ac * ac;
        if (!(fabs(detA) >= 1e-6)) { flag = DF_DEGENERATE; break; }
        const double at = Rf[0] * t[0] + Rf[1] * t[1] + Rf[2] * t[2];
        const double ct = c.x * t[0] + c.y * t[1] + c.z * t[2];
        const double z = fabs(-((cc * at - ac * ct) / detA));
        tr.z = z;
        double trc[3];
#pragma unroll
        for (int i = 0; i < 3; i++) trc[i] = -(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]);
        const double a0 = f.x * z - trc[0], a1 = f.y * z - trc[1], a2 = f.z * z - trc[2];
        const double t_norm = sqrt(trc[0] * trc[0] + trc[1] * trc[1] + trc[2] * trc[2]);
        const double a_norm = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
        const double alpha = df_acos((f.x * trc[0] + f.y * trc[1] + f.z * trc[2]) / t_norm);
        const double beta = df_acos(-(a0 * trc[0] + a1 * trc[1] + a2 * trc[2]) / (t_norm * a_norm));
        const double beta_plus = beta + g.px_err;
        const double gamma_plus = 3.141592653589793 - alpha - beta_plus;
        const double z_plus = t_norm * sin(beta_plus) / sin(gamma_plus);
        const double tau = z_plus - z;
        tr.tau = tau;
        const double tau_inv = 0.5 * (1.0 / fmax(1e-7, z - tau) - 1.0 / (z + tau));
        /* 7. Vogiatzis-Hernandez */
        const double x = 1.0 / z;
        const double tau2 = tau_inv * tau_inv;
        const double norm_scale = sqrt(sigma2 + tau2);
        if (!isfinite(norm_scale)) { flag = DF_NONFINITE; break; }
        const double s2 = 1.0 / (1.0 / sigma2 + 1.0 / tau2);
        const double m = s2 * (mu / sigma2 + x / tau2);
        const double q = (x - mu) / norm_scale;
        const double pdf = exp(-0.5 * (q * q)) / (norm_scale * sqrt(2.0 * 3.141592653589793));
        double C1 = a / (a + b) * pdf;
        double C2 = b / (a + b) * (1.0 / z_range);
        const double nrm = C1 + C2;
        C1 = C1 / nrm;
        C2 = C2 / nrm;
        const double ff = C1 * (a + 1.0) / (a + b + 1.0) + C2 * a / (a + b + 1.0);
        const double ee = C1 * (a + 1.0) * (a + 2.0) / ((a + b + 1.0) * (a + b + 2.0)) + C2 * a * (a + 1.0) / ((a + b + 1.0) * (a + b + 2.0));
        n_mu = C1 * m + C2 * mu;
        n_sigma2 = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - n_mu * n_mu;
        n_a = (ee - ff) / (ff - ee / ff);
        n_b = n_a * (1.0 - ff) / ff;
        changed = true;
        /* 8. convergence */
        if (sqrt(n_sigma2) < z_range / g.conv_div) { n_state = 2; flag = DF_CONVERGED; }
    } while (0);
    if (lane == 0) {
        if (flag == DF_NO_MATCH) {
            sp->b = b + 1.0;
            sp->updates = updates + 1;
        } else if (changed) {
            sp->mu = n_mu; sp->sigma2 = n_sigma2; sp->a = n_a; sp->b = n_b;
            sp->state = n_state;
            sp->updates = updates + 1;
        }
        tr.flag = flag;
        *tp = tr;
    }
}

__global__ __launch_bounds__(256) void k_df_add(int pitch, int R, int seq0, double mu0, double sigma20, double z_range, tb_df_seed* seeds,
                                                int32_t* newest, int32_t* freelist, const float* Tcw, float* ring_Tcw,
                                                const float* keys_xy, const int32_t* counts, int key_pitch, const uint8_t* skip,
                                                int32_t* not_added) {
    __shared__ int wsum[4];
    const int s = seq0 + blockIdx.x, tid = threadIdx.x;
    const int slot = (newest[s] + 1) % R;
    tb_df_seed* sd = seeds + (size_t)s * pitch;
    int32_t* fl = freelist + (size_t)s * pitch;
    int nfree = 0;
    for (int e0 = 0; e0 < pitch; e0 += 256) {
        const int e = e0 + tid;
        bool fr = false;
        if (e < pitch) {
            int st = sd[e].state;
            if (st != 0 && sd[e].slot == slot) { st = 3; sd[e].state = 3; }
            fr = st == 0 || st == 3;
        }
        const int at = tb_block_ordered_slot(fr, nfree, wsum);
        if (fr) fl[at] = e;
    }
    __syncthreads();   /* the list is complete before a key reads it */
    const int n = min(max(counts[s], 0), key_pitch);
    int nk = 0;
    for (int k0 = 0; k0 < n; k0 += 256) {
        const int k = k0 + tid;
        const bool keep = k < n && !(skip && skip[(size_t)s * key_pitch + k]);
        const int at = tb_block_ordered_slot(keep, nk, wsum);
        if (keep && at < nfree) {
            tb_df_seed q;
            q.mu = mu0; q.sigma2 = sigma20; q.a = 10.0; q.b = 10.0; q.z_range = z_range;
            q.u = keys_xy[((size_t)s * key_pitch + k) * 2]; q.v = keys_xy[((size_t)s * key_pitch + k) * 2 + 1];
            q.slot = slot; q.state = 1; q.updates = 0; q.reserved = 0;
            sd[fl[at]] = q;
        }
    }
    if (tid < 16) ring_Tcw[((size_t)s * R + slot) * 16 + tid] = Tcw[(size_t)s * 16 + tid];
    if (tid == 0) {
        newest[s] = slot;   /* every thread read it before the first barrier */
        if (not_added) not_added[s] = max(0, nk - nfree);
    }
}

/* row blockIdx.x of sequence seq0 + blockIdx.y's image into the ring slot newest[s] */
__global__ __launch_bounds__(256) void k_df_copy(int R, int W, int H, int seq0, const int32_t* newest, const uint8_t* images, int stride,
                                                 size_t image_pitch, uint8_t* ring) {
    const int s = seq0 + blockIdx.y, row = blockIdx.x;
    const int slot = newest[s];
    if ((unsigned)slot >= (unsigned)R) return;
    const uint8_t* src = images + (size_t)s * image_pitch + (size_t)row * stride;
    uint8_t* dst = ring + (((size_t)s * R + slot) * H + row) * (size_t)W;
    for (int x = threadIdx.x; x < W; x += 256) dst[x] = src[x];
}

__global__ __launch_bounds__(256) void k_df_points(DfGeom g, tb_df_seed* seeds, const float* ring_Tcw, float* points, uint8_t* flags,
                                                   int release) {
    const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (e >= g.pitch) return;
    tb_df_seed* sp = seeds + (size_t)s * g.pitch + e;
    const int slot = sp->slot;
    const bool done = sp->state == 2 && (unsigned)slot < (unsigned)g.R;
    float X0 = 0.f, X1 = 0.f, X2 = 0.f;
    if (done) {
        const float* Tr = ring_Tcw + ((size_t)s * g.R + slot) * 16;
        const DfRay f = df_unit_ray((double)sp->u, (double)sp->v, g);
        const double d = 1.0 / sp->mu;
        const double x0 = f.x * d - (double)Tr[3], x1 = f.y * d - (double)Tr[7], x2 = f.z * d - (double)Tr[11];
        X0 = (float)((double)Tr[0] * x0 + (double)Tr[4] * x1 + (double)Tr[8] * x2);
        X1 = (float)((double)Tr[1] * x0 + (double)Tr[5] * x1 + (double)Tr[9] * x2);
        X2 = (float)((double)Tr[2] * x0 + (double)Tr[6] * x1 + (double)Tr[10] * x2);
        if (release) sp->state = 0;
    }
    float* o = points + ((size_t)s * g.pitch + e) * 3;
    o[0] = X0; o[1] = X1; o[2] = X2;
    flags[(size_t)s * g.pitch + e] = done ? 1 : 0;
}

static DfGeom df_geom(const tb_depth_filter* df) {
    DfGeom g;
    g.pitch = df->pitch; g.R = df->ref_slots; g.W = df->width; g.H = df->height;
    g.max_steps = df->prm.max_steps; g.zmssd_max = df->prm.zmssd_max; g.align_iters = df->prm.align_iters; g.pad_ = 0;
    g.fx = df->K[0]; g.fy = df->K[1]; g.cx = df->K[2]; g.cy = df->K[3];
    g.conv_div = df->prm.conv_div; g.px_err = df->px_err;
    return g;
}

int tbk_df_update(tb_depth_filter* df, int seq0, int nseq, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw) {
    return tb_launch(df->ctx, "k_df_update", k_df_update, dim3((df->pitch + 3) / 4, nseq), dim3(256), 0, df_geom(df), seq0, df->seeds,
                     df->traces, (const uint8_t*)df->ring, (const float*)df->ring_Tcw, images, stride, image_pitch, Tcw);
}

int tbk_df_add(tb_depth_filter* df, int seq0, int nseq, const uint8_t* images, int stride, size_t image_pitch, const float* Tcw,
               const float* keys_xy, const int32_t* counts, int key_pitch, const uint8_t* skip, int32_t* not_added) {
    const double z_range = 1.0 / df->prm.depth_min;
    TB_TRY(tb_launch(df->ctx, "k_df_add", k_df_add, dim3(nseq), dim3(256), 0, df->pitch, df->ref_slots, seq0, 1.0 / df->prm.depth_mean,
                     z_range * z_range / 36.0, z_range, df->seeds, df->newest, df->freelist, Tcw, df->ring_Tcw, keys_xy, counts, key_pitch,
                     skip, not_added));
    return tb_launch(df->ctx, "k_df_copy", k_df_copy, dim3(df->height, nseq), dim3(256), 0, df->ref_slots, df->width, df->height, seq0,
                     (const int32_t*)df->newest, images, stride, image_pitch, df->ring);
}

int tbk_df_points(tb_depth_filter* df, float* points, uint8_t* flags, int release) {
    return tb_launch(df->ctx, "k_df_points", k_df_points, dim3((df->pitch + 255) / 256, df->nseq), dim3(256), 0, df_geom(df), df->seeds,
                     (const float*)df->ring_Tcw, points, flags, release);
}
