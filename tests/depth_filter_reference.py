"""The definition of the depth filter (tb_depth_filter_*, kernels k_df_update / k_df_add / k_df_points): numpy and plain Python
floats, written statement for statement in float64 unless marked integer; one rounding per statement, sums left to right, no
fused multiply-add. The kernel is held to this file: the integer stage (flag, n, winning sample, score) bit for bit, the rest
at 1e-6 relative.

Sources. The affine warp and the warped 10 x 10 patch follow the statements of the reference's Matcher::FindMatchDirect
(matcher.cpp:1518-1538 the warp, :1567-1592 the patch), in float64 where the reference computes in float; the 1-D alignment
follows the body of Matcher::Align1D the reference keeps commented out (matcher.cpp:1247-1364). Nothing of SVO is in the
reference: the depth from two rays, tau and the Gaussian x Beta seed update follow the published SVO / REMODE formulas
(Forster et al., ICRA 2014; Pizzoli et al., ICRA 2014; Vogiatzis and Hernandez, IVC 2011).

Two rules are the project's own: the search runs at level 0 only and a warp whose determinant leaves (1/3, 3) is flagged WARP;
and a degenerate two-ray intersection (|det A'A| < 1e-6) is DEGENERATE and leaves the seed unchanged, where SVO counts a failed
match -- which penalises the seeds near the epipole of a camera that drives along its rays.

Sum order of Align1D's 64-pixel sums (H, Jres, chi2): pixel (y, x) of the 8 x 8 patch is element t = 8 y + x, and the sum is the
butterfly p[t] = p[t] + p[t ^ d] for d = 1, 2, 4, 8, 16, 32; every element ends with the same bits.
"""
import math

import numpy as np

# tb_df_seed (64 bytes) and tb_df_trace (56 bytes) of include/tb_types.h
DF_SEED = np.dtype([("mu", "<f8"), ("sigma2", "<f8"), ("a", "<f8"), ("b", "<f8"), ("z_range", "<f8"), ("u", "<f4"), ("v", "<f4"),
                    ("slot", "<i4"), ("state", "<i4"), ("updates", "<i4"), ("reserved", "<i4")])
DF_TRACE = np.dtype([("score", "<i8"), ("px", "<f8"), ("py", "<f8"), ("z", "<f8"), ("tau", "<f8"), ("flag", "<i4"), ("n", "<i4"),
                     ("win", "<i4"), ("reserved", "<i4")])

FREE, ACTIVE, DONE, DROPPED = 0, 1, 2, 3                      # seed states
IDLE, UPDATED, BEHIND, OUTSIDE, WARP, DEGENERATE, NO_MATCH, CONVERGED, NONFINITE = -1, 0, 1, 2, 3, 4, 5, 6, 7   # trace flags
UNCHANGED = (BEHIND, OUTSIDE, WARP, DEGENERATE, NONFINITE)    # the flags that leave every byte of the seed

MARGIN = 5          # step 1: the point at d must project inside the image less this margin
HALF = 5            # step 2: half size of the warp's finite difference (matcher.cpp:1522)
PATCH_BORDER = 4    # step 4: a sample closer than this to the border is skipped
STEP_PX = 0.7       # step 4: pixels per sample
INT_MAX = 2147483647


class Params:
    def __init__(self, depth_mean=15.0, depth_min=2.0, conv_div=200.0, px_noise=1.0, max_steps=1000, zmssd_max=2000, align_iters=10,
                 ref_slots=4):
        self.depth_mean, self.depth_min, self.conv_div, self.px_noise = float(depth_mean), float(depth_min), float(conv_div), float(px_noise)
        self.max_steps, self.zmssd_max, self.align_iters, self.ref_slots = int(max_steps), int(zmssd_max), int(align_iters), int(ref_slots)


def px_error_angle(K, prm):
    return 2.0 * math.atan(prm.px_noise / (2.0 * math.sqrt(float(K[0]) * float(K[1]))))


def init_seed(rec, u, v, slot, prm):
    """Initialisation: mu = 1 / depth_mean, z_range = 1 / depth_min, sigma2 = z_range^2 / 36, a = b = 10"""
    z_range = 1.0 / prm.depth_min
    rec["mu"] = 1.0 / prm.depth_mean
    rec["z_range"] = z_range
    rec["sigma2"] = z_range * z_range / 36.0
    rec["a"] = 10.0
    rec["b"] = 10.0
    rec["u"] = u
    rec["v"] = v
    rec["slot"] = slot
    rec["state"] = ACTIVE
    rec["updates"] = 0
    rec["reserved"] = 0


def _rt(T):
    T = np.asarray(T, np.float32)
    return [[float(T[i, j]) for j in range(3)] for i in range(3)], [float(T[i, 3]) for i in range(3)]


def relative_pose(Tcw, Tcw_ref):
    """T_cr = Tcw Tcw_ref^-1 from two float32 poses, in float64: R = Rc Rr', t = tc - R tr"""
    Rc, tc = _rt(Tcw)
    Rr, tr = _rt(Tcw_ref)
    R = [[Rc[i][0] * Rr[j][0] + Rc[i][1] * Rr[j][1] + Rc[i][2] * Rr[j][2] for j in range(3)] for i in range(3)]
    t = [tc[i] - (R[i][0] * tr[0] + R[i][1] * tr[1] + R[i][2] * tr[2]) for i in range(3)]
    return R, t


def unit_ray(u, v, K):
    fx, fy, cx, cy = K
    x = (u - cx) / fx
    y = (v - cy) / fy
    nrm = math.sqrt(x * x + y * y + 1.0)
    return [x / nrm, y / nrm, 1.0 / nrm]


def _mul(R, p):
    return [R[i][0] * p[0] + R[i][1] * p[1] + R[i][2] * p[2] for i in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _butterfly(p):
    """p[t] = p[t] + p[t ^ d], d = 1 .. 32, on 64 float64 in patch order; returns the common value"""
    p = np.asarray(p, np.float64).reshape(64).copy()
    idx = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        p = p + p[idx ^ d]
    return float(p[0])


def warp_matrix(R, t, f, d, u, v, K):
    """step 2: A_cur_ref at depth d (range along f), level 0 (matcher.cpp:1518-1538) -> (A00, A01, A10, A11, uc, vc)"""
    fx, fy, cx, cy = K
    X = [f[0] * d, f[1] * d, f[2] * d]
    zr = X[2]
    xu = (u + HALF - cx) / fx
    yu = (v - cy) / fy
    xv = (u - cx) / fx
    yv = (v + HALF - cy) / fy
    Xu = [xu * zr, yu * zr, zr]
    Xv = [xv * zr, yv * zr, zr]
    px = []
    for P in (X, Xu, Xv):
        Q = _mul(R, P)
        Q = [Q[0] + t[0], Q[1] + t[1], Q[2] + t[2]]
        px.append((fx * (Q[0] / Q[2]) + cx, fy * (Q[1] / Q[2]) + cy))
    (uc, vc), (uu, vu), (uv, vv) = px
    return (uu - uc) / HALF, (uv - uc) / HALF, (vu - vc) / HALF, (vv - vc) / HALF, uc, vc


def warped_patch(ref_img, u, v, Ai):
    """step 3: the 10 x 10 patch with border, uint8: floor of the bilinear sample, 0 outside (matcher.cpp:1567-1592)"""
    H, W = ref_img.shape
    I00, I01, I10, I11 = Ai
    out = np.zeros((10, 10), np.uint8)
    for y in range(10):
        for x in range(10):
            dx = float(x - 5)
            dy = float(y - 5)
            px = I00 * dx + I01 * dy + u
            py = I10 * dx + I11 * dy + v
            if not (px >= 0.0 and py >= 0.0 and px < W - 1.0 and py < H - 1.0):
                continue
            iu = math.floor(px)
            iv = math.floor(py)
            su = px - iu
            sv = py - iv
            w00 = (1.0 - su) * (1.0 - sv)
            w01 = (1.0 - su) * sv
            w10 = su * (1.0 - sv)
            w11 = 1.0 - w00 - w01 - w10
            val = w00 * float(ref_img[iv, iu]) + w01 * float(ref_img[iv + 1, iu]) + w10 * float(ref_img[iv, iu + 1]) + \
                w11 * float(ref_img[iv + 1, iu + 1])
            out[y, x] = int(min(math.floor(val), 255.0))
    return out


def epipolar_search(img, patch8, A, B, n, K, prm):
    """step 4 from the sample count on: samples i = 0..n from B to A -> (winning index or -1, its score or -1, its pixel)"""
    H, W = img.shape
    fx, fy, cx, cy = K
    i = np.arange(n + 1, dtype=np.float64)
    tt = i / float(n)
    x = B[0] + tt * (A[0] - B[0])
    y = B[1] + tt * (A[1] - B[1])
    pu = np.floor(fx * x + cx + 0.5)
    pv = np.floor(fy * y + cy + 0.5)
    ok = (pu >= PATCH_BORDER) & (pv >= PATCH_BORDER) & (pu <= W - 1.0 - PATCH_BORDER) & (pv <= H - 1.0 - PATCH_BORDER)
    ok[1:] &= ~((pu[1:] == pu[:-1]) & (pv[1:] == pv[:-1]))      # a sample on the previous sample's pixel is skipped
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return -1, -1, (0, 0)
    iu = pu[idx].astype(np.int64)
    iv = pv[idx].astype(np.int64)
    oy, ox = np.mgrid[0:8, 0:8]
    Bp = img[iv[:, None, None] - 4 + oy[None], iu[:, None, None] - 4 + ox[None]].astype(np.int64)   # integer from here
    Ap = patch8.astype(np.int64)
    sA = int(Ap.sum())
    sAA = int((Ap * Ap).sum())
    sB = Bp.sum((1, 2))
    sBB = (Bp * Bp).sum((1, 2))
    sAB = (Bp * Ap[None]).sum((1, 2))
    score = 64 * (sAA - 2 * sAB + sBB) - (sA - sB) ** 2
    k = int(np.argmin(score))                                  # the first minimum wins
    return int(idx[k]), int(score[k]), (int(iu[k]), int(iv[k]))


def align_1d(img, patch10, dirx, diry, u, v, n_iter):
    """step 5: matcher.cpp:1247-1364 in float64 with the butterfly sums -> (converged, u, v)"""
    H, W = img.shape
    P = patch10.astype(np.float64)
    ref = P[1:9, 1:9]
    dv = 0.5 * (dirx * (P[1:9, 2:10] - P[1:9, 0:8]) + diry * (P[2:10, 1:9] - P[0:8, 1:9]))
    H00 = _butterfly(dv * dv)
    H01 = _butterfly(dv)
    H11 = 64.0
    det = H00 * H11 - H01 * H01
    with np.errstate(all="ignore"):
        det = np.float64(det)
        Hi00 = float(np.float64(H11) / det)
        Hi01 = float(-np.float64(H01) / det)
        Hi11 = float(np.float64(H00) / det)
    mean_diff = 0.0
    chi2 = 0.0
    up0 = 0.0
    up1 = 0.0
    converged = False
    for it in range(n_iter):
        fu = math.floor(u) if math.isfinite(u) else math.nan
        fv = math.floor(v) if math.isfinite(v) else math.nan
        if not (fu >= 4.0 and fv >= 4.0 and fu < W - 4.0 and fv < H - 4.0):
            break
        iu = int(fu)
        iv = int(fv)
        sx = u - fu
        sy = v - fv
        wTL = (1.0 - sx) * (1.0 - sy)
        wTR = sx * (1.0 - sy)
        wBL = (1.0 - sx) * sy
        wBR = sx * sy
        I = img[iv - 4:iv + 5, iu - 4:iu + 5].astype(np.float64)
        sp = wTL * I[0:8, 0:8] + wTR * I[0:8, 1:9] + wBL * I[1:9, 0:8] + wBR * I[1:9, 1:9]
        res = sp - ref + mean_diff
        J0 = -_butterfly(res * dv)
        J1 = -_butterfly(res)
        new_chi2 = _butterfly(res * res)
        if it > 0 and new_chi2 > chi2:
            u = u - up0       # the reference's statements: the step back takes the mean-difference update off v
            v = v - up1
            break
        chi2 = new_chi2
        up0 = Hi00 * J0 + Hi01 * J1
        up1 = Hi01 * J0 + Hi11 * J1
        u = u + up0 * dirx
        v = v + up0 * diry
        mean_diff = mean_diff + up1
        if up0 * up0 + up1 * up1 < 0.03 * 0.03:
            converged = True
            break
    return converged, u, v


def _acos(x):
    return math.acos(min(1.0, max(-1.0, x)))


def update_seed(seed, ref_img, Tcw_ref, img, Tcw, K, prm):
    """One update of one ACTIVE seed (a DF_SEED record) against a frame -> (new record, DF_TRACE record)"""
    K = tuple(float(k) for k in K)
    fx, fy, cx, cy = K
    H, W = img.shape
    out = np.array(seed, DF_SEED).copy()
    tr = np.zeros((), DF_TRACE)
    tr["win"] = -1
    tr["score"] = -1
    mu, sigma2, a, b, z_range = (float(seed[k]) for k in ("mu", "sigma2", "a", "b", "z_range"))
    u, v = float(seed["u"]), float(seed["v"])
    R, t = relative_pose(Tcw, Tcw_ref)
    f = unit_ray(u, v, K)
    Rf = _mul(R, f)

    def done(flag):
        tr["flag"] = flag
        return out, tr

    def no_match():
        out["b"] = b + 1.0
        out["updates"] = int(seed["updates"]) + 1
        return done(NO_MATCH)

    # 1. range ends
    sd = math.sqrt(sigma2)
    d = 1.0 / mu
    d_min = 1.0 / (mu + sd)
    d_max = 1.0 / max(mu - sd, 1e-8)
    P = [[Rf[i] * dd + t[i] for i in range(3)] for dd in (d, d_min, d_max)]
    if not (P[0][2] > 0.0 and P[1][2] > 0.0 and P[2][2] > 0.0):
        return done(BEHIND)
    A = (P[1][0] / P[1][2], P[1][1] / P[1][2])
    B = (P[2][0] / P[2][2], P[2][1] / P[2][2])
    uc = fx * (P[0][0] / P[0][2]) + cx
    vc = fy * (P[0][1] / P[0][2]) + cy
    if not (uc >= MARGIN and vc >= MARGIN and uc < W - float(MARGIN) and vc < H - float(MARGIN)):
        return done(OUTSIDE)
    # 2. affine warp
    A00, A01, A10, A11, _, _ = warp_matrix(R, t, f, d, u, v, K)
    det = A00 * A11 - A01 * A10
    if not (det > 1.0 / 3.0 and det < 3.0):
        return done(WARP)
    Ai = (A11 / det, -A01 / det, -A10 / det, A00 / det)
    # 3. reference patch
    patch10 = warped_patch(ref_img, u, v, Ai)
    # 4. epipolar search
    ax = fx * A[0] + cx
    ay = fy * A[1] + cy
    bx = fx * B[0] + cx
    by = fy * B[1] + cy
    ex = ax - bx
    ey = ay - by
    epi_len = math.sqrt(ex * ex + ey * ey)
    if not (epi_len >= 1e-6):
        return done(DEGENERATE)
    nd = max(1.0, float(np.floor(epi_len / STEP_PX)))
    tr["n"] = int(min(nd, float(INT_MAX)))
    if nd > prm.max_steps:
        return no_match()
    n = int(nd)
    win, score, (wu, wv) = epipolar_search(img, patch10[1:9, 1:9], A, B, n, K, prm)
    tr["win"] = win
    tr["score"] = score
    if win < 0 or score >= 64 * prm.zmssd_max:
        return no_match()
    # 5. sub-pixel alignment along the line
    conv, pu, pv = align_1d(img, patch10, ex / epi_len, ey / epi_len, float(wu), float(wv), prm.align_iters)
    tr["px"] = pu
    tr["py"] = pv
    if not conv:
        return no_match()
    # 6. depth: least-squares intersection of R f and the current unit ray
    c = unit_ray(pu, pv, K)
    aa = _dot(Rf, Rf)
    ac = _dot(Rf, c)
    cc = _dot(c, c)
    detA = aa * cc - ac * ac
    if not (abs(detA) >= 1e-6):
        return done(DEGENERATE)
    at = _dot(Rf, t)
    ct = _dot(c, t)
    z = abs(-((cc * at - ac * ct) / detA))
    tr["z"] = z
    t_rc = [-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) for i in range(3)]     # translation of T_cr^-1
    av = [f[i] * z - t_rc[i] for i in range(3)]
    t_norm = math.sqrt(_dot(t_rc, t_rc))
    a_norm = math.sqrt(_dot(av, av))
    alpha = _acos(_dot(f, t_rc) / t_norm)
    beta = _acos(-_dot(av, t_rc) / (t_norm * a_norm))
    beta_plus = beta + px_error_angle(K, prm)
    gamma_plus = math.pi - alpha - beta_plus
    z_plus = t_norm * math.sin(beta_plus) / math.sin(gamma_plus)
    tau = z_plus - z
    tr["tau"] = tau
    tau_inv = 0.5 * (1.0 / max(1e-7, z - tau) - 1.0 / (z + tau))
    # 7. Vogiatzis-Hernandez update
    x = 1.0 / z
    tau2 = tau_inv * tau_inv
    norm_scale = math.sqrt(sigma2 + tau2)
    if not math.isfinite(norm_scale):
        return done(NONFINITE)
    s2 = 1.0 / (1.0 / sigma2 + 1.0 / tau2)
    m = s2 * (mu / sigma2 + x / tau2)
    q = (x - mu) / norm_scale
    pdf = math.exp(-0.5 * (q * q)) / (norm_scale * math.sqrt(2.0 * math.pi))
    C1 = a / (a + b) * pdf
    C2 = b / (a + b) * (1.0 / z_range)
    nrm = C1 + C2
    C1 = C1 / nrm
    C2 = C2 / nrm
    ff = C1 * (a + 1.0) / (a + b + 1.0) + C2 * a / (a + b + 1.0)
    e = C1 * (a + 1.0) * (a + 2.0) / ((a + b + 1.0) * (a + b + 2.0)) + C2 * a * (a + 1.0) / ((a + b + 1.0) * (a + b + 2.0))
    mu_new = C1 * m + C2 * mu
    sigma2_new = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new
    a_new = (e - ff) / (ff - e / ff)
    b_new = a_new * (1.0 - ff) / ff
    out["mu"], out["sigma2"], out["a"], out["b"] = mu_new, sigma2_new, a_new, b_new
    out["updates"] = int(seed["updates"]) + 1
    # 8. convergence
    if math.sqrt(sigma2_new) < z_range / prm.conv_div:
        out["state"] = DONE
        return done(CONVERGED)
    return done(UPDATED)


def convergence_margin(seed, prm):
    """|sqrt(sigma2) / (z_range / conv_div) - 1|: how far a seed's convergence test is from its threshold"""
    return abs(math.sqrt(max(float(seed["sigma2"]), 0.0)) / (float(seed["z_range"]) / prm.conv_div) - 1.0)


def update_all(seeds, ring_img, ring_Tcw, img, Tcw, K, prm):
    """One update of every entry of one sequence -> (new seeds, traces); entries that are not ACTIVE keep their bytes, trace IDLE"""
    out = seeds.copy()
    traces = np.zeros(len(seeds), DF_TRACE)
    traces["flag"] = IDLE
    traces["win"] = -1
    traces["score"] = -1
    for e in np.nonzero(seeds["state"] == ACTIVE)[0]:
        s = int(seeds["slot"][e])
        out[e], traces[e] = update_seed(seeds[e], ring_img[s], ring_Tcw[s], img, Tcw, K, prm)
    return out, traces


def world_point(seed, Tcw_ref, K):
    """Tcw_ref^-1 (f / mu) in float64 -> 3 floats"""
    Rr, tr = _rt(Tcw_ref)
    f = unit_ray(float(seed["u"]), float(seed["v"]), tuple(float(k) for k in K))
    d = 1.0 / float(seed["mu"])
    X = [f[i] * d - tr[i] for i in range(3)]
    return [Rr[0][i] * X[0] + Rr[1][i] * X[1] + Rr[2][i] * X[2] for i in range(3)]


def add_keyframe(seeds, ring_img, ring_Tcw, newest, img, Tcw, keys_xy, count, skip, prm):
    """The ring takes the slot after the newest one; the seeds bound to it are DROPPED; one seed per offered key that is not
    skipped, in key order, into the entries that are FREE or DROPPED, in ascending entry order -> (slot, keys not added)"""
    slot = (newest + 1) % prm.ref_slots
    bound = (seeds["state"] != FREE) & (seeds["slot"] == slot)
    seeds["state"][bound] = DROPPED
    ring_img[slot] = img
    ring_Tcw[slot] = np.asarray(Tcw, np.float32)
    free = np.nonzero((seeds["state"] == FREE) | (seeds["state"] == DROPPED))[0]
    keep = [k for k in range(int(count)) if skip is None or not skip[k]]
    for e, k in zip(free, keep):
        init_seed(seeds[e:e + 1], np.float32(keys_xy[k][0]), np.float32(keys_xy[k][1]), slot, prm)
    return slot, max(0, len(keep) - len(free))


def points(seeds, ring_Tcw, K, release):
    """World points (float32 [pitch, 3], zero where not converged) and flags (uint8) of the DONE seeds; release frees them"""
    pts = np.zeros((len(seeds), 3), np.float32)
    flags = (seeds["state"] == DONE).astype(np.uint8)
    for e in np.nonzero(flags)[0]:
        pts[e] = world_point(seeds[e], ring_Tcw[int(seeds["slot"][e])], K)
    if release:
        seeds["state"][flags != 0] = FREE
    return pts, flags


class Filter:
    """One sequence of the filter on the functions above"""

    def __init__(self, width, height, K, pitch, prm=None):
        self.prm = prm or Params()
        self.K = tuple(float(k) for k in K)
        self.seeds = np.zeros(pitch, DF_SEED)
        self.traces = np.zeros(pitch, DF_TRACE)
        self.ring_img = np.zeros((self.prm.ref_slots, height, width), np.uint8)
        self.ring_Tcw = np.zeros((self.prm.ref_slots, 4, 4), np.float32)
        self.newest = -1

    def add_keyframe(self, img, Tcw, keys_xy, count=None, skip=None):
        count = len(keys_xy) if count is None else count
        self.newest, not_added = add_keyframe(self.seeds, self.ring_img, self.ring_Tcw, self.newest, img, Tcw, keys_xy, count, skip, self.prm)
        return not_added

    def update(self, img, Tcw):
        self.seeds, self.traces = update_all(self.seeds, self.ring_img, self.ring_Tcw, img, Tcw, self.K, self.prm)
        return self.traces

    def points(self, release=False):
        return points(self.seeds, self.ring_Tcw, self.K, release)
