"""Two-view linear triangulation with known poses (LocalBA::LinearTriangle, LocalBA.cpp:24-43) and its acceptance gates: the
definition tb_linear_triangle_batch_dev (include/tb_capi.h, k_triangulate.hip) is held to, bit for bit.

float64 throughout, one operation per statement, only + - * / sqrt (numpy's are correctly rounded, as the device's are), in the
order written here; every statement works on all the point pairs of one pose pair at once, element by element. The pixels are
normalised first -- x = (u - cx) / fx, y = (v - cy) / fy -- because the reference's rows p * Tcw.row(2) - Tcw.row(0) only
describe a projection when p is in normalised coordinates (documented deviation: the reference passes px_un, pixels). The null
vector of the 4 x 4 design matrix A is found by SWEEPS cyclic Jacobi sweeps on M = A^T A in the pair order (0,1) (0,2) (0,3)
(1,2) (1,3) (2,3) with the rotation formulas of the shim's LinearTriangle; a rotation is skipped only where M[p][q] == 0 and
there is no convergence test.

Flag codes: 0 not a candidate, 1 accepted, 2 V[3] == 0 or a non-finite result, 3 depth not above 0 in a view, 4 parallax (the
cosine of the two pixel rays in the world frame is not below cos_parallax_max), 5 reprojection (squared pixel error times
inv_sigma2 above chi2_max in a view). The first failing gate decides.
"""
import numpy as np

F64 = np.float64
F32 = np.float32
SWEEPS = 6
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
COS_PARALLAX_MAX = 0.9998
CHI2_MAX = 5.991
NOT_CANDIDATE, ACCEPTED, DEGENERATE, DEPTH, PARALLAX, REPROJECTION = range(6)


def design_matrix(x0, y0, x1, y1, T0, T1):
    """LocalBA.cpp:31-35 on normalised coordinates: A[r][c] float64 arrays [n]"""
    A = [[None] * 4 for _ in range(4)]
    for c in range(4):
        A[0][c] = x0 * T0[2, c] - T0[0, c]
        A[1][c] = y0 * T0[2, c] - T0[1, c]
        A[2][c] = x1 * T1[2, c] - T1[0, c]
        A[3][c] = y1 * T1[2, c] - T1[1, c]
    return A


def _rotate(a, b, c, s, skip):
    ca = c * a
    sb = s * b
    sa = s * a
    cb = c * b
    return np.where(skip, a, ca - sb), np.where(skip, b, sa + cb)


def null_vector(A):
    """The column of V at the smallest diagonal entry of the rotated M = A^T A (lowest index on a tie): 4 float64 arrays [n]"""
    n = len(A[0][0])
    M = [[None] * 4 for _ in range(4)]
    V = [[np.full(n, 1.0 if i == j else 0.0, F64) for j in range(4)] for i in range(4)]
    for i in range(4):
        for j in range(i, 4):
            m = A[0][i] * A[0][j]
            m = m + A[1][i] * A[1][j]
            m = m + A[2][i] * A[2][j]
            m = m + A[3][i] * A[3][j]
            M[i][j] = m
            M[j][i] = m.copy()
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            skip = M[p][q] == 0
            num = M[q][q] - M[p][p]
            den = 2.0 * M[p][q]
            th = num / den
            r = th * th
            r = r + 1.0
            r = np.sqrt(r)
            r = np.abs(th) + r
            t = np.where(th >= 0, 1.0, -1.0) / r
            c = t * t
            c = c + 1.0
            c = np.sqrt(c)
            c = 1.0 / c
            s = t * c
            for k in range(4):
                M[k][p], M[k][q] = _rotate(M[k][p], M[k][q], c, s, skip)
            for k in range(4):
                M[p][k], M[q][k] = _rotate(M[p][k], M[q][k], c, s, skip)
            for k in range(4):
                V[k][p], V[k][q] = _rotate(V[k][p], V[k][q], c, s, skip)
    best = M[0][0]
    h = [V[k][0] for k in range(4)]
    for i in range(1, 4):
        less = M[i][i] < best
        best = np.where(less, M[i][i], best)
        h = [np.where(less, V[k][i], h[k]) for k in range(4)]
    return h


def _row(T, r, X):
    a = T[r, 0] * X[0]
    a = a + T[r, 1] * X[1]
    a = a + T[r, 2] * X[2]
    return a + T[r, 3]


def _ray(T, x, y):
    """R^T (x, y, 1): the pixel's ray in the world frame"""
    out = []
    for i in range(3):
        a = T[0, i] * x
        a = a + T[1, i] * y
        out.append(a + T[2, i])
    return out


def _dot(a, b):
    d = a[0] * b[0]
    d = d + a[1] * b[1]
    return d + a[2] * b[2]


def _chi2(T, X, z, u, v, K, inv_sigma2):
    fx, fy, cx, cy = K
    pu = _row(T, 0, X) / z
    pu = fx * pu
    pu = pu + cx
    pv = _row(T, 1, X) / z
    pv = fy * pv
    pv = pv + cy
    du = pu - u
    dv = pv - v
    e = du * du + dv * dv
    return e * inv_sigma2


def triangulate_points(p0, p1, Tcw0, Tcw1, K, inv_sigma2_0=None, inv_sigma2_1=None, cos_parallax_max=COS_PARALLAX_MAX,
                       chi2_max=CHI2_MAX):
    """n point pairs of one pose pair: p0 / p1 float32 [n][2] pixels, Tcw0 / Tcw1 float32 4 x 4, inv_sigma2 float32 [n] or None
    (= 1). Returns (flags [n] uint8 in 1..5, points [n][3] float32 -- the float32 of X wherever it was computed; the operator
    writes it where the flag is 1 --, dict of float64 intermediates: A, h, X, cos, chi2)."""
    fx, fy, cx, cy = K = tuple(F64(k) for k in K)
    T0 = np.asarray(Tcw0, F32).reshape(4, 4).astype(F64)
    T1 = np.asarray(Tcw1, F32).reshape(4, 4).astype(F64)
    p0 = np.asarray(p0, F32).reshape(-1, 2).astype(F64)
    p1 = np.asarray(p1, F32).reshape(-1, 2).astype(F64)
    n = len(p0)
    s0 = np.ones(n, F64) if inv_sigma2_0 is None else np.asarray(inv_sigma2_0, F32).reshape(n).astype(F64)
    s1 = np.ones(n, F64) if inv_sigma2_1 is None else np.asarray(inv_sigma2_1, F32).reshape(n).astype(F64)
    u0, v0, u1, v1 = p0[:, 0].copy(), p0[:, 1].copy(), p1[:, 0].copy(), p1[:, 1].copy()
    with np.errstate(all="ignore"):
        x0 = (u0 - cx) / fx
        y0 = (v0 - cy) / fy
        x1 = (u1 - cx) / fx
        y1 = (v1 - cy) / fy
        A = design_matrix(x0, y0, x1, y1, T0, T1)
        h = null_vector(A)
        X = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]
        Xf = np.stack(X, -1).astype(F32)
        degenerate = (h[3] == 0) | ~np.isfinite(Xf).all(-1)
        z0 = _row(T0, 2, X)
        z1 = _row(T1, 2, X)
        behind = ~(z0 > 0) | ~(z1 > 0)
        r0 = _ray(T0, x0, y0)
        r1 = _ray(T1, x1, y1)
        n0 = np.sqrt(_dot(r0, r0))
        n1 = np.sqrt(_dot(r1, r1))
        cosv = _dot(r0, r1) / (n0 * n1)
        flat = ~(cosv < cos_parallax_max)
        c0 = _chi2(T0, X, z0, u0, v0, K, s0)
        c1 = _chi2(T1, X, z1, u1, v1, K, s1)
        off = (c0 > chi2_max) | (c1 > chi2_max)
    flags = np.full(n, ACCEPTED, np.uint8)
    for code, bad in ((REPROJECTION, off), (PARALLAX, flat), (DEPTH, behind), (DEGENERATE, degenerate)):   # the first gate wins
        flags[bad] = code
    info = dict(A=np.array([[A[r][c] for c in range(4)] for r in range(4)]).transpose(2, 0, 1), h=np.stack(h, -1),
                X=np.stack(X, -1), cos=cosv, chi2=np.stack([c0, c1], -1))
    return flags, Xf, info


def triangulate(p0, p1, Tcw0, Tcw1, K, inv_sigma2_0=1.0, inv_sigma2_1=1.0, cos_parallax_max=COS_PARALLAX_MAX, chi2_max=CHI2_MAX):
    """One point pair -> (flag, float32 [3] point, dict of float64 intermediates)"""
    f, X, info = triangulate_points([p0], [p1], Tcw0, Tcw1, K, [inv_sigma2_0], [inv_sigma2_1], cos_parallax_max, chi2_max)
    return int(f[0]), X[0], {k: v[0] for k, v in info.items()}


def triangulate_batch(xy0, xy1, counts, Tcw0, Tcw1, K, inv_sigma2_0=None, inv_sigma2_1=None, skip=None,
                      cos_parallax_max=COS_PARALLAX_MAX, chi2_max=CHI2_MAX):
    """tb_linear_triangle_batch_dev on the host: xy0 / xy1 [npairs][pitch][2], counts [npairs] or None, Tcw0 / Tcw1
    [npairs][4][4], inv_sigma2 / skip [npairs][pitch] or None. Returns (points [npairs][pitch][3] float32, zero where not
    accepted; flags [npairs][pitch] uint8; tally [npairs][6] int32)."""
    xy0 = np.asarray(xy0, F32); xy1 = np.asarray(xy1, F32)
    npairs, pitch = xy0.shape[:2]
    pts = np.zeros((npairs, pitch, 3), F32)
    flags = np.zeros((npairs, pitch), np.uint8)
    tally = np.zeros((npairs, 6), np.int32)
    for p in range(npairs):
        n = pitch if counts is None else min(max(int(counts[p]), 0), pitch)
        cand = np.zeros(pitch, bool)
        cand[:n] = True
        if skip is not None:
            cand &= np.asarray(skip[p]).reshape(pitch) == 0
        idx = np.nonzero(cand)[0]
        if len(idx):
            f, X, _ = triangulate_points(xy0[p, idx], xy1[p, idx], Tcw0[p], Tcw1[p], K,
                                         None if inv_sigma2_0 is None else np.asarray(inv_sigma2_0[p])[idx],
                                         None if inv_sigma2_1 is None else np.asarray(inv_sigma2_1[p])[idx], cos_parallax_max, chi2_max)
            flags[p, idx] = f
            ok = f == ACCEPTED
            pts[p, idx[ok]] = X[ok]
        tally[p] = np.bincount(flags[p], minlength=6)[:6]
    return pts, flags, tally
