"""Sim(3) from 3D-3D rows: Horn's closed form inside a RANSAC, with a least-squares refit. The definition
tb_sim3_ransac_batch_dev (include/tb_capi.h, k_sim3.hip) is held to, bit for bit (DESIGN.md 9n has the derivation).

float64 throughout, one operation per statement, only + - * / sqrt fabs and comparisons, fixed loop counts, in the order written
here (numpy's are correctly rounded, as the device's are; the library builds with -ffp-contract=off). Every statement works on
all the hypotheses of a problem at once, element by element; a branch of the kernel is a np.where here.

A row is one physical point in camera-1 coordinates (X1) and in camera-2 coordinates (X2) with the two keys' invLevelSigma2; its
observation in image i is the projection of its own point Xi. The transform sought is X1 = s R12 X2 + t12.

Sampling: pnp_reference.sample, unchanged (three distinct rows out of at most 8 draws).

Horn (horn): sums S1, S2 of the m points of each set, O = S / m; Pr = X - O; M[i][j] = sum Pr2[i] Pr1[j]; the symmetric 4 x 4 N
of Horn 1987; SWEEPS cyclic Jacobi sweeps with the triangulation's rotation; the eigenvector at the largest diagonal entry, the
lowest index on a tie, corrected once from its residual (quaternion, residual: the residual N v - lam v is formed with Dekker's
exact products and Knuth's exact sums, which are + - * only), negated where w < 0, is the quaternion w x y z of R12; P3 = R12 Pr2; s = sum(Pr1 . P3) / sum(P3 . P3) or
exactly 1.0; t12 = O1 - s (R12 O2). A sum over the three points of a sample is ((0 + v0) + v1) + v2. A sum over the consensus
rows of the refit (total_rows): row i belongs to thread i mod 256, a thread adds its rows in ascending order to 0.0, and the 256
partial sums meet in the butterfly p[t] = p[t] + p[t ^ d], d = 1, 2, 4, ..., 128.

derive: sR12 = s R12, s21 = 1 / s, t21 = -(R12' t12) / s, sR21 = s21 R12'. A transform is void when s is not finite or not above
0, or when an entry of t12, t21 or s21 is not finite.

Score (inliers): Q1 = sR12 X2 + t12, Q2 = sR21 X1 + t21; a row is an inlier iff Z1, Z2, Q1z, Q2z > 0 and
|proj(Q1) - proj(X1)|^2 inv_sigma2_1 <= chi2_max and |proj(Q2) - proj(X2)|^2 inv_sigma2_2 <= chi2_max. The winner has the most
inliers, ties to the lower hypothesis. The refit runs Horn on the winner's consensus rows; it replaces the hypothesis iff it is
not void and its own consensus is not smaller.
"""
import numpy as np

import pnp_reference as pr
import two_view_reference as tv

F64 = np.float64
F32 = np.float32
SWEEPS = 5               # tests/test_sim3_reference.py: the smallest count that agrees with numpy's eigh to 1e-12 (4), plus one
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SLOTS = 256
CHI2_MAX = 9.210         # chi-square, 2 degrees of freedom, 99 %: ORB-SLAM's Sim3Solver threshold
HYPOTHESES = 256
DEGENERATE = 1e-6        # |a x b|^2 <= 1e-6 |a|^2 |b|^2: the sine of the sample's angle is below 1e-3
DBL_MAX = np.finfo(F64).max
FLAG_VOID = 1
ROW = np.dtype([("X1", "<f4"), ("Y1", "<f4"), ("Z1", "<f4"), ("X2", "<f4"), ("Y2", "<f4"), ("Z2", "<f4"),
                ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
FIELDS = ROW.names


def _dot(a, b):
    d = a[0] * b[0]
    d = d + a[1] * b[1]
    return d + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _finite(v):
    return np.abs(v) <= DBL_MAX


def total_sample(v):
    """v [H][3]: ((0 + v0) + v1) + v2"""
    a = 0.0 + v[..., 0]
    a = a + v[..., 1]
    return a + v[..., 2]


def total_rows(inl):
    """the refit's sum over the consensus rows inl [n] of per-row values v [n], in the stated order"""
    n = len(inl)
    J = (n + SLOTS - 1) // SLOTS
    t = np.arange(SLOTS)
    pad = np.zeros(J * SLOTS - n, F64)

    def total(v):
        v = np.concatenate([np.where(inl, v, 0.0), pad]).reshape(J, SLOTS)
        p = np.zeros(SLOTS, F64)
        for k in range(J):
            p = p + v[k]
        d = 1
        while d < SLOTS:
            p = p + p[t ^ d]
            d *= 2
        return F64(p[0])
    return total


def horn_matrix(M):
    """Horn's symmetric 4 x 4 N of M[i][j] = sum Pr2[i] Pr1[j]"""
    N = [[None] * 4 for _ in range(4)]
    a = M[0][0] + M[1][1]
    N[0][0] = a + M[2][2]
    a = M[0][0] - M[1][1]
    N[1][1] = a - M[2][2]
    a = M[1][1] - M[0][0]
    N[2][2] = a - M[2][2]
    a = M[2][2] - M[0][0]
    N[3][3] = a - M[1][1]
    N[0][1] = M[1][2] - M[2][1]
    N[0][2] = M[2][0] - M[0][2]
    N[0][3] = M[0][1] - M[1][0]
    N[1][2] = M[0][1] + M[1][0]
    N[1][3] = M[2][0] + M[0][2]
    N[2][3] = M[1][2] + M[2][1]
    for i in range(4):
        for j in range(i):
            N[i][j] = N[j][i]
    return N


SPLIT = 134217729.0       # 2^27 + 1: Veltkamp's splitter


def _split(a):
    c = SPLIT * a
    d = c - a
    hi = c - d
    return hi, a - hi


def two_prod(a, b):
    """(p, e): p = fl(a b) and a b = p + e exactly (Dekker; no fused multiply-add)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ah * bh
    e = e - p
    e = e + ah * bl
    e = e + al * bh
    e = e + al * bl
    return p, e


def two_sum(a, b):
    """(s, e): s = fl(a + b) and a + b = s + e exactly (Knuth)"""
    s = a + b
    bb = s - a
    e = s - bb
    e = a - e
    f = b - bb
    return s, e + f


def residual(N0, lam, v):
    """r = N0 v - lam v, every product and partial sum carried with its rounding error (a pair hi + lo), rounded once at the end"""
    r = []
    for j in range(4):
        hi, lo = two_prod(N0[j][0], v[0])
        for a, b in ((N0[j][1], v[1]), (N0[j][2], v[2]), (N0[j][3], v[3]), (-lam, v[j])):
            p, e = two_prod(a, b)
            hi, t = two_sum(hi, p)
            t = t + e
            lo = lo + t
        r.append(hi + lo)
    return r


def quaternion(M, sweeps=SWEEPS, refine=True):
    """the unit quaternion w x y z of R12 from M: Jacobi on N, the column k at the largest diagonal entry, one first-order
    correction of that column from its residual against the N the sweeps started from -- v_k + sum_(i != k) (v_i . r) /
    (lam_k - lam_i) v_i, a term left out where its denominator is 0 --, then w >= 0"""
    N = horn_matrix(M)
    N0 = [[N[i][j] for j in range(4)] for i in range(4)]
    V = [[np.ones_like(N[0][0]) if i == j else np.zeros_like(N[0][0]) for j in range(4)] for i in range(4)]
    tv.jacobi(N, V, PAIRS, sweeps)
    with np.errstate(all="ignore"):
        best = N[0][0]
        kidx = np.zeros(np.shape(best), np.int64)
        q = [V[i][0] for i in range(4)]
        for k in range(1, 4):
            more = N[k][k] > best
            best = np.where(more, N[k][k], best)
            kidx = np.where(more, k, kidx)
            q = [np.where(more, V[i][k], q[i]) for i in range(4)]
        if refine:
            r = residual(N0, best, q)
            out = [q[j] for j in range(4)]
            for i in range(4):
                c = V[0][i] * r[0]
                c = c + V[1][i] * r[1]
                c = c + V[2][i] * r[2]
                c = c + V[3][i] * r[3]
                d = best - N[i][i]
                coef = np.where((kidx != i) & (d != 0), c / d, 0.0)
                out = [out[j] + coef * V[j][i] for j in range(4)]
            q = out
        neg = q[0] < 0
        return [np.where(neg, -q[i], q[i]) for i in range(4)]


def rotation(q):
    w, x, y, z = q
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    R = [[None] * 3 for _ in range(3)]
    for (i, a, b) in ((0, yy, zz), (1, xx, zz), (2, xx, yy)):
        d = a + b
        d = 2.0 * d
        R[i][i] = 1.0 - d
    for (i, j, a, b, sign) in ((0, 1, xy, wz, -1), (0, 2, xz, wy, +1), (1, 0, xy, wz, +1), (1, 2, yz, wx, -1), (2, 0, xz, wy, -1),
                               (2, 1, yz, wx, +1)):
        d = a + b if sign > 0 else a - b
        R[i][j] = 2.0 * d
    return R


def horn(P1, P2, m, total, fixed_scale, sweeps=SWEEPS):
    """P1, P2: three coordinate arrays each with the points on the last axis, m the number of points (float64), total the sum over
    the points. Returns (q [4], s, t12 [3]); meaningless where the caller's void tests say so."""
    with np.errstate(all="ignore"):
        O1 = [total(P1[k]) / m for k in range(3)]
        O2 = [total(P2[k]) / m for k in range(3)]
        Pr1 = [P1[k] - np.asarray(O1[k])[..., None] for k in range(3)]
        Pr2 = [P2[k] - np.asarray(O2[k])[..., None] for k in range(3)]
        M = [[total(Pr2[i] * Pr1[j]) for j in range(3)] for i in range(3)]
        q = quaternion(M, sweeps)
        R = rotation(q)
        Rb = [[np.asarray(R[i][j])[..., None] for j in range(3)] for i in range(3)]
        P3 = []
        for i in range(3):
            a = Rb[i][0] * Pr2[0]
            a = a + Rb[i][1] * Pr2[1]
            P3.append(a + Rb[i][2] * Pr2[2])
        nom = total(_dot(Pr1, P3))
        den = total(_dot(P3, P3))
        s = nom / den
        if fixed_scale:
            s = np.ones_like(s)
        t = []
        for i in range(3):
            a = R[i][0] * O2[0]
            a = a + R[i][1] * O2[1]
            a = a + R[i][2] * O2[2]
            a = s * a
            t.append(O1[i] - a)
    return q, s, t


def derive(q, s, t):
    """(sR12 [3][3], t12, sR21 [3][3], t21, ok): what the score uses, and whether the transform is not void"""
    with np.errstate(all="ignore"):
        R = rotation(q)
        s21 = 1.0 / s
        sR12 = [[s * R[i][j] for j in range(3)] for i in range(3)]
        sR21 = [[s21 * R[j][i] for j in range(3)] for i in range(3)]
        t21 = []
        for i in range(3):
            b = R[0][i] * t[0]
            b = b + R[1][i] * t[1]
            b = b + R[2][i] * t[2]
            b = -b
            t21.append(b / s)
        ok = (s > 0) & _finite(s) & _finite(s21)
        for i in range(3):
            ok = ok & _finite(t[i]) & _finite(t21[i])
    return sR12, t, sR21, t21, ok


def project(X, Y, Z, K):
    fx, fy, cx, cy = (F64(k) for k in K)
    with np.errstate(all="ignore"):
        u = X / Z
        u = fx * u
        u = u + cx
        v = Y / Z
        v = fy * v
        v = v + cy
    return u, v


def row_chi2(T, rows, K):
    """(positive [..][n] bool, c1, c2 [..][n]) of rows (eight float64 arrays [n]) under the transforms T = derive()[:4], whose
    trailing shape broadcasts against [n]"""
    sR12, t12, sR21, t21 = T
    X1, Y1, Z1, X2, Y2, Z2, w1, w2 = rows
    with np.errstate(all="ignore"):
        u1, v1 = project(X1, Y1, Z1, K)
        u2, v2 = project(X2, Y2, Z2, K)
        Q1, Q2 = [], []
        for i in range(3):
            a = sR12[i][0] * X2
            a = a + sR12[i][1] * Y2
            a = a + sR12[i][2] * Z2
            Q1.append(a + t12[i])
            b = sR21[i][0] * X1
            b = b + sR21[i][1] * Y1
            b = b + sR21[i][2] * Z1
            Q2.append(b + t21[i])
        pu, pv = project(Q1[0], Q1[1], Q1[2], K)
        du = pu - u1
        dv = pv - v1
        e = du * du
        e = e + dv * dv
        c1 = e * w1
        pu, pv = project(Q2[0], Q2[1], Q2[2], K)
        du = pu - u2
        dv = pv - v2
        e = du * du
        e = e + dv * dv
        c2 = e * w2
        pos = (Z1 > 0) & (Z2 > 0) & (Q1[2] > 0) & (Q2[2] > 0)
    return pos, c1, c2


def inliers(T, rows, K, chi2_max):
    with np.errstate(all="ignore"):
        pos, c1, c2 = row_chi2(T, rows, K)
        return pos & (c1 <= F64(chi2_max)) & (c2 <= F64(chi2_max))


def sample_ok(P1, P2):
    """the void rules of a sample: P1, P2 three coordinate arrays [H][3] each"""
    with np.errstate(all="ignore"):
        ok = np.ones(P1[0].shape[:-1], bool)
        for P in (P1, P2):
            for k in range(3):
                ok = ok & _finite(P[k]).all(-1)
            ok = ok & (P[2] > 0).all(-1)
            a = [P[k][..., 1] - P[k][..., 0] for k in range(3)]
            b = [P[k][..., 2] - P[k][..., 0] for k in range(3)]
            c = _cross(a, b)
            cc, aa, bb = _dot(c, c), _dot(a, a), _dot(b, b)
            lim = DEGENERATE * aa
            lim = lim * bb
            ok = ok & (cc > lim)
    return ok


def _rows64(rows, n):
    return [np.asarray(rows[f][:n], F32).astype(F64) for f in FIELDS]


def make_rows(X1, X2, w1=None, w2=None, pitch=None):
    """a ROW array [pitch] from X1, X2 [n][3] and the two inv_sigma2 columns (default 1)"""
    n = len(X1)
    r = np.zeros(n if pitch is None else pitch, ROW)
    for k, f in enumerate(("X1", "Y1", "Z1")):
        r[f][:n] = np.asarray(X1)[:, k]
    for k, f in enumerate(("X2", "Y2", "Z2")):
        r[f][:n] = np.asarray(X2)[:, k]
    r["inv_sigma2_1"][:n] = 1.0 if w1 is None else w1
    r["inv_sigma2_2"][:n] = 1.0 if w2 is None else w2
    return r


def matrix(q, s, t):
    """[s R12 | t12; 0 0 0 1] in float64"""
    sR = derive(q, s, t)[0]
    T = np.eye(4)
    for i in range(3):
        T[i, :3] = [F64(sR[i][j]) for j in range(3)]
        T[i, 3] = F64(t[i])
    return T


def ransac(K, rows, n=None, hypotheses=HYPOTHESES, fixed_scale=False, chi2_max=CHI2_MAX, seed=0, sweeps=SWEEPS):
    """One problem: rows a ROW array (pitch rows), n its count (clamped to the pitch). Returns a dict: srt float64 [8] (w x y z,
    t12, s), S12 float64 4 x 4 and S1232 its float32 rounding, consensus, inlier uint8 [pitch], winner (hypothesis, refitted), flags,
    chi2 (c1, c2 [n] under the final transform; None when void), chi2_hyp (the same under the winning hypothesis), counts int64 [H]
    (-1 where void), samples (idx [H][3], ok [H])."""
    pitch = len(rows)
    n = pitch if n is None else min(max(int(n), 0), pitch)
    H = int(hypotheses)
    srt0 = np.array([1, 0, 0, 0, 0, 0, 0, 1], F64)
    out = dict(srt=srt0, S12=np.eye(4), S1232=np.eye(4, dtype=F32), consensus=0, inlier=np.zeros(pitch, np.uint8), winner=(-2, 0),
               flags=FLAG_VOID, chi2=None, chi2_hyp=None, counts=np.full(H, -1, np.int64), samples=None)
    if n < 3:
        return out
    r64 = _rows64(rows, n)
    idx, ok_s = pr.sample(seed, H, n)
    ii = np.where(idx < 0, 0, idx)
    P1 = [r64[k][ii] for k in range(3)]            # [H][3]
    P2 = [r64[3 + k][ii] for k in range(3)]
    q, s, t = horn(P1, P2, F64(3.0), total_sample, fixed_scale, sweeps)
    sR12, t12, sR21, t21, ok_t = derive(q, s, t)
    ok = ok_s & sample_ok(P1, P2) & ok_t
    col = lambda A: [[a[:, None] for a in r] for r in A]
    T = (col(sR12), [a[:, None] for a in t12], col(sR21), [a[:, None] for a in t21])
    inl = inliers(T, [c[None, :] for c in r64], K, chi2_max)
    counts = np.where(ok, inl.sum(1), -1)
    out["counts"] = counts
    out["samples"] = (idx, ok)
    if counts.max() < 0:
        return out
    h = int(np.argmax(counts))                     # the first maximum: the lower hypothesis
    best = int(counts[h])
    qw, sw, tw = [F64(a[h]) for a in q], F64(s[h]), [F64(a[h]) for a in t]
    Tw = derive(qw, sw, tw)[:4]
    pos, c1, c2 = row_chi2(Tw, r64, K)
    with np.errstate(all="ignore"):
        mask = pos & (c1 <= F64(chi2_max)) & (c2 <= F64(chi2_max))
    assert int(mask.sum()) == best
    out["chi2_hyp"] = (c1, c2)
    refitted = 0
    if best >= 3:
        total = total_rows(mask)
        qr, sr, trr = horn(r64[0:3], r64[3:6], F64(best), total, fixed_scale, sweeps)
        D = derive(qr, sr, trr)
        if bool(D[4]):
            pos_r, c1r, c2r = row_chi2(D[:4], r64, K)
            with np.errstate(all="ignore"):
                mask_r = pos_r & (c1r <= F64(chi2_max)) & (c2r <= F64(chi2_max))
            if int(mask_r.sum()) >= best:
                refitted = 1
                qw, sw, tw, mask, best, c1, c2 = [F64(a) for a in qr], F64(sr), [F64(a) for a in trr], mask_r, int(mask_r.sum()), c1r, c2r
    m = np.zeros(pitch, np.uint8)
    m[:n] = mask
    S = matrix(qw, sw, tw)
    out.update(srt=np.array(list(qw) + list(tw) + [sw], F64), S12=S, S1232=S.astype(F32), consensus=best, inlier=m, winner=(h, refitted),
               flags=0, chi2=(c1, c2))
    return out


def ransac_batch(K, rows, counts, **kw):
    """tb_sim3_ransac_batch_dev on the host: rows [nproblems][pitch] ROW, counts [nproblems]. A list of ransac()'s dicts."""
    return [ransac(K, rows[p], counts[p], **kw) for p in range(len(rows))]


def margin(res, chi2_max=CHI2_MAX):
    """the smallest relative distance of a gated quantity, under the winning hypothesis and under the final transform, from
    chi2_max (inf when void)"""
    best = np.inf
    for key in ("chi2_hyp", "chi2"):
        if res[key] is None:
            continue
        for c in res[key]:
            c = c[np.isfinite(c)]
            if len(c):
                best = min(best, float(np.min(np.abs(c - chi2_max)) / chi2_max))
    return best
