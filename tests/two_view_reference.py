"""Two-view initialisation -- a relative pose and first points from 2D-2D rows alone: the definition tb_two_view_batch_dev
(include/tb_capi.h, k_two_view.hip) is held to, bit for bit (DESIGN.md 9m has the derivation and the deviations from ORB-SLAM's
Initializer).

float64 throughout, one operation per statement, only + - * / sqrt and comparisons, fixed loop counts, in the order written here
(numpy's are correctly rounded, as the device's are; the library builds with -ffp-contract=off). A statement of the RANSAC works
on all the hypotheses of a problem at once, a statement of the later stages on all its rows; a branch of the kernel is a np.where.

rows      the candidates are the rows below the count whose skip byte is 0, in index order, n of them; n < 8 is void.
sampling  draw k of hypothesis h is mix(seed + (16 h + k + 1) * 0x9E3779B97F4A7C15); its high 32 bits times n, shifted right by
          32, is a candidate. Draws k = 0, 1, ... are taken until eight distinct candidates are found or 16 are used up; a
          hypothesis that runs out is void.
solver    x = (u - cx) / fx, y = (v - cy) / fy; the 8 x 9 system with the rows (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1)
          (rs_run_7point's layout: x1' E x0 = 0, E row-major). Gauss-Jordan over the columns 0..8: the pivot is the unused row
          with the largest |a| in the column (the lowest row on a tie), taken iff |a| > 1e-12 * scale, scale = the largest
          |entry| of the unused rows from this column on; a column without a pivot is free. The pivot row is multiplied by
          1 / pivot and subtracted f times from every other row with f != 0. Exactly one free column c gives the null vector
          e[c] = 1, e[pivot column of row r] = -A[r][c]; any other count, or an entry that is not finite, is void.
score     F = K^-T E K^-1 (fundamental()). l1 = F (u0, v0, 1), l0 = F' (u1, v1, 1), d = (u1, v1, 1) . l1; a row is in the
          consensus iff d^2 / (l1x^2 + l1y^2) * inv_sigma2_1 <= chi2_epi and d^2 / (l0x^2 + l0y^2) * inv_sigma2_0 <= chi2_epi
          (a NaN is not). The winner has the most rows, ties to the lower hypothesis.
refit     the 9 x 9 normal matrix of the consensus rows: candidate c belongs to slot c mod 256, a slot adds its candidates'
          products in index order (a row outside the consensus adds 0.0), the 256 slots are summed by the butterfly
          p[t] = p[t] + p[t ^ d], d = 1, 2, 4, ..., 128. REFIT_SWEEPS cyclic Jacobi sweeps in the pair order (0,1) (0,2) ... (7,8)
          with the triangulation's rotation; the column of V at the smallest diagonal entry (the lowest index on a tie) is the
          new E, and the consensus is counted again against it.
decompose M = E' E, DECOMP_SWEEPS sweeps in the order (0,1) (0,2) (1,2). k3 = the smallest diagonal entry (lowest index on a
          tie), i1 < i2 the two others; s = sqrt(M[i][i]), v = V[:, i], u = E v / s; u3 = u1 x u2, v3 = v1 x v2 (both
          determinants are +1 by construction). Candidates: 0 (Ra, +u3), 1 (Ra, -u3), 2 (Rb, +u3), 3 (Rb, -u3) with
          Ra = U W V' = u2 v1' - u1 v2' + u3 v3', Rb = U W' V' = u1 v2' - u2 v1' + u3 v3'.
cheirality every candidate triangulates every consensus row with tests/triangulate_reference.py's statements and gates, view 0
          at the identity and view 1 at [R | t] in float64. good[c] counts the flags 1 and 4, tri[c] the flags 1.
decision  c* = the largest good, ties to the lower candidate. status 0 ok; 1 void; 2 good[c*] < min_points or
          (float64) good[c*] < min_good_ratio * (float64) consensus; 3 some other candidate has (float64) good[c] >
          ambiguity_ratio * (float64) good[c*]; 4 tri[c*] < min_points. The first failing test decides.
outputs   Tcw1 = [R | baseline t] Tcw0 (float32 of the float64 product; on failure Tcw0 as given); points: the accepted
          float32 points of c*, times baseline, taken to the world frame of Tcw0 (R0' (b X - t0)) in float64, as float32.
"""
import numpy as np

import triangulate_reference as tr

F64 = np.float64
F32 = np.float32
U64 = np.uint64
GAMMA = 0x9E3779B97F4A7C15
DRAWS = 16
SAMPLE = 8
SLOTS = 256
REFIT_SWEEPS = 5
DECOMP_SWEEPS = 6
DBL_MAX = np.finfo(F64).max
HYPOTHESES = 256
CHI2_EPI = 3.841
OK, VOID, FEW_GOOD, AMBIGUOUS, FEW_POINTS = range(5)
PAIRS9 = tuple((p, q) for p in range(9) for q in range(p + 1, 9))
PAIRS3 = ((0, 1), (0, 2), (1, 2))


def params(hypotheses=HYPOTHESES, chi2_epi=CHI2_EPI, refit=1, cos_parallax_max=tr.COS_PARALLAX_MAX, chi2_max=tr.CHI2_MAX,
           min_good_ratio=0.9, ambiguity_ratio=0.7, min_points=50, baseline=1.0, seed=0):
    """tb_two_view_params with its defaults (min_good_ratio, ambiguity_ratio, min_points: ORB-SLAM's ReconstructF)"""
    return dict(hypotheses=int(hypotheses), chi2_epi=F64(chi2_epi), refit=int(refit), cos_parallax_max=F64(cos_parallax_max),
                chi2_max=F64(chi2_max), min_good_ratio=F64(min_good_ratio), ambiguity_ratio=F64(ambiguity_ratio),
                min_points=int(min_points), baseline=F64(baseline), seed=int(seed))


def mix(z):
    """splitmix64's output function on uint64 arrays"""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draw(seed, h, k, n):
    """candidate index of draw k of the hypotheses h (array) among n candidates"""
    with np.errstate(over="ignore"):
        c = np.asarray(h, U64) * U64(DRAWS) + U64(k + 1)
        z = mix(U64(seed & 0xFFFFFFFFFFFFFFFF) + c * U64(GAMMA))
    return (((z >> U64(32)) * U64(n)) >> U64(32)).astype(np.int64)


def sample(seed, H, n):
    """(idx [H][8] int64, ok [H] bool): the eight candidates of every hypothesis; ok False = void (-1 where nothing was found)"""
    h = np.arange(H)
    idx = np.full((H, SAMPLE), -1, np.int64)
    cnt = np.zeros(H, np.int64)
    if n >= 1:
        for k in range(DRAWS):
            d = draw(seed, h, k, n)
            take = ~(idx == d[:, None]).any(1) & (cnt < SAMPLE)
            idx[take, cnt[take]] = d[take]
            cnt = cnt + take
    return idx, cnt == SAMPLE


def normalise(u, v, K):
    fx, fy, cx, cy = (F64(k) for k in K)
    x = u - cx
    x = x / fx
    y = v - cy
    y = y / fy
    return x, y


def epipolar_row(x0, y0, x1, y1):
    """the row of the epipolar system: nine arrays"""
    return [x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones_like(x0)]


def solve8(x0, y0, x1, y1):
    """x0, y0, x1, y1 [8][m] normalised coordinates of m samples -> (E [9][m], ok [m])"""
    m = len(x0[0])
    with np.errstate(all="ignore"):
        A = [epipolar_row(x0[i], y0[i], x1[i], y1[i]) for i in range(8)]
        used = [np.zeros(m, bool) for _ in range(8)]
        pivcol = [np.full(m, -1, np.int64) for _ in range(8)]
        nfree = np.zeros(m, np.int64)
        freecol = np.full(m, -1, np.int64)
        for col in range(9):
            bv = np.full(m, -1.0, F64)
            best = np.full(m, -1, np.int64)
            for r in range(8):
                a = np.abs(A[r][col])
                more = ~used[r] & (a > bv)
                bv = np.where(more, a, bv)
                best = np.where(more, r, best)
            scale = np.zeros(m, F64)
            for r in range(8):
                for k in range(col, 9):
                    a = np.abs(A[r][k])
                    more = ~used[r] & (a > scale)
                    scale = np.where(more, a, scale)
            thr = 1e-12 * scale
            piv = bv > thr
            nfree = nfree + ~piv
            freecol = np.where(piv, freecol, col)
            prow = [np.zeros(m, F64) for _ in range(9)]
            for r in range(8):
                for k in range(9):
                    prow[k] = np.where(best == r, A[r][k], prow[k])
            inv = 1.0 / prow[col]
            prow = [prow[k] * inv for k in range(9)]
            for r in range(8):
                isb = piv & (best == r)
                f = A[r][col]
                do = piv & ~isb & (f != 0)
                for k in range(9):
                    t = f * prow[k]
                    v = A[r][k] - t
                    A[r][k] = np.where(isb, prow[k], np.where(do, v, A[r][k]))
                used[r] = used[r] | isb
                pivcol[r] = np.where(isb, col, pivcol[r])
        ok = nfree == 1
        e = [np.where(freecol == k, 1.0, 0.0) for k in range(9)]
        for r in range(8):
            v = np.zeros(m, F64)
            for k in range(9):
                v = np.where(freecol == k, A[r][k], v)
            v = -v
            for k in range(9):
                e[k] = np.where(pivcol[r] == k, v, e[k])
        for k in range(9):
            ok = ok & (np.abs(e[k]) <= DBL_MAX)
    return e, ok


def fundamental(E, K):
    """F = K^-T E K^-1, nine entries row-major (E likewise; scalars or arrays)"""
    fx, fy, cx, cy = (F64(k) for k in K)
    with np.errstate(all="ignore"):
        G = []
        for i in range(3):
            g0 = E[3 * i] / fx
            g1 = E[3 * i + 1] / fy
            t = g0 * cx
            u = g1 * cy
            g2 = E[3 * i + 2] - t
            g2 = g2 - u
            G.append([g0, g1, g2])
        F = [None] * 9
        for j in range(3):
            f0 = G[0][j] / fx
            f1 = G[1][j] / fy
            t = f0 * cx
            u = f1 * cy
            f2 = G[2][j] - t
            f2 = f2 - u
            F[j], F[3 + j], F[6 + j] = f0, f1, f2
    return F


def inliers(F, rows, chi2_epi):
    """rows = (u0, v0, u1, v1, w0, w1) float64 arrays; F's entries broadcast against them"""
    u0, v0, u1, v1, w0, w1 = rows
    with np.errstate(all="ignore"):
        a = F[0] * u0
        a = a + F[1] * v0
        a = a + F[2]
        b = F[3] * u0
        b = b + F[4] * v0
        b = b + F[5]
        c = F[6] * u0
        c = c + F[7] * v0
        c = c + F[8]
        d = u1 * a
        d = d + v1 * b
        d = d + c
        dd = d * d
        s = a * a
        s = s + b * b
        e1 = dd / s
        e1 = e1 * w1
        a = F[0] * u1
        a = a + F[3] * v1
        a = a + F[6]
        b = F[1] * u1
        b = b + F[4] * v1
        b = b + F[7]
        s = a * a
        s = s + b * b
        e0 = dd / s
        e0 = e0 * w0
        return (e1 <= chi2_epi) & (e0 <= chi2_epi)


def jacobi(M, V, pairs, sweeps):
    """cyclic Jacobi on the symmetric M (list of lists, in place) with the triangulation's rotation; V accumulates"""
    m = len(M)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in pairs:
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
                for k in range(m):
                    M[k][p], M[k][q] = tr._rotate(M[k][p], M[k][q], c, s, skip)
                for k in range(m):
                    M[p][k], M[q][k] = tr._rotate(M[p][k], M[q][k], c, s, skip)
                for k in range(m):
                    V[k][p], V[k][q] = tr._rotate(V[k][p], V[k][q], c, s, skip)


def normal_matrix(a, inl):
    """a: nine arrays [n] (the epipolar rows), inl [n] bool -> the 9 x 9 sum over the consensus rows in the stated order"""
    n = len(inl)
    J = (n + SLOTS - 1) // SLOTS
    t = np.arange(SLOTS)
    N = [[None] * 9 for _ in range(9)]
    pad = np.zeros(J * SLOTS - n, F64)
    for i in range(9):
        for j in range(i, 9):
            prod = np.where(inl, a[i] * a[j], 0.0)
            prod = np.concatenate([prod, pad]).reshape(J, SLOTS)
            p = np.zeros(SLOTS, F64)
            for k in range(J):
                p = p + prod[k]
            d = 1
            while d < SLOTS:
                p = p + p[t ^ d]
                d *= 2
            N[i][j] = F64(p[0])
            N[j][i] = F64(p[0])
    return N


def refit(rows, inl, K):
    """the least-squares E of the consensus rows: nine float64"""
    with np.errstate(all="ignore"):
        x0, y0 = normalise(rows[0], rows[1], K)
        x1, y1 = normalise(rows[2], rows[3], K)
        N = normal_matrix(epipolar_row(x0, y0, x1, y1), inl)
        V = [[F64(1.0 if i == j else 0.0) for j in range(9)] for i in range(9)]
        jacobi(N, V, PAIRS9, REFIT_SWEEPS)
        best, k = N[0][0], 0
        for i in range(1, 9):
            if N[i][i] < best:
                best, k = N[i][i], i
    return [F64(V[i][k]) for i in range(9)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def decompose(E):
    """E nine float64 -> (R [4] of 3 x 3 nested lists, t [4] of lists): the four candidates"""
    with np.errstate(all="ignore"):
        M = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(i, 3):
                m = E[i] * E[j]
                m = m + E[3 + i] * E[3 + j]
                m = m + E[6 + i] * E[6 + j]
                M[i][j] = F64(m)
                M[j][i] = F64(m)
        V = [[F64(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
        jacobi(M, V, PAIRS3, DECOMP_SWEEPS)
        best, k3 = M[0][0], 0
        for i in range(1, 3):
            if M[i][i] < best:
                best, k3 = M[i][i], i
        i1, i2 = [i for i in range(3) if i != k3]
        s1, s2 = np.sqrt(M[i1][i1]), np.sqrt(M[i2][i2])
        v1 = [F64(V[k][i1]) for k in range(3)]
        v2 = [F64(V[k][i2]) for k in range(3)]
        u1, u2 = [], []
        for r in range(3):
            a = E[3 * r] * v1[0]
            a = a + E[3 * r + 1] * v1[1]
            a = a + E[3 * r + 2] * v1[2]
            u1.append(a / s1)
            a = E[3 * r] * v2[0]
            a = a + E[3 * r + 1] * v2[1]
            a = a + E[3 * r + 2] * v2[2]
            u2.append(a / s2)
        u3 = _cross(u1, u2)
        v3 = _cross(v1, v2)
        Ra = [[None] * 3 for _ in range(3)]
        Rb = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                a = u2[i] * v1[j]
                b = u1[i] * v2[j]
                c = u3[i] * v3[j]
                d = a - b
                Ra[i][j] = d + c
                d = b - a
                Rb[i][j] = d + c
        neg = [-u3[0], -u3[1], -u3[2]]
    return [Ra, Ra, Rb, Rb], [u3, neg, u3, neg]


def pose44(R, t):
    T = np.zeros((4, 4), F64)
    for i in range(3):
        for j in range(3):
            T[i, j] = R[i][j]
        T[i, 3] = t[i]
    T[3, 3] = 1.0
    return T


def triangulate(rows, T1, K, cos_parallax_max, chi2_max):
    """tests/triangulate_reference.py's triangulate_points with view 0 at the identity and view 1 at the float64 T1 ->
    (flags uint8 [n] in 1..5, points [n][3] float32 in the frame of view 0)"""
    fx, fy, cx, cy = K = tuple(F64(k) for k in K)
    u0, v0, u1, v1, s0, s1 = rows
    T0 = np.eye(4, dtype=F64)
    n = len(u0)
    with np.errstate(all="ignore"):
        x0 = (u0 - cx) / fx
        y0 = (v0 - cy) / fy
        x1 = (u1 - cx) / fx
        y1 = (v1 - cy) / fy
        A = tr.design_matrix(x0, y0, x1, y1, T0, T1)
        h = tr.null_vector(A)
        X = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]
        Xf = np.stack(X, -1).astype(F32)
        degenerate = (h[3] == 0) | ~np.isfinite(Xf).all(-1)
        z0 = tr._row(T0, 2, X)
        z1 = tr._row(T1, 2, X)
        behind = ~(z0 > 0) | ~(z1 > 0)
        r0 = tr._ray(T0, x0, y0)
        r1 = tr._ray(T1, x1, y1)
        n0 = np.sqrt(tr._dot(r0, r0))
        n1 = np.sqrt(tr._dot(r1, r1))
        cosv = tr._dot(r0, r1) / (n0 * n1)
        flat = ~(cosv < cos_parallax_max)
        c0 = tr._chi2(T0, X, z0, u0, v0, K, s0)
        c1 = tr._chi2(T1, X, z1, u1, v1, K, s1)
        off = (c0 > chi2_max) | (c1 > chi2_max)
    flags = np.full(n, tr.ACCEPTED, np.uint8)
    for code, bad in ((tr.REPROJECTION, off), (tr.PARALLAX, flat), (tr.DEPTH, behind), (tr.DEGENERATE, degenerate)):
        flags[bad] = code
    return flags, Xf


def compose(R, t, baseline, T0):
    """[R | baseline t] T0 in float64"""
    T = np.zeros((4, 4), F64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                a = R[i][0] * T0[0, j]
                a = a + R[i][1] * T0[1, j]
                a = a + R[i][2] * T0[2, j]
                T[i, j] = a
            a = R[i][0] * T0[0, 3]
            a = a + R[i][1] * T0[1, 3]
            a = a + R[i][2] * T0[2, 3]
            bt = baseline * t[i]
            T[i, 3] = a + bt
    T[3, 3] = 1.0
    return T


def to_world(Xf, baseline, T0):
    """the float32 points Xf [n][3] of view 0's frame times baseline, in the world frame of T0: [n][3] float32"""
    with np.errstate(all="ignore"):
        X = np.asarray(Xf, F32).astype(F64)
        d = []
        for k in range(3):
            a = baseline * X[:, k]
            d.append(a - T0[k, 3])
        out = []
        for i in range(3):
            a = T0[0, i] * d[0]
            a = a + T0[1, i] * d[1]
            a = a + T0[2, i] * d[2]
            out.append(a)
        return np.stack(out, -1).astype(F32)


def two_view(K, xy0, xy1, n=None, skip=None, inv_sigma2_0=None, inv_sigma2_1=None, Tcw0=None, prm=None):
    """One problem: xy0 / xy1 [pitch][2] float32 pixels. Returns a dict: status, Tcw1 float32 4 x 4, Tcw1_64 (float64, None on
    failure), points float32 [pitch][3] with written bool [pitch] (where the operator writes), point_flags uint8 [pitch], inlier
    uint8 [pitch], consensus, winner (hypothesis, candidate), good [4], tri [4], E (the nine float64 that were decomposed), counts
    int64 [H] (-1 where void), consensus0 (before the refit)."""
    prm = params() if prm is None else prm
    xy0 = np.asarray(xy0, F32).reshape(-1, 2)
    xy1 = np.asarray(xy1, F32).reshape(-1, 2)
    pitch = len(xy0)
    n = pitch if n is None else min(max(int(n), 0), pitch)
    H = prm["hypotheses"]
    T0_32 = np.eye(4, dtype=F32) if Tcw0 is None else np.asarray(Tcw0, F32).reshape(4, 4)
    T0 = T0_32.astype(F64)
    out = dict(status=VOID, Tcw1=T0_32.copy(), Tcw1_64=None, points=np.zeros((pitch, 3), F32), written=np.zeros(pitch, bool),
               point_flags=np.zeros(pitch, np.uint8), inlier=np.zeros(pitch, np.uint8), consensus=0, winner=(-1, -1),
               good=np.zeros(4, np.int32), tri=np.zeros(4, np.int32), E=None, counts=np.full(H, -1, np.int64), consensus0=0)
    cand = np.zeros(pitch, bool)
    cand[:n] = True
    if skip is not None:
        cand &= np.asarray(skip).reshape(pitch) == 0
    ids = np.nonzero(cand)[0]
    n = len(ids)
    if n < SAMPLE:
        return out
    w0 = np.ones(pitch, F32) if inv_sigma2_0 is None else np.asarray(inv_sigma2_0, F32).reshape(pitch)
    w1 = np.ones(pitch, F32) if inv_sigma2_1 is None else np.asarray(inv_sigma2_1, F32).reshape(pitch)
    rows = [xy0[ids, 0].astype(F64), xy0[ids, 1].astype(F64), xy1[ids, 0].astype(F64), xy1[ids, 1].astype(F64),
            w0[ids].astype(F64), w1[ids].astype(F64)]
    idx, ok_s = sample(prm["seed"], H, n)
    ii = np.where(idx < 0, 0, idx)
    with np.errstate(all="ignore"):
        x0, y0 = normalise(rows[0], rows[1], K)
        x1, y1 = normalise(rows[2], rows[3], K)
    E, ok = solve8([x0[ii[:, i]] for i in range(8)], [y0[ii[:, i]] for i in range(8)], [x1[ii[:, i]] for i in range(8)],
                   [y1[ii[:, i]] for i in range(8)])
    ok = ok & ok_s
    F = fundamental(E, K)
    inl = inliers([f[:, None] for f in F], [c[None, :] for c in rows], prm["chi2_epi"])
    counts = np.where(ok, inl.sum(1), -1)
    out["counts"] = counts
    if counts.max() < 0:
        return out
    h = int(np.argmax(counts))                     # the first maximum: the lower hypothesis
    Ew = [F64(e[h]) for e in E]
    mask = inl[h]
    out["consensus0"] = int(mask.sum())
    if prm["refit"]:
        Ew = refit(rows, mask, K)
        mask = inliers(fundamental(Ew, K), rows, prm["chi2_epi"])
    consensus = int(mask.sum())
    Rs, ts = decompose(Ew)
    sel = [r[mask] for r in rows]
    good, tri, fl, Xs = [], [], [], []
    for c in range(4):
        f, X = triangulate(sel, pose44(Rs[c], ts[c]), K, prm["cos_parallax_max"], prm["chi2_max"])
        fl.append(f); Xs.append(X)
        good.append(int(((f == tr.ACCEPTED) | (f == tr.PARALLAX)).sum()))
        tri.append(int((f == tr.ACCEPTED).sum()))
    cs = int(np.argmax(good))                      # ties to the lower candidate
    status = OK
    if good[cs] < prm["min_points"] or F64(good[cs]) < prm["min_good_ratio"] * F64(consensus):
        status = FEW_GOOD
    elif any(c != cs and F64(good[c]) > prm["ambiguity_ratio"] * F64(good[cs]) for c in range(4)):
        status = AMBIGUOUS
    elif tri[cs] < prm["min_points"]:
        status = FEW_POINTS
    inlier = np.zeros(pitch, np.uint8)
    inlier[ids[mask]] = 1
    pf = np.zeros(pitch, np.uint8)
    pf[ids[mask]] = fl[cs]
    out.update(status=status, inlier=inlier, consensus=consensus, winner=(h, cs), good=np.array(good, np.int32),
               tri=np.array(tri, np.int32), E=Ew, point_flags=pf)
    if status == OK:
        T1 = compose(Rs[cs], ts[cs], prm["baseline"], T0)
        world = to_world(Xs[cs], prm["baseline"], T0)
        acc = fl[cs] == tr.ACCEPTED
        out["points"][ids[mask][acc]] = world[acc]
        out["written"][ids[mask][acc]] = True
        out.update(Tcw1=T1.astype(F32), Tcw1_64=T1, R=np.array(Rs[cs], F64), t=np.array(ts[cs], F64))
    return out


def two_view_batch(K, xy0, xy1, counts=None, skip=None, inv_sigma2_0=None, inv_sigma2_1=None, Tcw0=None, prm=None):
    """tb_two_view_batch_dev on the host: xy0 / xy1 [nproblems][pitch][2]; the nullable inputs None. A list of two_view()'s dicts."""
    pick = lambda a, p: None if a is None else a[p]
    return [two_view(K, xy0[p], xy1[p], pick(counts, p), pick(skip, p), pick(inv_sigma2_0, p), pick(inv_sigma2_1, p), pick(Tcw0, p), prm)
            for p in range(len(xy0))]
