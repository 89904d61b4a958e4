"""P3P-RANSAC pose from 3D-2D rows without a prior: the definition tb_pnp_ransac_batch_dev (include/tb_capi.h, k_pnp.hip) is held
to, bit for bit (DESIGN.md 9l has the derivation).

float64 throughout, one operation per statement, only + - * / sqrt and comparisons, fixed loop counts, in the order written here
(numpy's are correctly rounded, as the device's are; the library builds with -ffp-contract=off). Every statement works on all
the hypotheses of a problem at once, element by element; a branch of the kernel is a np.where here.

Sampling: draw k of hypothesis h is mix(seed + (8 h + k + 1) * 0x9E3779B97F4A7C15) (output 8 h + k of synth.Stream(seed)); its
high 32 bits times n, shifted right by 32, is a row. Draws k = 0, 1, ... are taken until three distinct rows are found or 8 are
used up; a hypothesis that runs out is void.

Minimal solver (solve_p3p): unit bearings y_i, squared side lengths a_ij, the cosines b_ij = y_i . y_j. The depths L solve
L' M_ij L = a_ij; D1 = M12 a23 - M23 a12 and D2 = M13 a23 - M23 a13 are homogeneous. A real root g of det(D1 + g D2) = 0 (monic
cubic, 80 bisections inside the Cauchy bound, 2 Newton steps) gives a rank-2 conic D0 = l m' + m l'; adj(D0) = -(l x m)(l x m)'
yields p = l x m from its largest diagonal entry, D0 + [p]x = 2 m l' yields l (a row) and m (a column) at its largest entry.
Each plane n . L = 0 is spanned by n x e_j, n x e_k (i = the largest |n_i|), on which D1 is a binary quadratic with the two
roots (q, A) and (C, q), q = -(B + sign(B) sqrt(B^2 - A C)). The direction is scaled by the sum of the three side equations;
a solution needs three positive depths. R = Y X^-1 from the two edge vectors and their cross product, t = L1 y1 - R x1.
Solutions 0, 1 are the plane l's, 2, 3 the plane m's.

Score: a row is an inlier iff its camera depth is > 0 and ((u - u^)^2 + (v - v^)^2) * inv_sigma2 <= chi2_max. The winner has the
most inliers, ties to the lower hypothesis then the lower solution; a prior is hypothesis -1 and wins ties.
"""
import numpy as np

F64 = np.float64
F32 = np.float32
U64 = np.uint64
GAMMA = 0x9E3779B97F4A7C15
DRAWS = 8
BISECTIONS = 80
NEWTONS = 2
CHI2_MAX = 5.991
HYPOTHESES = 256
DBL_MAX = np.finfo(F64).max
FLAG_VOID = 1           # flags bit 0: no pose was found (n < 3, or no hypothesis with a solution and no prior)


def mix(z):
    """splitmix64's output function on uint64 arrays"""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draw(seed, h, k, n):
    """row index of draw k of the hypotheses h (array) among n rows"""
    with np.errstate(over="ignore"):
        c = np.asarray(h, U64) * U64(8) + U64(k + 1)
        z = mix(U64(seed & 0xFFFFFFFFFFFFFFFF) + c * U64(GAMMA))
    return (((z >> U64(32)) * U64(n)) >> U64(32)).astype(np.int64)


def sample(seed, H, n):
    """(idx [H][3] int64, ok [H] bool): the three rows of every hypothesis; ok False = void (idx then holds what was found, -1
    where nothing was)"""
    h = np.arange(H)
    i0 = np.full(H, -1, np.int64); i1 = i0.copy(); i2 = i0.copy()
    if n >= 1:
        for k in range(DRAWS):
            d = draw(seed, h, k, n)
            take0 = i0 < 0
            take1 = ~take0 & (i1 < 0) & (d != i0)
            take2 = ~take0 & (i1 >= 0) & (i2 < 0) & (d != i0) & (d != i1)
            i0 = np.where(take0, d, i0)
            i1 = np.where(take1, d, i1)
            i2 = np.where(take2, d, i2)
    return np.stack([i0, i1, i2], -1), i2 >= 0


def _dot(a, b):
    d = a[0] * b[0]
    d = d + a[1] * b[1]
    return d + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _adj(s):
    """adjugate of the symmetric 3 x 3 s = (00, 01, 02, 11, 12, 22), same packing"""
    return [s[3] * s[5] - s[4] * s[4], s[2] * s[4] - s[1] * s[5], s[1] * s[4] - s[2] * s[3],
            s[0] * s[5] - s[2] * s[2], s[1] * s[2] - s[0] * s[4], s[0] * s[3] - s[1] * s[1]]


def _det(s, a):
    d = s[0] * a[0]
    d = d + s[1] * a[1]
    return d + s[2] * a[2]


def _trace(a, b):
    """trace(a b) of two packed symmetric matrices"""
    d = a[0] * b[0]
    d = d + a[3] * b[3]
    d = d + a[5] * b[5]
    e = a[1] * b[1]
    e = e + a[2] * b[2]
    e = e + a[4] * b[4]
    e = 2.0 * e
    return d + e


def _quad(s, a, b):
    """a' s b, s packed symmetric"""
    r0 = s[0] * b[0]
    r0 = r0 + s[1] * b[1]
    r0 = r0 + s[2] * b[2]
    r1 = s[1] * b[0]
    r1 = r1 + s[3] * b[1]
    r1 = r1 + s[4] * b[2]
    r2 = s[2] * b[0]
    r2 = r2 + s[4] * b[1]
    r2 = r2 + s[5] * b[2]
    return _dot(a, [r0, r1, r2])


def _cubic(g, p2, p1, p0):
    f = g + p2
    f = f * g
    f = f + p1
    f = f * g
    return f + p0


def _side(d, i, j, b):
    """d' M_ij d"""
    q = d[i] * d[i]
    q = q + d[j] * d[j]
    c = b * d[i]
    c = c * d[j]
    c = 2.0 * c
    return q - c


def solve_p3p(uv, X, K):
    """uv [3][2][m] pixels and X [3][3][m] world points of m samples (float64 arrays holding float32 values), K = fx, fy, cx, cy.
    Returns (R [4][3][3][m], t [4][3][m], ok [4][m]): up to four poses per sample; where ok is False the pose is meaningless."""
    fx, fy, cx, cy = (F64(k) for k in K)
    with np.errstate(all="ignore"):
        y = []
        for i in range(3):
            bx = (uv[i][0] - cx) / fx
            by = (uv[i][1] - cy) / fy
            nn = bx * bx
            nn = nn + by * by
            nn = nn + 1.0
            nn = np.sqrt(nn)
            y.append([bx / nn, by / nn, 1.0 / nn])
        b12, b13, b23 = _dot(y[0], y[1]), _dot(y[0], y[2]), _dot(y[1], y[2])
        e1 = [X[1][k] - X[0][k] for k in range(3)]
        e2 = [X[2][k] - X[0][k] for k in range(3)]
        e12 = [X[2][k] - X[1][k] for k in range(3)]
        a12, a13, a23 = _dot(e1, e1), _dot(e2, e2), _dot(e12, e12)
        good = (a12 > 0) & (a13 > 0) & (a23 > 0)
        zero = np.zeros_like(a12)
        D1 = [a23, -(b12 * a23), zero, a23 - a12, b23 * a12, -a12]
        D2 = [a23, zero, -(b13 * a23), -a13, b23 * a13, a23 - a13]
        A1, A2 = _adj(D1), _adj(D2)
        c0, c1, c2, c3 = _det(D1, A1), _trace(A1, D2), _trace(A2, D1), _det(D2, A2)
        p2, p1, p0 = c2 / c3, c1 / c3, c0 / c3
        bound = np.abs(p2)
        bound = np.where(np.abs(p1) > bound, np.abs(p1), bound)
        bound = np.where(np.abs(p0) > bound, np.abs(p0), bound)
        bound = bound + 1.0
        lo, hi = -bound, bound
        for _ in range(BISECTIONS):
            mid = lo + hi
            mid = 0.5 * mid
            pos = _cubic(mid, p2, p1, p0) > 0
            hi = np.where(pos, mid, hi)
            lo = np.where(pos, lo, mid)
        g = lo + hi
        g = 0.5 * g
        for _ in range(NEWTONS):
            f = _cubic(g, p2, p1, p0)
            df = 3.0 * g
            df = df + 2.0 * p2
            df = df * g
            df = df + p1
            step = f / df
            g = np.where(df != 0, g - step, g)
        D0 = [D1[k] + g * D2[k] for k in range(6)]
        B = _adj(D0)
        # p = l x m from the largest diagonal entry of -adj(D0)
        best = -B[0]
        col = [B[0], B[1], B[2]]
        for diag, c in ((B[3], [B[1], B[3], B[4]]), (B[5], [B[2], B[4], B[5]])):
            more = -diag > best
            best = np.where(more, -diag, best)
            col = [np.where(more, c[k], col[k]) for k in range(3)]
        good = good & (best > 0)
        sq = np.sqrt(best)
        p = [-(col[k] / sq) for k in range(3)]
        N = [[D0[0], D0[1] - p[2], D0[2] + p[1]], [D0[1] + p[2], D0[3], D0[4] - p[0]], [D0[2] - p[1], D0[4] + p[0], D0[5]]]
        big = np.abs(N[0][0])
        l = [N[0][0], N[0][1], N[0][2]]
        m = [N[0][0], N[1][0], N[2][0]]
        for r in range(3):
            for c in range(3):
                if r == 0 and c == 0:
                    continue
                more = np.abs(N[r][c]) > big
                big = np.where(more, np.abs(N[r][c]), big)
                l = [np.where(more, N[r][k], l[k]) for k in range(3)]
                m = [np.where(more, N[k][c], m[k]) for k in range(3)]
        # the pose-independent half of R = Y X^-1
        e3 = _cross(e1, e2)
        g1, g2, g3 = _cross(e2, e3), _cross(e3, e1), _cross(e1, e2)
        det = _dot(e1, g1)
        good = good & (det > 0)
        g1 = [v / det for v in g1]
        g2 = [v / det for v in g2]
        g3 = [v / det for v in g3]
        asum = a12 + a13
        asum = asum + a23
        Rs, ts, oks = [], [], []
        for n in (l, m):
            k1 = np.abs(n[1]) > np.abs(n[0])
            top = np.where(k1, np.abs(n[1]), np.abs(n[0]))
            k2 = np.abs(n[2]) > top
            # n x e0 = (0, n2, -n1), n x e1 = (-n2, 0, n0), n x e2 = (n1, -n0, 0); largest |n_k|: u = n x e_(k+1), w = n x e_(k+2)
            c0_, c1_, c2_ = [zero, n[2], -n[1]], [-n[2], zero, n[0]], [n[1], -n[0], zero]
            u = [np.where(k2, c0_[k], np.where(k1, c2_[k], c1_[k])) for k in range(3)]
            w = [np.where(k2, c1_[k], np.where(k1, c0_[k], c2_[k])) for k in range(3)]
            A, Bq, Cq = _quad(D1, u, u), _quad(D1, u, w), _quad(D1, w, w)
            disc = Bq * Bq
            disc = disc - A * Cq
            real = disc >= 0
            r = np.sqrt(disc)
            q = np.where(Bq >= 0, Bq + r, Bq - r)
            q = -q
            for sg, ta in ((q, A), (Cq, q)):
                d = [sg * u[k] + ta * w[k] for k in range(3)]
                Q = _side(d, 0, 1, b12) + _side(d, 0, 2, b13)
                Q = Q + _side(d, 1, 2, b23)
                s = asum / Q
                s = np.sqrt(s)
                s = np.where(d[0] < 0, -s, s)
                L = [s * d[k] for k in range(3)]
                ok = good & real & (L[0] > 0) & (L[1] > 0) & (L[2] > 0)
                c = [[L[i] * y[i][k] for k in range(3)] for i in range(3)]
                f1 = [c[1][k] - c[0][k] for k in range(3)]
                f2 = [c[2][k] - c[0][k] for k in range(3)]
                f3 = _cross(f1, f2)
                R = [[None] * 3 for _ in range(3)]
                for i in range(3):
                    for j in range(3):
                        v = f1[i] * g1[j]
                        v = v + f2[i] * g2[j]
                        R[i][j] = v + f3[i] * g3[j]
                t = []
                for i in range(3):
                    v = R[i][0] * X[0][0]
                    v = v + R[i][1] * X[0][1]
                    v = v + R[i][2] * X[0][2]
                    t.append(c[0][i] - v)
                for i in range(3):
                    ok = ok & (np.abs(t[i]) <= DBL_MAX)
                    for j in range(3):
                        ok = ok & (np.abs(R[i][j]) <= DBL_MAX)
                Rs.append(R); ts.append(t); oks.append(ok)
    return np.array(Rs), np.array(ts), np.array(oks)


def row_chi2(R, t, rows, K):
    """(depth, chi2) of rows [n] (float64 columns u, v, X, Y, Z, w as a [6][n] list) under poses R [3][3][...], t [3][...]; the
    poses' trailing shape broadcasts against [n]"""
    fx, fy, cx, cy = (F64(k) for k in K)
    u, v, X, Y, Z, w = rows
    with np.errstate(all="ignore"):
        pc = []
        for i in range(3):
            a = R[i][0] * X
            a = a + R[i][1] * Y
            a = a + R[i][2] * Z
            pc.append(a + t[i])
        pu = pc[0] / pc[2]
        pu = fx * pu
        pu = pu + cx
        pv = pc[1] / pc[2]
        pv = fy * pv
        pv = pv + cy
        du = u - pu
        dv = v - pv
        e = du * du
        e = e + dv * dv
        return pc[2], e * w


def inliers(R, t, rows, K, chi2_max):
    with np.errstate(all="ignore"):
        z, c = row_chi2(R, t, rows, K)
        return (z > 0) & (c <= F64(chi2_max))


def _rows64(obs, n):
    return [np.asarray(obs[f][:n], F32).astype(F64) for f in ("u", "v", "X", "Y", "Z", "inv_sigma2")]


def ransac(K, obs, n=None, hypotheses=HYPOTHESES, chi2_max=CHI2_MAX, seed=0, prior=None):
    """One problem: obs an OBS record array (pitch rows), n its count (clamped to the pitch). Returns a dict: Tcw float64 4 x 4 (the
    winning pose; the prior or the identity when void), Tcw32 its float32 rounding, consensus, inlier uint8 [pitch], winner (h, s),
    flags, chi2 float64 [n] of the rows under the winner (None when void), counts int64 [H][4] (-1 where no solution)."""
    pitch = len(obs)
    n = pitch if n is None else min(max(int(n), 0), pitch)
    H = int(hypotheses)
    T0 = np.eye(4) if prior is None else np.asarray(prior, F32).reshape(4, 4).astype(F64)
    out = dict(Tcw=T0.copy(), consensus=0, inlier=np.zeros(pitch, np.uint8), winner=(-2, 0), flags=FLAG_VOID, chi2=None,
               counts=np.full((H, 4), -1, np.int64))
    out["Tcw32"] = out["Tcw"].astype(F32)
    if n < 3:
        return out
    rows = _rows64(obs, n)
    idx, ok_s = sample(seed, H, n)
    ii = np.where(idx < 0, 0, idx)
    uv = [[rows[0][ii[:, i]], rows[1][ii[:, i]]] for i in range(3)]
    Xs = [[rows[2 + k][ii[:, i]] for k in range(3)] for i in range(3)]
    R, t, ok = solve_p3p(uv, Xs, K)            # [4][3][3][H], [4][3][H], [4][H]
    ok = ok & ok_s[None, :]
    counts = np.full((H, 4), -1, np.int64)
    for s in range(4):
        Rb = [[R[s, i, j][:, None] for j in range(3)] for i in range(3)]
        tb = [t[s, i][:, None] for i in range(3)]
        inl = inliers(Rb, tb, [c[None, :] for c in rows], K, chi2_max)
        counts[:, s] = np.where(ok[s], inl.sum(1), -1)
    out["counts"] = counts
    best, win = -1, (-2, 0)
    Rw = tw = None
    if prior is not None:
        Rw = [[T0[i, j] for j in range(3)] for i in range(3)]
        tw = [T0[i, 3] for i in range(3)]
        best, win = int(inliers(Rw, tw, rows, K, chi2_max).sum()), (-1, 0)
    flat = counts.reshape(-1)
    if flat.max() > best:
        a = int(np.argmax(flat))               # the first maximum: the lower hypothesis, then the lower solution
        h, s = divmod(a, 4)
        best, win = int(flat[a]), (h, s)
        Rw = [[R[s, i, j, h] for j in range(3)] for i in range(3)]
        tw = [t[s, i, h] for i in range(3)]
    if win[0] == -2:
        return out
    T = np.eye(4)
    for i in range(3):
        T[i, :3] = Rw[i]
        T[i, 3] = tw[i]
    z, c = row_chi2(Rw, tw, rows, K)
    mask = np.zeros(pitch, np.uint8)
    with np.errstate(all="ignore"):
        mask[:n] = (z > 0) & (c <= F64(chi2_max))
    assert int(mask.sum()) == best
    out.update(Tcw=T, Tcw32=T.astype(F32), consensus=best, inlier=mask, winner=win, flags=0, chi2=c)
    return out


def ransac_batch(K, obs, counts, hypotheses=HYPOTHESES, chi2_max=CHI2_MAX, seed=0, priors=None):
    """tb_pnp_ransac_batch_dev on the host: obs [nproblems][pitch] OBS, counts [nproblems], priors [nproblems][4][4] or None. A
    list of ransac()'s dicts."""
    return [ransac(K, obs[p], counts[p], hypotheses, chi2_max, seed, None if priors is None else priors[p]) for p in range(len(obs))]


def margin(res, chi2_max=CHI2_MAX):
    """the smallest relative distance of a row's chi2 under the winner from chi2_max (inf when void)"""
    if res["chi2"] is None:
        return np.inf
    c = res["chi2"][np.isfinite(res["chi2"])]
    return float(np.min(np.abs(c - chi2_max)) / chi2_max) if len(c) else np.inf
