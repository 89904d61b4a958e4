"""The batched OptimizeSim3 in numpy float64, from its definitions: the yardstick of tb_sim3_optimize_batch_dev (k_sim3_opt.hip).

The unknown is one similarity S12 = (s, R12, t12), X1 = s R12 X2 + t12, refined on the two-image reprojection cost of ORB-SLAM's
Optimizer::OptimizeSim3 from a seed (k_sim3's winner). The group, Exp and the srt records are pose_graph_sim3_reference's.

Rows. A row (OBS_ROW, twelve floats) holds the same physical point in camera-1 and camera-2 coordinates, the pixels (u1, v1) and
(u2, v2) of the two keys that observe it and the two keys' invLevelSigma2. One K = fx, fy, cx, cy serves both cameras;
proj(X) = (fx X / Z + cx, fy Y / Z + cy).

Cost. With Q1 = s R12 X2 + t12 and Q2 = S12^-1 X1 = R12' (X1 - t12) / s a row has two edges

    e12 = (u1, v1) - proj(Q1),  c1 = inv_sigma2_1 |e12|^2          e21 = (u2, v2) - proj(Q2),  c2 = inv_sigma2_2 |e21|^2

(c: the edge's plain chi2) and each goes under g2o's Huber kernel with delta = sqrt(th2): rho(c) = c and rho' = 1 where
sqrt(c) <= delta, otherwise rho(c) = 2 sqrt(c) delta - th2 and rho' = delta / sqrt(c). The robust chi2 of a transform is the sum of
rho over both edges of the active rows; it is +inf where an active row's Q1z or Q2z is not above 0.

Update and Jacobians. S <- Exp(delta) S, delta = (omega, upsilon, sigma). To first order Exp(delta) X = X + omega x X + upsilon +
sigma X, and S^-1 becomes S^-1 Exp(-delta), so

    dQ1 / ddelta = [-[Q1]x | I | Q1]                      dQ2 / ddelta = -(1 / s) R12' [-[X1]x | I | X1]
    de / ddelta = -P(Q) dQ / ddelta,    P(Q) = [[fx / Z, 0, -fx X / Z^2], [0, fy / Z, -fy Y / Z^2]]

exactly. H = sum J' (w rho') J and g = -sum J' (w rho') e over both edges of the active rows; with fixed_scale the seventh column
is left out, sigma = 0, and s keeps its bytes.

Sums. Row i belongs to slot i mod 256; a slot adds its rows in ascending order to 0.0 and the 256 partial sums meet in the
butterfly p[t] = p[t] + p[t ^ d], d = 1, 2, 4, ..., 128 (k_sim3's rule), for each of the 28 + 7 + 1 sums.

LM. One round of `iters` iterations is k_pgo's rule unchanged (pose_graph_reference.solve): lambda0 = 1e-5 max |diag H| at the
round's first iteration; a trial solves (H + lambda I) x = g by pose_graph_reference.cholesky_solve (a failed factorisation is a
trial of chi2 DBL_MAX), rho = (cur - trial) / (x . (lambda x + g) + 1e-3) with the exact robust chi2 of the trial; accepted on
rho > 0 and a finite trial: lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2; otherwise lambda *= nu, nu *= 2; at most 10
trials an iteration; the round stops after 10 rejections, at rho == 0 or after `iters`.

Procedure (ORB-SLAM's).
  0. A seed with a non-finite entry, a quaternion of norm 0 (or a non-finite norm) or s not above 0 is malformed: stats[7] = -1,
     srt_out = srt_in byte for byte, S12 the identity, no inliers, the other stats 0. Otherwise the quaternion is normalised
     (w >= 0, unit). The count is clamped to [0, pitch]. The rows that start active are those of active_in (None: all) below the
     count; of these a row with a non-finite field, with Z1 or Z2 not above 0, or with Q1z or Q2z not above 0 under the seed is
     dropped (stats[5] counts them).
  1. Fewer than min_keep rows active: stop as in 3. Otherwise `iters_first` LM iterations on the active rows.
  2. A row is bad where either of its edges' plain chi2 exceeds th2 under the result; bad rows leave (nBad, stats[4]).
  3. Fewer than min_keep rows left: the problem stops: inliers 0, an all-zero mask, srt_out = srt_in byte for byte, S12 the seed's,
     stats[7] = 1.
  4. Otherwise a second round of `iters_bad` iterations if nBad > 0, else `iters_clean`, on the rows left (lambda starts anew, as
     a second g2o optimize() call does).
  5. The mask marks the rows still active whose two chi2 are both at most th2 under the final transform; inliers is their count.
stats = iterations run, initial robust chi2 (the starting rows under the seed), final robust chi2 (the rows left under the final
transform), trials, nBad, dropped rows, final lambda, flag. A problem that accepted no trial returns srt_in byte for byte.
"""
import numpy as np

import pose_graph_reference as pg
import pose_graph_sim3_reference as ps

OBS_ROW = np.dtype([("X1", "<f4"), ("Y1", "<f4"), ("Z1", "<f4"), ("X2", "<f4"), ("Y2", "<f4"), ("Z2", "<f4"), ("u1", "<f4"), ("v1", "<f4"),
                    ("u2", "<f4"), ("v2", "<f4"), ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
FIELDS = OBS_ROW.names
SLOTS = 256
TH2 = 10.0           # ORB-SLAM's th2 (LoopClosing calls OptimizeSim3 with 10): a default, not a measurement
ITERS_FIRST, ITERS_BAD, ITERS_CLEAN, MIN_KEEP = 5, 10, 5, 10
DBL_MAX = np.finfo(np.float64).max
FLAG_STOPPED, FLAG_MALFORMED = 1, -1
IDENT_SRT = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])


def project(X, K):
    X = np.asarray(X, np.float64)
    return np.stack([K[0] * X[..., 0] / X[..., 2] + K[2], K[1] * X[..., 1] / X[..., 2] + K[3]], -1)


def make_rows(X1, X2, uv1, uv2, w1=None, w2=None, pitch=None):
    n = len(X1)
    rows = np.zeros(n if pitch is None else pitch, OBS_ROW)
    for k, (a, b) in enumerate((("X1", "X2"), ("Y1", "Y2"), ("Z1", "Z2"))):
        rows[a][:n], rows[b][:n] = X1[:, k], X2[:, k]
    rows["u1"][:n], rows["v1"][:n], rows["u2"][:n], rows["v2"][:n] = uv1[:, 0], uv1[:, 1], uv2[:, 0], uv2[:, 1]
    rows["inv_sigma2_1"][:n] = 1.0 if w1 is None else w1
    rows["inv_sigma2_2"][:n] = 1.0 if w2 is None else w2
    return rows


def _fields(rows):
    r = {f: rows[f].astype(np.float64) for f in FIELDS}
    return (np.stack([r["X1"], r["Y1"], r["Z1"]], -1), np.stack([r["X2"], r["Y2"], r["Z2"]], -1), np.stack([r["u1"], r["v1"]], -1),
            np.stack([r["u2"], r["v2"]], -1), r["inv_sigma2_1"], r["inv_sigma2_2"])


def mapped(S, X1, X2):
    """(Q1, Q2) of every row under the 4 x 4 S"""
    s, R, t = ps.parts(S)
    return s * X2 @ R.T + t, ((X1 - t) @ R) / s


def row_chi2(S, rows, K):
    """(c1, c2, Q1z, Q2z) of every row: the two edges' plain chi2 and the two mapped depths"""
    X1, X2, uv1, uv2, w1, w2 = _fields(rows)
    Q1, Q2 = mapped(S, X1, X2)
    with np.errstate(all="ignore"):
        e1, e2 = uv1 - project(Q1, K), uv2 - project(Q2, K)
        return w1 * (e1 ** 2).sum(-1), w2 * (e2 ** 2).sum(-1), Q1[:, 2], Q2[:, 2]


def huber(c, th2):
    """(rho, rho') of g2o's RobustKernelHuber with delta = sqrt(th2) on the plain chi2 c"""
    delta, sq = np.sqrt(th2), np.sqrt(c)
    big = sq > delta
    with np.errstate(all="ignore"):
        return np.where(big, 2 * sq * delta - th2, c), np.where(big, delta / sq, 1.0)


def total(v, idx):
    """the sum of v[k] (belonging to row idx[k], ascending) by the kernel's rule; v [m] or [m, c]"""
    v = np.asarray(v, np.float64)
    part = np.zeros((SLOTS,) + v.shape[1:])
    for k, i in enumerate(idx):
        part[i % SLOTS] = part[i % SLOTS] + v[k]
    t = np.arange(SLOTS)
    d = 1
    while d < SLOTS:
        part = part + part[t ^ d]
        d *= 2
    return part[0]


def jacobians(S, X1, X2, K):
    """(J1, J2) [m, 2, 7]: de12 / ddelta and de21 / ddelta of every row at S"""
    s, R, t = ps.parts(S)
    Q1, Q2 = mapped(S, X1, X2)
    m = len(X1)

    def dproj(Q):
        P = np.zeros((m, 2, 3))
        P[:, 0, 0], P[:, 0, 2] = K[0] / Q[:, 2], -K[0] * Q[:, 0] / Q[:, 2] ** 2
        P[:, 1, 1], P[:, 1, 2] = K[1] / Q[:, 2], -K[1] * Q[:, 1] / Q[:, 2] ** 2
        return P

    def dpoint(X):
        D = np.zeros((m, 3, 7))
        for k in range(m):
            D[k, :, :3] = -pg.hat(X[k])
        D[:, :, 3:6] = np.eye(3)
        D[:, :, 6] = X
        return D

    J1 = -dproj(Q1) @ dpoint(Q1)
    J2 = -dproj(Q2) @ (-(1.0 / s) * (R.T @ dpoint(X1)))
    return J1, J2


def evaluate(S, rows, idx, K, th2, D=7, linearise=True):
    """the robust chi2 of the rows idx (ascending) under S, and (H, g) if asked for"""
    r = rows[idx]
    X1, X2, uv1, uv2, w1, w2 = _fields(r)
    c1, c2, z1, z2 = row_chi2(S, r, K)
    if np.any(~(z1 > 0)) or np.any(~(z2 > 0)):
        return np.inf, None, None
    (r1, d1), (r2, d2) = huber(c1, th2), huber(c2, th2)
    chi = float(total(r1 + r2, idx))
    if not linearise:
        return chi, None, None
    Q1, Q2 = mapped(S, X1, X2)
    e1, e2 = uv1 - project(Q1, K), uv2 - project(Q2, K)
    J1, J2 = jacobians(S, X1, X2, K)
    J1, J2 = J1[:, :, :D], J2[:, :, :D]
    a1, a2 = (w1 * d1)[:, None, None], (w2 * d2)[:, None, None]
    Hr = a1 * (J1.transpose(0, 2, 1) @ J1) + a2 * (J2.transpose(0, 2, 1) @ J2)
    gr = -((a1 * J1.transpose(0, 2, 1)) @ e1[:, :, None] + (a2 * J2.transpose(0, 2, 1)) @ e2[:, :, None])[:, :, 0]
    return chi, total(Hr.reshape(len(idx), -1), idx).reshape(D, D), total(gr, idx)


def lm_round(S, rows, idx, K, th2, iters, D, trace, rnd):
    """(S, chi2, lambda, iterations, trials, accepted any) of one round"""
    cur = evaluate(S, rows, idx, K, th2, D, False)[0]
    lam, nu, done, trials, any_acc, ok = 0.0, 2.0, 0, 0, False, True
    for it in range(iters):
        if not ok:
            break
        _, H, g = evaluate(S, rows, idx, K, th2, D)
        if it == 0:
            lam, nu = 1e-5 * np.abs(np.diag(H)).max(), 2.0
        rho, q = 0.0, 0
        while True:
            x = pg.cholesky_solve(H + lam * np.eye(D), g)
            solved = x is not None
            if not solved:
                x = np.zeros(D)
            d = np.zeros(7)
            d[:D] = x
            Sn = ps.exp(d) @ S
            trial = evaluate(Sn, rows, idx, K, th2, D, False)[0] if solved else DBL_MAX
            with np.errstate(all="ignore"):
                rho = (cur - trial) / (float(x @ (lam * x + g)) + 1e-3)
            acc = bool(rho > 0 and np.isfinite(trial))
            if trace is not None:
                trace.append((rnd, it, q, rho, acc, cur, trial))
            if acc:
                lam *= max(1.0 / 3, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3))
                nu = 2.0
                cur, S, any_acc = trial, Sn, True
            else:
                lam *= nu
                nu *= 2
            q += 1
            trials += 1
            if not (rho < 0 and q < 10):
                break
        done += 1
        if q == 10 or rho == 0:
            ok = False
    return S, cur, lam, done, trials, any_acc


def malformed(srt):
    return ps._bad_srt(srt)


def s12_f32(S):
    M = np.array(S, np.float64)
    M[3] = (0, 0, 0, 1)
    return M.astype(np.float32)


def optimize(K, rows, n, srt0, active=None, fixed_scale=False, th2=TH2, iters_first=ITERS_FIRST, iters_bad=ITERS_BAD,
             iters_clean=ITERS_CLEAN, min_keep=MIN_KEEP, trace=None, gates=None):
    """One problem. rows OBS_ROW [pitch], n the count, srt0 [8]. Returns dict(srt [8], S12 float32 [4, 4], inliers, mask uint8
    [pitch], stats [8]). trace (a list) receives (round, iteration, trial, rho, accepted, chi2 before, chi2 of the trial) of every
    trial; gates (a list) receives every plain chi2 that steps 2 and 5 compare with th2."""
    pitch = len(rows)
    n = min(max(int(n), 0), pitch)
    srt0 = np.array(srt0, np.float64)
    out = dict(srt=srt0.copy(), S12=np.eye(4, dtype=np.float32), inliers=0, mask=np.zeros(pitch, np.uint8), stats=np.zeros(8))
    if malformed(srt0):
        out["stats"][7] = FLAG_MALFORMED
        return out
    S = ps.srt_to_matrix(srt0)
    out["S12"] = s12_f32(S)
    D = 6 if fixed_scale else 7
    start = np.ones(n, bool) if active is None else np.asarray(active[:n]) != 0
    raw = np.stack([rows[f][:n].astype(np.float64) for f in FIELDS], -1) if n else np.zeros((0, 12))
    c1, c2, z1, z2 = row_chi2(S, rows[:n], K)
    with np.errstate(all="ignore"):
        good = np.isfinite(raw).all(-1) & (raw[:, 2] > 0) & (raw[:, 5] > 0) & (z1 > 0) & (z2 > 0)
    act = start & good
    st = out["stats"]
    st[5] = int((start & ~good).sum())
    idx = np.flatnonzero(act)
    st[1] = st[2] = evaluate(S, rows, idx, K, th2, D, False)[0]
    if len(idx) < min_keep:
        st[7] = FLAG_STOPPED
        return out
    S1, cur, lam, done, trials, acc1 = lm_round(S, rows, idx, K, th2, iters_first, D, trace, 0)
    c1, c2, _, _ = row_chi2(S1, rows[:n], K)
    if gates is not None:
        gates.extend(list(c1[idx]) + list(c2[idx]))
    bad = act & ((c1 > th2) | (c2 > th2))
    nbad = int(bad.sum())
    act = act & ~bad
    idx = np.flatnonzero(act)
    st[0], st[2], st[3], st[4], st[6] = done, cur, trials, nbad, lam
    if len(idx) < min_keep:
        st[7] = FLAG_STOPPED
        return out
    S2, cur, lam, done2, trials2, acc2 = lm_round(S1, rows, idx, K, th2, iters_bad if nbad > 0 else iters_clean, D, trace, 1)
    c1, c2, _, _ = row_chi2(S2, rows[:n], K)
    if gates is not None:
        gates.extend(list(c1[idx]) + list(c2[idx]))
    inl = act & (c1 <= th2) & (c2 <= th2)
    out["mask"][:n] = inl
    out["inliers"] = int(inl.sum())
    st[0], st[2], st[3], st[6] = done + done2, cur, trials + trials2, lam
    if acc1 or acc2:
        v = ps.srt_from_matrix(S2)
        if fixed_scale:
            v[7] = srt0[7]
        out["srt"] = v
    out["S12"] = s12_f32(S2)
    return out


def optimize_batch(K, rows, counts, srt0, active=None, **kw):
    """rows [P, pitch], counts [P], srt0 [P, 8], active None or [P, pitch] -> list of optimize()'s dicts"""
    return [optimize(K, rows[p], counts[p], srt0[p], None if active is None else active[p], **kw) for p in range(len(rows))]


def margins(trace, gates, th2=TH2):
    """(the closest accept / reject decision, relative to the chi2 before it; the closest gated chi2 to th2, relative to th2)"""
    with np.errstate(all="ignore"):
        dec = min([abs(t[5] - t[6]) / t[5] if t[5] > 0 else 0.0 for t in trace], default=np.inf)
    gate = min([abs(c - th2) / th2 for c in gates], default=np.inf) if th2 > 0 else np.inf
    return dec, gate


def cost(S, rows, idx, K, th2=TH2):
    """the robust chi2 as a plain numpy sum, for optimisers outside this file"""
    c1, c2, _, _ = row_chi2(S, rows[idx], K)
    return float((huber(c1, th2)[0] + huber(c2, th2)[0]).sum())
