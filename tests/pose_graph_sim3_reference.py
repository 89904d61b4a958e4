"""The batched Sim(3) pose-graph optimiser in numpy float64, from its definitions: the yardstick of tb_pose_graph_sim3_batch_dev.

Element and tangent. S = (s, R, t) acts as X' = s R X + t; as a matrix [[sR, t], [0, 1]], so composition is the 4 x 4 product and
the inverse is (1/s, R', -(R' t) / s). The tangent vector is u = (omega, upsilon, sigma), the solvers' (omega, upsilon) with the
log-scale appended (g2o's Sim3). Exp(u) = (e^sigma, exp(omega), W upsilon) with

    W = int_0^1 e^(sigma tau) exp(tau Omega) dtau = C I + A Omega + B Omega^2,      Omega = [omega]x, theta = |omega|,
    C = g_0(sigma),    A = Im phi(sigma + i theta) / theta,    B = (C - Re phi(sigma + i theta)) / theta^2,
    phi(z) = (e^z - 1) / z = int_0^1 e^(z tau) dtau,    g_k(sigma) = int_0^1 tau^k e^(sigma tau) dtau = phi^(k)(sigma).

With sigma = 0: C = 1, A = (1 - cos theta) / theta^2, B = (theta - sin theta) / theta^3, SE(3)'s V. Log inverts it: sigma = log s,
omega from the unit quaternion of R as pose_graph_reference.log takes it, upsilon = W^-1 t (W is a 3 x 3 solve; its eigenvalues are
phi(sigma) and phi(sigma +- i theta), which vanish only at sigma = 0, theta = 2 pi, outside Log's range theta <= pi).

Where the closed forms cancel, and what replaces them:
  theta >= SMALL: A = (e^sigma (sigma sin theta - theta cos theta) + theta) / (theta (sigma^2 + theta^2)) and
      B = (C - (e^sigma (sigma cos theta + theta sin theta) - sigma) / (sigma^2 + theta^2)) / theta^2 lose no more than the SE(3)
      coefficients do at the same angle (at sigma = 0 they are those coefficients).
  theta < SMALL: both cancel like theta^2. Taylor's expansion of phi about sigma in i theta gives alternating series
      A = g_1 - g_3 theta^2 / 3! + g_5 theta^4 / 5! - g_7 theta^6 / 7!,   B = g_2 / 2! - g_4 theta^2 / 4! + g_6 theta^4 / 6! - g_8 theta^6 / 8!.
      0 <= tau <= 1 makes g_k decrease in k, so the terms decrease and the truncation is below the first term left out:
      relative to the leading term at most theta^8 / 9! = 2.8e-14 for A and 2 theta^8 / 10! = 5.6e-15 for B at theta = SMALL = 0.1.
      Three terms would leave theta^6 / 7! = 2.0e-10 and 2 theta^6 / 8! = 5.0e-11, above the 2e-11 wanted: hence N_THETA = 4.
  g_k, |sigma| >= SMALL_S: g_0 = (e^sigma - 1) / sigma and g_k = (e^sigma - k g_(k-1)) / sigma. Each step multiplies the error by
      k / |sigma|, so g_k carries about eps k! / |sigma|^k; it enters A and B with theta^(k-1) / k! or theta^(k-2) / k!, which
      leaves eps / |sigma| (theta / |sigma|)^(k-1) <= 10 eps, theta < SMALL <= |sigma|. Only g_0 is needed when theta >= SMALL.
  g_k, |sigma| < SMALL_S: g_k = sum_m sigma^m / (m! (m + k + 1)), m = 0 .. N_SIGMA - 1. The terms are bounded by |sigma|^m / m!, the
      truncation relative to g_k (>= e^-|sigma| / (k + 1)) by (k + 1) / (N_SIGMA + k + 1) |sigma|^N_SIGMA / N_SIGMA! e^(2 |sigma|): with N_SIGMA = 8 at
      |sigma| = 0.1 that is 1e-8 / 40320 * 1.22 = 3.0e-13 (seven terms would give 2.4e-11, above 2e-11): hence N_SIGMA = 8.

Residual, cost, update. With E = Z^-1 S_b S_a^-1, r = Log(E), chi2 = sum r' diag(w_rot I3, w_trans I3, w_scale) r, S <- Exp(delta) S,
no robust kernel. Jacobians for those left perturbations:

    J_b = Jl^-1(r) Ad(Z^-1),     J_a = -Jl^-1(r) Ad(E),     Ad(S)(omega, upsilon, sigma) = (R omega, s R upsilon + [t]x R omega - sigma t, sigma),
    ad(r) = [[Omega, 0, 0], [Upsilon, Omega + sigma I, -upsilon], [0, 0, 0]]   (d/d eps of Ad(Exp(eps r)) at 0).

Jl^-1(r) = sum_n B_n / n! ad(r)^n (B_1 = -1/2, the odd B_n above 1 vanish) is summed to the fixed order JL_ORDER for every input, by
Horner's rule in ad^2, so the control flow is uniform. JL_ORDER = 22 is the smallest even order for which both Jacobians agree
with (five-point) central differences to 1e-9 over the domain |omega| <= 2 rad, |sigma| <= 1, |upsilon| <= 5 (4000 draws, the
norms at the domain's edge in a quarter of them: worst difference 4.8e-10; order 20 leaves 3.6e-9, and the differences' own floor
is 4e-12). The series converges for
|eigenvalues of ad| = |sigma +- i theta| < 2 pi and its tail is governed by (sqrt(5) / 2 pi)^n = 0.356^n there. Outside the domain the
Jacobians degrade gradually; LM stays safe because a trial is accepted on the exact chi2, never on the model.

LM. k_pgo's rule unchanged (pose_graph_reference.solve): lambda0 = 1e-5 max diag H; accept on rho > 0 and a finite chi2, then
lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2; otherwise lambda *= nu, nu *= 2; at most 10 trials per iteration; stop at 10
rejections, at rho == 0 or after `iters`; pose_graph_reference.cholesky_solve's dense Cholesky.

fixed_scale (ORB-SLAM's bFixScale): every free node has 6 unknowns (omega, upsilon) and its s keeps its bytes; the residual's
seventh component still counts. With every scale exactly 1 this is the SE(3) pose graph.

Nodes are float64 [nnodes][8] in k_sim3's srt layout: the quaternion w x y z, t, s; edges carry Z ~ S_b S_a^-1 in the same layout.
Quaternions are normalised on entry (w >= 0, unit). A graph that is malformed (stats[7] = -1), has no edge, or accepted no step
keeps every byte of its nodes, and fixed nodes always do.
"""
import numpy as np

import pose_graph_reference as pg

SMALL = 0.1      # rotation angle below which A and B take their series in theta
SMALL_S = 0.1    # |sigma| below which the g_k take their series in sigma
N_THETA = 4      # terms of the series in theta^2
N_SIGMA = 8      # terms of the series in sigma
JL_ORDER = 22    # highest power of ad(r) in Jl^-1
# domain over which JL_ORDER was chosen, and what was measured there (test_pose_graph_sim3_reference.py measures it again)
JL_DOMAIN = dict(omega=2.0, upsilon=5.0, sigma=1.0)
JL_WORST = 4.8e-10
EDGE = np.dtype([("a", "<i4"), ("b", "<i4"), ("srt", "<f8", (8,)), ("w_rot", "<f8"), ("w_trans", "<f8"), ("w_scale", "<f8")])
MAX_NODES, MAX_EDGES = pg.MAX_NODES, pg.MAX_EDGES

hat = pg.hat


def _bernoulli_over_factorial(order):
    """B_n / n! for n = 0 .. order (B_1 = -1/2), exact rationals rounded once"""
    from fractions import Fraction
    from math import comb, factorial
    B = [Fraction(1)]
    for n in range(1, order + 1):
        B.append(-sum(comb(n + 1, k) * B[k] for k in range(n)) / (n + 1))
    return [float(B[n] / factorial(n)) for n in range(order + 1)]


JL_COEFF = _bernoulli_over_factorial(JL_ORDER)


# ---------------------------------------------------------------- the group
def g_coeffs(sigma, kmax):
    """g_k(sigma) = int_0^1 tau^k e^(sigma tau) dtau, k = 0 .. kmax"""
    g = np.zeros(kmax + 1)
    if abs(sigma) < SMALL_S:
        for k in range(kmax + 1):
            term, acc = 1.0, 0.0          # term = sigma^m / m!
            for m in range(N_SIGMA):
                acc += term / (m + k + 1)
                term *= sigma / (m + 1)
            g[k] = acc
    else:
        es = np.exp(sigma)
        g[0] = (es - 1.0) / sigma
        for k in range(1, kmax + 1):
            g[k] = (es - k * g[k - 1]) / sigma
    return g


def w_coeffs(theta, sigma):
    """(A, B, C) of W = C I + A Omega + B Omega^2"""
    if theta < SMALL:
        g = g_coeffs(sigma, 2 * N_THETA)
        t2 = theta * theta
        A = g[1] - t2 * (g[3] / 6 - t2 * (g[5] / 120 - t2 * g[7] / 5040))
        B = g[2] / 2 - t2 * (g[4] / 24 - t2 * (g[6] / 720 - t2 * g[8] / 40320))
        return A, B, g[0]
    C = g_coeffs(sigma, 0)[0]
    es, sn, cs = np.exp(sigma), np.sin(theta), np.cos(theta)
    d = sigma * sigma + theta * theta
    A = (es * (sigma * sn - theta * cs) + theta) / (theta * d)
    B = (C - (es * (sigma * cs + theta * sn) - sigma) / d) / (theta * theta)
    return A, B, C


def w_matrix(omega, sigma):
    th = np.sqrt((np.asarray(omega) ** 2).sum())
    A, B, C = w_coeffs(th, sigma)
    Om = hat(omega)
    return C * np.eye(3) + A * Om + B * (Om @ Om)


def make(s, R, t):
    S = np.eye(4)
    S[:3, :3] = s * np.asarray(R, np.float64)
    S[:3, 3] = t
    return S


def parts(S):
    """(s, R, t) of a 4 x 4 [[sR, t], [0, 1]]: s from the determinant, so that R is a rotation to rounding"""
    s = np.cbrt(np.linalg.det(S[:3, :3]))
    return s, S[:3, :3] / s, S[:3, 3].copy()


def inv(S):
    s, R, t = parts(S)
    return make(1.0 / s, R.T, -(R.T @ t) / s)


def exp(u):
    u = np.asarray(u, np.float64)
    om, sigma = u[:3], u[6]
    th = np.sqrt((om ** 2).sum())
    Om = hat(om)
    if th < 0.00001:                       # pose_graph_reference.exp's rule for R
        a, b = 1.0, 0.5
    else:
        a, b = np.sin(th) / th, (1 - np.cos(th)) / th ** 2
    R = np.eye(3) + a * Om + b * (Om @ Om)
    return make(np.exp(sigma), R, w_matrix(om, sigma) @ u[3:6])


def log(S):
    s, R, t = parts(S)
    q = pg.quat_from_R(R)
    n = np.sqrt((q[:3] ** 2).sum())
    th = 2.0 * np.arctan2(n, q[3])
    om = q[:3] * (2.0 / q[3]) if th < 0.00001 else q[:3] * (th / n)
    sigma = np.log(s)
    return np.concatenate([om, np.linalg.solve(w_matrix(om, sigma), t), [sigma]])


def adjoint(S):
    s, R, t = parts(S)
    A = np.zeros((7, 7))
    A[:3, :3] = R
    A[3:6, :3] = hat(t) @ R
    A[3:6, 3:6] = s * R
    A[3:6, 6] = -t
    A[6, 6] = 1.0
    return A


def ad(r):
    M = np.zeros((7, 7))
    M[:3, :3] = hat(r[:3])
    M[3:6, :3] = hat(r[3:6])
    M[3:6, 3:6] = hat(r[:3]) + r[6] * np.eye(3)
    M[3:6, 6] = -np.asarray(r[3:6])
    return M


def jl_inv(r, order=JL_ORDER):
    """sum_{n <= order} B_n / n! ad(r)^n: I - ad / 2 + (Horner in ad^2 over the even orders)"""
    coeff = JL_COEFF if order <= JL_ORDER else _bernoulli_over_factorial(order)
    M = ad(np.asarray(r, np.float64))
    P = M @ M
    I = np.eye(7)
    S = coeff[order - order % 2] * I
    for n in range(order - order % 2 - 2, -1, -2):
        S = S @ P + coeff[n] * I
    return S - 0.5 * M


# ---------------------------------------------------------------- records
def quat_wxyz_from_R(R):
    q = pg.quat_from_R(R)
    return np.array([q[3], q[0], q[1], q[2]])


def srt_from_matrix(S):
    s, R, t = parts(np.asarray(S, np.float64))
    return np.concatenate([quat_wxyz_from_R(R), t, [s]])


def srt_to_matrix(srt):
    """the element a record stands for, its quaternion normalised as the kernel normalises it (w >= 0, unit)"""
    srt = np.asarray(srt, np.float64)
    q = np.array([srt[1], srt[2], srt[3], srt[0]])
    if q[3] < 0:
        q = -q
    q = q / np.sqrt((q * q).sum())
    return make(srt[7], pg.R_from_quat(q), srt[4:7])


def srt_normalised(srt):
    srt = np.array(srt, np.float64)
    if srt[0] < 0:
        srt[:4] = -srt[:4]
    srt[:4] /= np.sqrt((srt[:4] ** 2).sum())
    return srt


def make_edge(a, b, Z, w_rot=1.0, w_trans=1.0, w_scale=1.0):
    e = np.zeros((), EDGE)
    e["a"], e["b"], e["w_rot"], e["w_trans"], e["w_scale"] = a, b, w_rot, w_trans, w_scale
    e["srt"] = srt_from_matrix(Z)
    return e


def residual(Z, Sa, Sb):
    return log(inv(Z) @ Sb @ inv(Sa))


def jacobians(Z, Sa, Sb):
    """(r, J_a, J_b), 7 x 7 each"""
    Zi = inv(Z)
    E = Zi @ Sb @ inv(Sa)
    r = log(E)
    Ji = jl_inv(r)
    return r, -Ji @ adjoint(E), Ji @ adjoint(Zi)


def _bad_srt(v):
    v = np.asarray(v, np.float64)
    n2 = float((v[:4] ** 2).sum())
    return not np.all(np.isfinite(v)) or not (n2 > 0 and np.isfinite(n2)) or not v[7] > 0


def malformed(nodes, edges):
    n = len(nodes)
    if any(_bad_srt(v) for v in nodes):
        return True
    for e in edges:
        a, b = int(e["a"]), int(e["b"])
        if a < 0 or a >= n or b < 0 or b >= n or a == b or _bad_srt(e["srt"]):
            return True
        w = np.array([e["w_rot"], e["w_trans"], e["w_scale"]])
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            return True
    return False


def _weights(e):
    return np.array([e["w_rot"]] * 3 + [e["w_trans"]] * 3 + [e["w_scale"]])


def chi2_of(S, edges, Zs):
    c = 0.0
    for e, Z in zip(edges, Zs):
        r = residual(Z, S[e["a"]], S[e["b"]])
        c += float((_weights(e) * r * r).sum())
    return c


def solve(nodes, nfixed, edges, iters=10, fixed_scale=False, trace=None):
    """One graph. nodes float64 [nnodes, 8] srt; edges an EDGE array. Returns (nodes [nnodes, 8], stats [8]): iterations, initial
    chi2, final chi2, final lambda, trials; stats[7] = -1 flags a malformed graph. trace (a list) receives (iteration, trial, rho,
    accepted, chi2 before, chi2 of the trial) of every trial."""
    nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 8)
    n = len(nodes)
    assert 1 <= nfixed < n <= MAX_NODES and len(edges) <= MAX_EDGES and iters >= 0
    stats = np.zeros(8)
    out = nodes.copy()
    if malformed(nodes, edges):
        stats[7] = -1
        return out, stats
    if len(edges) == 0:
        return out, stats
    S = [srt_to_matrix(v) for v in nodes]
    Zs = [srt_to_matrix(e["srt"]) for e in edges]
    D = 6 if fixed_scale else 7
    N = D * (n - nfixed)
    cur = chi2_of(S, edges, Zs)
    stats[1] = stats[2] = cur
    lam, nu, done, trials, accepted_any, ok = 0.0, 2.0, 0, 0, False, True
    for it in range(iters):
        if not ok:
            break
        H, g = np.zeros((N, N)), np.zeros(N)
        for e, Z in zip(edges, Zs):
            a, b = int(e["a"]), int(e["b"])
            r, Ja, Jb = jacobians(Z, S[a], S[b])
            Ja, Jb = Ja[:, :D], Jb[:, :D]
            W = _weights(e)
            for (i, Ji) in ((a, Ja), (b, Jb)):
                if i < nfixed:
                    continue
                oi = D * (i - nfixed)
                H[oi:oi + D, oi:oi + D] += Ji.T @ (W[:, None] * Ji)
                g[oi:oi + D] -= Ji.T @ (W * r)
            if a >= nfixed and b >= nfixed:
                oa, ob = D * (a - nfixed), D * (b - nfixed)
                blk = Ja.T @ (W[:, None] * Jb)
                H[oa:oa + D, ob:ob + D] += blk
                H[ob:ob + D, oa:oa + D] += blk.T
        if it == 0:
            lam, nu = 1e-5 * np.abs(np.diag(H)).max(), 2.0
        rho, q = 0.0, 0
        while True:
            x = pg.cholesky_solve(H + lam * np.eye(N), g)
            solved = x is not None
            if not solved:
                x = np.zeros(N)
            Sn = list(S)
            for k in range(nfixed, n):
                d = np.zeros(7)
                d[:D] = x[D * (k - nfixed):D * (k - nfixed) + D]
                Sn[k] = exp(d) @ S[k]
            trial = chi2_of(Sn, edges, Zs) if solved else np.finfo(np.float64).max
            rho = (cur - trial) / (float(x @ (lam * x + g)) + 1e-3)
            acc = bool(rho > 0 and np.isfinite(trial))
            if trace is not None:
                trace.append((it, q, rho, acc, cur, trial))
            if acc:
                lam *= max(1.0 / 3, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3))
                nu = 2.0
                cur, S, accepted_any = trial, Sn, True
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
    if accepted_any:
        for k in range(nfixed, n):
            v = srt_from_matrix(S[k])
            if fixed_scale:
                v[7] = nodes[k, 7]
            out[k] = v
    stats[0], stats[2], stats[3], stats[4] = done, cur, lam, trials
    return out, stats


def solve_batch(nodes, nfixed, edges, counts, iters=10, fixed_scale=False):
    """nodes [G, nnodes, 8], edges [G, pitch] EDGE, counts [G] (a count above the pitch or below 0 flags its graph)"""
    nodes = np.ascontiguousarray(nodes, np.float64)
    out, stats = nodes.copy(), np.zeros((len(nodes), 8))
    for g in range(len(nodes)):
        if counts[g] > edges.shape[1] or counts[g] < 0:
            stats[g, 7] = -1
            continue
        out[g], stats[g] = solve(nodes[g], nfixed, edges[g, :counts[g]], iters, fixed_scale)
    return out, stats


# ---------------------------------------------------------------- shared cases (CPU and GPU tests)
def nodes_from_se3(poses):
    """float32 / float64 [n, 4, 4] Tcw as the SE(3) solver takes them (pose_graph_reference.pose_in) -> srt nodes with s = 1"""
    return np.stack([np.concatenate([quat_wxyz_from_R(pg.pose_in(T)[:3, :3]), np.asarray(T, np.float64).reshape(4, 4)[:3, 3], [1.0]])
                     for T in poses])


def edges_from_se3(edges, w_scale=1.0):
    out = np.zeros(len(edges), EDGE)
    for k, e in enumerate(edges):
        q = pg.quat_from_R(pg.edge_Z(e)[:3, :3])
        out[k]["a"], out[k]["b"], out[k]["w_rot"], out[k]["w_trans"], out[k]["w_scale"] = e["a"], e["b"], e["w_rot"], e["w_trans"], w_scale
        out[k]["srt"] = np.concatenate([[q[3]], q[:3], e["t"], [1.0]])
    return out


def chain_graph(seed, nnodes, chords, odo_noise=(0.01, 0.02, 0.01), start_noise=(0.02, 0.05, 0.03), w=(1.0, 1.0, 1.0), reverse=(),
                scale_walk=0.05, step_scale=None):
    """A chain of `nnodes` similarity nodes (a camera path whose map scale wanders by exp(N(0, scale_walk)) per step) with noisy
    odometry edges and noisy chords [(a, b), ...] (repeats and a > b allowed), started off the truth. reverse: indices of edges
    listed as (b, a). step_scale {i: factor}: the step into node i multiplies the scale by that factor as well, for nodes and
    edges whose s is far from 1. Returns (nodes0 [nnodes, 8], edges)."""
    rng = np.random.default_rng(seed)
    truth = [np.eye(4)]
    for i in range(1, nnodes):
        step = exp(np.concatenate([rng.normal(0, 0.05, 3), np.array([0.0, 0.0, -0.5]) + rng.normal(0, 0.05, 3), rng.normal(0, scale_walk, 1)]))
        step = make((step_scale or {}).get(i, 1.0), np.eye(3), np.zeros(3)) @ step
        truth.append(step @ truth[-1])

    def noisy(S, sd):
        return exp(np.concatenate([rng.normal(0, sd[0], 3), rng.normal(0, sd[1], 3), rng.normal(0, sd[2], 1)])) @ S

    pairs = [(i, i + 1) for i in range(nnodes - 1)] + list(chords)
    edges = np.zeros(len(pairs), EDGE)
    for k, (a, b) in enumerate(pairs):
        if k in reverse:
            a, b = b, a
        edges[k] = make_edge(a, b, noisy(truth[b] @ inv(truth[a]), odo_noise), *w)
    nodes0 = np.stack([srt_from_matrix(truth[i] if i == 0 else noisy(truth[i], start_noise)) for i in range(nnodes)])
    return nodes0, edges


def circuit(seed, N, scale_bias=0.01, scale_sd=0.01, radius=10.0, noise=(0.01, 0.02)):
    """pose_graph_reference.circuit on a one-camera map whose scale drifts: every odometry edge multiplies the map scale k by
    exp(N(scale_bias, scale_sd)), so the motion it measures is [R_rel | k t_rel] (with the circuit's noise) and it believes the
    scale ratio to be 1. The estimate is that odometry integrated from node 0, every s = 1. The exact element of camera i is
    S_i = (k_i, R_i, k_i t_i) -- the world at node 0's scale into camera i at its own -- whose centre -R' t / s is the true one, and
    the one exact loop edge (0, N - 1) is S_(N-1) S_0^-1 = (k, R_rel, k t_rel).
    Returns (truth [N, 4, 4] Tcw, nodes0 [N, 8], edges, poses0 float32 [N, 4, 4], SE(3) edges): the last two are the same graph
    with the scales ignored, for pose_graph_reference.solve."""
    rng = np.random.default_rng(seed)
    truth = pg.circuit(seed, N, radius, noise)[0]
    edges, se3_edges, est, k = np.zeros(N, EDGE), np.zeros(N, pg.EDGE), [truth[0].copy()], 1.0
    for i in range(N - 1):
        k *= np.exp(rng.normal(scale_bias, scale_sd))
        rel = truth[i + 1] @ pg.inv(truth[i])
        rel[:3, 3] *= k
        Z = pg.exp(np.concatenate([rng.normal(0, noise[0], 3), rng.normal(0, noise[1], 3)])) @ rel
        edges[i], se3_edges[i] = make_edge(i, i + 1, Z), pg.make_edge(i, i + 1, Z)
        est.append(Z @ est[-1])
    rel = truth[N - 1] @ pg.inv(truth[0])
    edges[N - 1] = make_edge(0, N - 1, make(k, rel[:3, :3], k * rel[:3, 3]))
    se3_edges[N - 1] = pg.make_edge(0, N - 1, make(1.0, rel[:3, :3], k * rel[:3, 3]))
    nodes0 = np.stack([srt_from_matrix(S) for S in est])
    poses0 = np.stack(est).astype(np.float32)
    poses0[:, 3] = (0, 0, 0, 1)
    return truth, nodes0, edges, poses0, se3_edges


def centre_rms(nodes, truth):
    """RMS distance of the camera centres -R' t / s of srt nodes from the truth's"""
    c = []
    for v in nodes:
        s, R, t = parts(srt_to_matrix(v))
        c.append(-(R.T @ t) / s)
    ct = np.stack([-T[:3, :3].T @ T[:3, 3] for T in truth])
    return float(np.sqrt(((np.stack(c) - ct) ** 2).sum(1).mean()))


def rejecting_case():
    """A start and loops so inconsistent that LM rejects trials long before convergence: (nodes0, edges, nfixed, iters)"""
    nodes0, edges = chain_graph(seed=23, nnodes=6, chords=[(0, 5), (1, 4), (0, 3), (2, 5)], odo_noise=(2.0, 5.0, 0.7),
                                start_noise=(1.0, 3.0, 0.5))
    return nodes0, edges, 1, 6
