"""The batched SE(3) pose-graph optimiser in numpy float64, from its definitions: the yardstick of tb_pose_graph_batch_dev.

A graph has `nnodes` camera poses Tcw, the first `nfixed` held, and edges (a, b, Z, w_rot, w_trans) that measure the motion
Z ~ T_b T_a^-1. With E = Z^-1 T_b T_a^-1 the residual is r = Log(E), ordered (omega, upsilon) like the update vector of every
solver here (T <- exp(delta) T, SE3Quat::exp), and the cost is chi2 = sum r' diag(w_rot I3, w_trans I3) r. The Jacobians are the
exact derivatives with respect to those left perturbations,

    J_b = Jl^-1(r) Ad(Z^-1),        J_a = -Jl^-1(r) Ad(E),        Ad(T) = [[R, 0], [[t]x R, R]],

Jl^-1 the inverse left Jacobian of SE(3) in closed form (Barfoot, State Estimation for Robotics, 7.85 / 7.86 reordered), every
coefficient that cancels taking its series below SMALL. The normal equations are assembled edge by edge in list order, solved
by a dense Cholesky factorisation, and stepped by g2o's Levenberg-Marquardt rule as the local BA restates it: lambda0 = 1e-5 max
diag H; a trial is accepted when rho > 0 and its chi2 is finite, then lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2;
otherwise lambda *= nu, nu *= 2; at most 10 trials per iteration; stop at 10 rejections, at rho == 0, or after `iters`.

Poses come in as float32 [R | t] and enter through the quaternion extraction and normalisation of po_from_Rt; they leave as
float32. A graph that is malformed, has no edge, or accepted no step keeps every byte of its poses, and fixed nodes always do.
"""
import numpy as np

SMALL = 0.1   # rotation angle below which the cancelling coefficients take their series (three terms: error below 2e-11 relative)
EDGE = np.dtype([("a", "<i4"), ("b", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("w_rot", "<f8"), ("w_trans", "<f8")])
MAX_NODES, MAX_EDGES = 64, 256


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def quat_from_R(R):
    """Eigen's Quaternion(Matrix3) as po_quat_from_R restates it, then po_normalize: (x, y, z, w), w >= 0, unit"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    if q[3] < 0:
        q = -q
    return q / np.sqrt((q * q).sum())


def R_from_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_in(T32):
    """a float32 pose as the solver takes it: 4x4 float64 whose rotation went through the unit quaternion"""
    T = np.asarray(T32, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = R_from_quat(quat_from_R(T[:3, :3]))
    out[:3, 3] = T[:3, 3]
    return out


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def exp(u):
    """SE3Quat::exp as po_exp_mul has it: u = (omega, upsilon) -> [R | V upsilon]"""
    u = np.asarray(u, np.float64)
    th = np.sqrt((u[:3] ** 2).sum())
    Om = hat(u[:3])
    Om2 = Om @ Om
    if th < 0.00001:
        a, b, d = 1.0, 0.5, 1.0 / 6.0
    else:
        a, b, d = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Om + b * Om2
    T[:3, 3] = (np.eye(3) + b * Om + d * Om2) @ u[3:]
    return T


def _so3_inv_coeff(th):
    """k of Jl^-1 = V^-1 = I - Omega / 2 + k Omega^2"""
    if th < SMALL:
        t2 = th * th
        return 1.0 / 12 + t2 / 720 + t2 * t2 / 30240
    h = 0.5 * th
    return (1.0 - h * np.cos(h) / np.sin(h)) / (th * th)


def log(T):
    """(omega, upsilon) with exp(log(T)) = T, the angle in [0, pi]: omega from the unit quaternion of R"""
    q = quat_from_R(T[:3, :3])
    n = np.sqrt((q[:3] ** 2).sum())
    th = 2.0 * np.arctan2(n, q[3])
    om = q[:3] * (2.0 / q[3]) if th < 0.00001 else q[:3] * (th / n)
    Om = hat(om)
    Vinv = np.eye(3) - 0.5 * Om + _so3_inv_coeff(th) * (Om @ Om)
    return np.concatenate([om, Vinv @ T[:3, 3]])


def adjoint(T):
    R = T[:3, :3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(T[:3, 3]) @ R
    return A


def jl_inv(r):
    """inverse left Jacobian of SE(3) at r = (omega, upsilon): [[J^-1, 0], [-J^-1 Q J^-1, J^-1]]"""
    th = np.sqrt((r[:3] ** 2).sum())
    Om, Up = hat(r[:3]), hat(r[3:])
    if th < SMALL:
        t2 = th * th
        c1 = 1.0 / 6 - t2 / 120 + t2 * t2 / 5040
        c2 = 1.0 / 24 - t2 / 720 + t2 * t2 / 40320
        c3 = 1.0 / 120 - t2 / 2520 + t2 * t2 / 120960
    else:
        s, c = np.sin(th), np.cos(th)
        c1 = (th - s) / th ** 3
        c2 = (th * th + 2 * c - 2) / (2 * th ** 4)
        c3 = (2 * th - 3 * s + th * c) / (2 * th ** 5)
    OU, UO = Om @ Up, Up @ Om
    OUO = OU @ Om
    Q = 0.5 * Up + c1 * (OU + UO + OUO) + c2 * (Om @ OU + UO @ Om - 3 * OUO) + c3 * (OUO @ Om + Om @ OUO)
    Ji = np.eye(3) - 0.5 * Om + _so3_inv_coeff(th) * (Om @ Om)
    J = np.zeros((6, 6))
    J[:3, :3] = Ji
    J[3:, 3:] = Ji
    J[3:, :3] = -Ji @ Q @ Ji
    return J


def edge_Z(e):
    """the measured motion of an edge record as a 4x4, its quaternion normalised as the kernel normalises it"""
    q = np.asarray(e["q"], np.float64)
    if q[3] < 0:
        q = -q
    q = q / np.sqrt((q * q).sum())
    Z = np.eye(4)
    Z[:3, :3] = R_from_quat(q)
    Z[:3, 3] = e["t"]
    return Z


def make_edge(a, b, Z, w_rot=1.0, w_trans=1.0):
    e = np.zeros((), EDGE)
    e["a"], e["b"], e["w_rot"], e["w_trans"] = a, b, w_rot, w_trans
    e["q"] = quat_from_R(np.asarray(Z, np.float64)[:3, :3])
    e["t"] = np.asarray(Z, np.float64)[:3, 3]
    return e


def edge_between(a, b, Ta32, Tb32, w_rot=1.0, w_trans=1.0):
    """the edge two stored float32 poses imply: its residual on those poses is of rounding size"""
    return make_edge(a, b, pose_in(Tb32) @ inv(pose_in(Ta32)), w_rot, w_trans)


def residual(Z, Ta, Tb):
    return log(inv(Z) @ Tb @ inv(Ta))


def jacobians(Z, Ta, Tb):
    """(r, J_a, J_b)"""
    Zi = inv(Z)
    E = Zi @ Tb @ inv(Ta)
    r = log(E)
    Ji = jl_inv(r)
    return r, -Ji @ adjoint(E), Ji @ adjoint(Zi)


def malformed(nnodes, edges):
    for e in edges:
        a, b = int(e["a"]), int(e["b"])
        if a < 0 or a >= nnodes or b < 0 or b >= nnodes or a == b:
            return True
        v = np.concatenate([e["q"], e["t"], [e["w_rot"], e["w_trans"]]])
        if not np.all(np.isfinite(v)) or e["w_rot"] < 0 or e["w_trans"] < 0:
            return True
        n2 = float((np.asarray(e["q"]) ** 2).sum())
        if not (n2 > 0 and np.isfinite(n2)):
            return True
    return False


def chi2_of(T, edges, Zs):
    c = 0.0
    for e, Z in zip(edges, Zs):
        r = residual(Z, T[e["a"]], T[e["b"]])
        c += e["w_rot"] * (r[:3] ** 2).sum() + e["w_trans"] * (r[3:] ** 2).sum()
    return c


def cholesky_solve(A, b):
    """un-pivoted dense Cholesky; None where a pivot is not positive and finite"""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not (d > 0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve(poses, nfixed, edges, iters=10, trace=None):
    """One graph. poses float32 [nnodes, 4, 4] (or [nnodes, 16]); edges an EDGE array. Returns (poses float32 [nnodes, 4, 4],
    stats [8]): iterations, initial chi2, final chi2, final lambda, trials; stats[7] = -1 flags a malformed graph.
    trace (a list) receives (iteration, trial, rho, accepted, chi2 before, chi2 of the trial) of every trial."""
    P32 = np.ascontiguousarray(poses, np.float32).reshape(-1, 4, 4)
    n = len(P32)
    assert 1 <= nfixed < n <= MAX_NODES and len(edges) <= MAX_EDGES and iters >= 0
    stats = np.zeros(8)
    out = P32.copy()
    if malformed(n, edges):
        stats[7] = -1
        return out, stats
    if len(edges) == 0:
        return out, stats
    T = [pose_in(p) for p in P32]
    Zs = [edge_Z(e) for e in edges]
    nfree = n - nfixed
    N = 6 * nfree
    cur = chi2_of(T, edges, Zs)
    stats[1] = stats[2] = cur
    lam, nu, done, trials, accepted_any, ok = 0.0, 2.0, 0, 0, False, True
    for it in range(iters):
        if not ok:
            break
        H, g = np.zeros((N, N)), np.zeros(N)
        for e, Z in zip(edges, Zs):
            a, b = int(e["a"]), int(e["b"])
            r, Ja, Jb = jacobians(Z, T[a], T[b])
            W = np.array([e["w_rot"]] * 3 + [e["w_trans"]] * 3)
            for (i, Ji) in ((a, Ja), (b, Jb)):
                if i < nfixed:
                    continue
                oi = 6 * (i - nfixed)
                H[oi:oi + 6, oi:oi + 6] += Ji.T @ (W[:, None] * Ji)
                g[oi:oi + 6] -= Ji.T @ (W * r)
            if a >= nfixed and b >= nfixed:
                oa, ob = 6 * (a - nfixed), 6 * (b - nfixed)
                blk = Ja.T @ (W[:, None] * Jb)
                H[oa:oa + 6, ob:ob + 6] += blk
                H[ob:ob + 6, oa:oa + 6] += blk.T
        if it == 0:
            lam, nu = 1e-5 * np.abs(np.diag(H)).max(), 2.0
        rho, q = 0.0, 0
        while True:
            x = cholesky_solve(H + lam * np.eye(N), g)
            solved = x is not None
            if not solved:
                x = np.zeros(N)
            Tn = list(T)
            for k in range(nfixed, n):
                Tn[k] = exp(x[6 * (k - nfixed):6 * (k - nfixed) + 6]) @ T[k]
            trial = chi2_of(Tn, edges, Zs) if solved else np.finfo(np.float64).max
            rho = (cur - trial) / (float(x @ (lam * x + g)) + 1e-3)
            acc = bool(rho > 0 and np.isfinite(trial))
            if trace is not None:
                trace.append((it, q, rho, acc, cur, trial))
            if acc:
                lam *= max(1.0 / 3, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3))
                nu = 2.0
                cur, T, accepted_any = trial, Tn, True
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
            out[k] = T[k].astype(np.float32)
            out[k, 3] = (0, 0, 0, 1)
    stats[0], stats[2], stats[3], stats[4] = done, cur, lam, trials
    return out, stats


def solve_batch(poses, nfixed, edges, counts, iters=10):
    """poses [G, nnodes, 16 | 4, 4] float32, edges [G, pitch] EDGE, counts [G] (a count above the pitch flags its graph)"""
    poses = np.ascontiguousarray(poses, np.float32)
    G = len(poses)
    out = poses.reshape(G, -1, 4, 4).copy()
    stats = np.zeros((G, 8))
    for g in range(G):
        if counts[g] > edges.shape[1] or counts[g] < 0:
            stats[g, 7] = -1
            continue
        out[g], stats[g] = solve(poses[g], nfixed, edges[g, :counts[g]], iters)
    return out, stats


# ---------------------------------------------------------------- shared cases (CPU and GPU tests)
def random_pose(rng, rot=0.3, trans=2.0):
    return exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))


def chain_graph(seed, nnodes, chords, odo_noise=(0.01, 0.02), start_noise=(0.02, 0.05), w=(1.0, 1.0), G=None, reverse=()):
    """A chain of `nnodes` cameras with noisy odometry edges and exact-plus-noise chords [(a, b), ...] (repeats and a > b
    allowed), started off the truth. G (4x4): the world gauge, Tcw' = Tcw G^-1. reverse: indices of edges listed as (b, a).
    Returns (poses0 float32 [nnodes, 4, 4], edges)."""
    rng = np.random.default_rng(seed)
    truth = [np.eye(4)]
    for i in range(1, nnodes):
        step = exp(np.concatenate([rng.normal(0, 0.05, 3), np.array([0.0, 0.0, -0.5]) + rng.normal(0, 0.05, 3)]))
        truth.append(step @ truth[-1])
    if G is not None:
        truth = [T @ inv(G) for T in truth]

    def noisy(T, s):
        return exp(np.concatenate([rng.normal(0, s[0], 3), rng.normal(0, s[1], 3)])) @ T

    pairs = [(i, i + 1) for i in range(nnodes - 1)] + list(chords)
    edges = np.zeros(len(pairs), EDGE)
    for k, (a, b) in enumerate(pairs):
        if k in reverse:
            a, b = b, a
        edges[k] = make_edge(a, b, noisy(truth[b] @ inv(truth[a]), odo_noise), w[0], w[1])
    poses0 = np.stack([(truth[i] if i == 0 else noisy(truth[i], start_noise)).astype(np.float32) for i in range(nnodes)])
    poses0[:, 3] = (0, 0, 0, 1)
    return poses0, edges


def circuit(seed, N, radius=10.0, noise=(0.01, 0.02)):
    """The drift case: N cameras on a circle, yaw = arc angle; odometry edges carry noise exp((N(0, noise[0])^3, N(0,
    noise[1])^3)) and are integrated from node 0; one exact loop edge (0, N - 1).
    Returns (truth [N, 4, 4] float64 Tcw, poses0 float32, edges)."""
    rng = np.random.default_rng(seed)
    truth = []
    for i in range(N):
        ang = 2 * np.pi * i / N
        Twc = np.eye(4)
        Twc[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        Twc[:3, 3] = (radius * np.sin(ang), 0.0, radius * (1 - np.cos(ang)))
        truth.append(inv(Twc))
    edges = np.zeros(N, EDGE)
    est = [truth[0]]
    for i in range(N - 1):
        Z = exp(np.concatenate([rng.normal(0, noise[0], 3), rng.normal(0, noise[1], 3)])) @ truth[i + 1] @ inv(truth[i])
        edges[i] = make_edge(i, i + 1, Z)
        est.append(Z @ est[-1])
    edges[N - 1] = make_edge(0, N - 1, truth[N - 1] @ inv(truth[0]))
    poses0 = np.stack(est).astype(np.float32)
    poses0[:, 3] = (0, 0, 0, 1)
    return np.stack(truth), poses0, edges


def centre_rms(poses, truth):
    c = np.stack([-np.asarray(T, np.float64)[:3, :3].T @ np.asarray(T, np.float64)[:3, 3] for T in poses])
    ct = np.stack([-T[:3, :3].T @ T[:3, 3] for T in truth])
    return float(np.sqrt(((c - ct) ** 2).sum(1).mean()))


def rejecting_case():
    """A start and loops so inconsistent (chords off by radians and metres) that LM rejects trials long before convergence:
    (poses0, edges, nfixed, iters). In the six iterations every |rho| is above 0.1, so no rounding decides a trial."""
    poses0, edges = chain_graph(seed=23, nnodes=6, chords=[(0, 5), (1, 4), (0, 3), (2, 5)], odo_noise=(2.0, 5.0), start_noise=(1.0, 3.0))
    return poses0, edges, 1, 6
