"""CPU test: the two solvers that have no reference fixture at all -- the multi-keyframe local BA (north-star extension,
SURVEY a17 / D1) and the optimum of LocalBA::PoseOptimization (LocalBA.cpp:291-490, g2o absent from the image) -- against an
INDEPENDENT library: scipy.optimize.least_squares on the same reprojection residuals must reach the same optimum as
oracle.local_ba / oracle.pose_opt run to convergence (cost within 1e-8 relative, poses within 1e-6).

This does not pin parity with g2o (still no reference vector: "parity unpinned"); it shows that the oracle the GPU kernels are
compared with minimises the function it claims to minimise. The problems are built so that every edge is an inlier at the
optimum (chi2 far below the Huber bound 5.991): g2o's Huber kernel acts on the 2-vector error of an edge, scipy's `loss`
on scalar residuals, so only the plain least-squares optimum is comparable; the last case has gross outliers and checks the
optimum over the edges the oracle kept, which is what its last two non-robust rounds minimise (LocalBA.cpp:426-443)."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import oracle
import ba_cases as bc
import gauge_cases as gc
from ba_cases import as_solver_pose as _as_solver_pose   # the solver's quaternion extraction, shared with robust_cost
from trackingbench_slam_amd import synth

K = (718.856, 718.856, 607.1928, 185.2157)


def _rodrigues(w):
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def _compose(xi, T0):
    """Tcw = [R(w) | t] * T0 -- any smooth chart works, the optimum is a point on SE(3)"""
    T = np.eye(4)
    T[:3, :3] = _rodrigues(xi[:3])
    T[:3, 3] = xi[3:6]
    return T @ T0


def _reproj(T, X, uv, w, K=K):
    pc = X @ T[:3, :3].T + T[:3, 3]
    proj = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
    return ((uv - proj) * np.sqrt(w)[:, None]).ravel()


def _solve(fun, x0):
    r = least_squares(fun, x0, jac="3-point", method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
    return r.x, 2.0 * r.cost


@pytest.mark.parametrize("seed,nkf,npt,nfixed", [(101, 4, 60, 2), (102, 6, 120, 2), (103, 5, 90, 1)])
def test_local_ba_optimum_matches_scipy(seed, nkf, npt, nfixed):
    _local_ba_vs_scipy(seed, nkf, npt, nfixed, None)


def test_local_ba_optimum_matches_scipy_gauged():
    """The first window in the y180 world gauge (tests/gauge_cases.py): every keyframe in the y branch of the quaternion
    extraction, in the oracle and in _as_solver_pose. The bounds are the ungauged test's."""
    _local_ba_vs_scipy(101, 4, 60, 2, "y180")


@pytest.mark.parametrize("seed,nkf,npt,nfixed", [(101, 4, 60, 2), (102, 6, 120, 2), (103, 5, 90, 1)])
def test_local_ba_optimum_matches_scipy_weighted_aniso(seed, nkf, npt, nfixed):
    """The same windows at fx != fy (ba_cases.K_ANISO) with octave weights 1.2^(-2o) drawn per observation: a weight on the
    wrong edge, applied twice or missing from the right-hand side, or an fx where fy belongs, moves the optimum away from
    scipy's. No outliers: the edge-wise Huber kernel has no scipy counterpart. The bounds are the unit-weight test's."""
    _local_ba_vs_scipy(seed, nkf, npt, nfixed, None, K=bc.K_ANISO, weighted=True)


def _local_ba_vs_scipy(seed, nkf, npt, nfixed, gname, K=K, weighted=False):
    Pt, Pi, Xt, Xi, obs = synth.ba_problem(seed, nkf, npt, K, obs_per_pt=4, noise_px=0.3, pose_noise=0.01, pt_noise=0.02)
    if weighted:
        obs["inv_sigma2"] = bc.octave_weights(np.random.default_rng(seed), len(obs))
        assert len(np.unique(obs["inv_sigma2"])) == 8
    if gname is not None:
        G = gc.get(gname)
        Pt, Pi, Xi = gc.gauge_poses(Pt, G), gc.gauge_poses(Pi, G), gc.gauge_points(Xi, G)
        assert all(gc.quat_branch(T) == gc.GAUGE_BRANCH[gname] for T in Pi)
    # a point seen by one keyframe has a free direction (its depth) and a residual that only vanishes in the limit: LM stops
    # a few 1e-7 of the cost short of it. Keep the points that two or more keyframes see, renumbered.
    cnt = np.bincount(obs["pt"], minlength=npt)
    keep = np.flatnonzero(cnt >= 2)
    remap = -np.ones(npt, np.int64); remap[keep] = np.arange(len(keep))
    obs = obs[cnt[obs["pt"]] >= 2].copy()
    obs["pt"] = remap[obs["pt"]]
    Xi, npt = Xi[keep], len(keep)
    if nfixed == 1:  # one fixed keyframe leaves the scale free: hold it through a second, exactly known pose instead
        Pi = Pi.copy(); Pi[1] = Pt[1]; nfixed_o = 2
    else:
        nfixed_o = nfixed
    it, Po, Xo, st = oracle.local_ba(K, Pi, nfixed_o, Xi, obs, 60)
    P0 = np.stack([_as_solver_pose(T) for T in Pi])
    X0 = Xi.astype(np.float64)
    kf, pt = obs["kf"], obs["pt"]
    uv = np.stack([obs["u"], obs["v"]], 1).astype(np.float64)
    w = obs["inv_sigma2"].astype(np.float64)
    nfree = nkf - nfixed_o

    def fun(x):
        T = [P0[k] if k < nfixed_o else _compose(x[6 * (k - nfixed_o):6 * (k - nfixed_o) + 6], P0[k]) for k in range(nkf)]
        X = X0 + x[6 * nfree:].reshape(-1, 3)
        r = np.empty(2 * len(obs))
        for k in range(nkf):
            m = kf == k
            r[np.repeat(m, 2)] = _reproj(T[k], X[pt[m]], uv[m], w[m], K)
        return r

    x, cost = _solve(fun, np.zeros(6 * nfree + 3 * npt))
    # every edge an inlier at the optimum, so the Huber sum the oracle reports IS the plain sum of squares
    r = fun(x).reshape(-1, 2)
    assert (r ** 2).sum(1).max() < 5.991
    assert abs(st[2] - cost) <= 1e-8 * cost, (st[2], cost)
    for k in range(nfixed_o, nkf):
        T = _compose(x[6 * (k - nfixed_o):6 * (k - nfixed_o) + 6], P0[k])
        assert np.abs(T - Po[k]).max() < 2e-6  # the oracle returns float32 poses
    seen = np.zeros(npt, bool); seen[pt] = True
    assert np.abs((X0 + x[6 * nfree:].reshape(-1, 3))[seen] - Xo[seen]).max() < 2e-5


# one gauge per quaternion branch. The bounds below are absolute on a float32 pose: gen2's 100 m translation alone rounds by up to
# 3.8e-6 there, so the "w" variant takes gen2's rotation with the small translation of the 180-degree gauges.
SCIPY_GAUGES = {"w": gc.gauge(gc.GAUGES["gen2"][:3, :3], (3, -2, 5)), "x": gc.GAUGES["x180"], "y": gc.GAUGES["y180"], "z": gc.GAUGES["z180"]}


@pytest.mark.parametrize("seed,n,outlier_frac", [(201, 120, 0.0), (202, 400, 0.0), (203, 300, 0.12)])
def test_pose_opt_optimum_matches_scipy(seed, n, outlier_frac):
    _pose_opt_vs_scipy(seed, n, outlier_frac, None)


@pytest.mark.parametrize("branch,seed,n,outlier_frac", [("w", 201, 120, 0.0), ("x", 202, 400, 0.0), ("y", 203, 300, 0.12), ("z", 201, 120, 0.0)])
def test_pose_opt_optimum_matches_scipy_gauged(branch, seed, n, outlier_frac):
    """The same problems in a world gauge that puts the start pose AND the optimum in the named branch of the quaternion
    extraction (the oracle's, and _as_solver_pose's). The bounds are the ungauged test's."""
    _pose_opt_vs_scipy(seed, n, outlier_frac, branch)


def _pose_opt_vs_scipy(seed, n, outlier_frac, branch):
    Tt, Ti, obs = synth.pose_problem(seed, n, K, noise_px=0.3, outlier_frac=outlier_frac)
    if branch is not None:
        Ti, obs = gc.gauge_pose_problem(Ti, obs, SCIPY_GAUGES[branch])
        assert gc.quat_branch(Ti) == branch
    ninl, To, outl, st = oracle.pose_opt(K, Ti, obs)
    assert branch is None or gc.quat_branch(To) == branch
    keep = outl == 0
    assert ninl == keep.sum() and (outlier_frac > 0) == (not keep.all())
    X = np.stack([obs["X"], obs["Y"], obs["Z"]], 1).astype(np.float64)[keep]
    uv = np.stack([obs["u"], obs["v"]], 1).astype(np.float64)[keep]
    w = obs["inv_sigma2"].astype(np.float64)[keep]
    T0 = _as_solver_pose(To)  # start at the oracle's answer: scipy must not move away from it ...
    x, cost = _solve(lambda x: _reproj(_compose(x, T0), X, uv, w), np.zeros(6))
    assert np.abs(_compose(x, T0) - To).max() < 2e-6
    # ... and from the initial pose it must arrive there as well (the optimum over the kept edges, not a local artefact)
    T1 = _as_solver_pose(Ti)
    x2, cost2 = _solve(lambda x: _reproj(_compose(x, T1), X, uv, w), np.zeros(6))
    assert np.abs(_compose(x2, T1) - To).max() < 2e-6
    assert abs(cost2 - cost) <= 1e-8 * cost
    c_or = (_reproj(T0, X, uv, w) ** 2).sum()
    assert abs(c_or - cost) <= 1e-6 * cost  # the float32 pose the oracle returns costs the same to first order
    if outlier_frac == 0:  # stats[1]: the chi2 the solver ended its last round with, all edges active
        assert abs(st[1] - cost) <= 1e-8 * cost, (st[1], cost)
