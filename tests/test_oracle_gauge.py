"""CPU tests: the oracle's pose optimisation and local BA under world gauges (tests/gauge_cases.py), away from the identity pose.

Equivariance. A gauge changes no residual, so the oracle must return the same flags and inlier counts, the ungauged pose times
G^-1 and the ungauged points times G. What is left is the float32 re-rounding of the transformed inputs (and of the output pose
at its new magnitude). Measured on the oracle itself, defect = max |gauged result - transformed ungauged result| relative to the
largest entry of the gauged result, over the eight gauges of the table:

    oracle.pose_opt    seeds 1, 3, 4, 6, 7, 8 (n = 300, 50, 9, 700, 10, 257), with and without pre-set flags:
                       poses 3.93e-7, flags and inlier counts identical               -> bound 4 x = 1.6e-6
    oracle.local_ba    windows "mfma" (seed 1, 5 kf, 200 pts) and "large" (seed 31, 13 kf, 300 pts, 11 free):
                       poses 2.30e-7 (gen2, the 100 m translation)                    -> bound 4 x = 9.2e-7
                       points 2.76e-6 (mfma under gen2; y175 1.86e-6, x170 1.67e-6)   -> bound 4 x = 1.1e-5
                       iterations and LM trials identical; final chi2 within 3.5e-6 relative
                       window "far" (seed 50, rejected steps): poses 8.3e-8, points 2.1e-7, 8 iterations / 15 trials in every gauge

The factor 4: the defect is input rounding and moves by a small factor from gauge to gauge; a wrong branch of the quaternion
extraction gives errors of order 1, so any margin far below 1e-2 discriminates.

Order probe. The GPU sums the edges in another order than the oracle. Every pose case of the shared table must therefore be
one the oracle itself resolves independently of the order: under a permutation of the edges (pre-set flags permuted along) the
same flags and a pose that moves by at most 1e-7 max(1, |T|). Measured: 0.0 on all 99 cases. A case that fails is ill-conditioned
and gets replaced, not loosened (twelve coincident points move the oracle by 1.65e-6: not in the table).
"""
import numpy as np
import pytest

import oracle
import gauge_cases as gc

K = gc.K
POSE_BOUND = 4 * 3.93e-7
BA_POSE_BOUND = 4 * 2.30e-7
BA_POINT_BOUND = 4 * 2.76e-6


def _rel(got, exp):
    return float(np.abs(got - exp).max() / np.abs(got).max())


@pytest.mark.parametrize("seed,n,frac", gc.EQUIVARIANCE_PROBLEMS)
def test_pose_opt_equivariance(seed, n, frac):
    _, Ti, obs = gc.problem(seed, n, frac)
    seen = set()
    for pre in (None, (np.arange(n) % 7 == 0).astype(np.uint8)):
        n0, T0, o0, _ = oracle.pose_opt(K, Ti, obs, pre)
        for g, G in gc.GAUGES.items():
            Tg, og = gc.gauge_pose_problem(Ti, obs, G)
            want = "x" if g == "perm120" else gc.GAUGE_BRANCH[g]     # Ti is the exact identity: the tie resolves to "x"
            assert gc.quat_branch(Tg) == want, g
            seen.add(want)
            n1, T1, o1, _ = oracle.pose_opt(K, Tg, og, pre)
            assert n1 == n0 and np.array_equal(o1, o0), g
            d = _rel(T1, T0.astype(np.float64) @ gc.inv(G))
            assert d <= POSE_BOUND, (g, d)
    assert seen == set("wxyz")


@pytest.mark.parametrize("name", ["mfma", "large", "far"])
def test_local_ba_equivariance(name):
    Pi, Xi, obs, nfixed, iters = gc.ba_window(name)
    assert name != "large" or len(Pi) - nfixed >= 11
    i0, P0, X0, s0 = oracle.local_ba(K, Pi, nfixed, Xi, obs, iters)
    if name == "far":
        assert s0[4] > i0, "the window is meant to contain rejected steps"
    seen = set()
    for g, G in gc.GAUGES.items():
        Pg, Xg = gc.gauge_ba(Pi, Xi, G)
        if name != "far" or g == gc.BA_FAR_GAUGE:                    # the far window's own pose noise is 0.6 rad: pinned at its GPU gauge only
            seen.add(gc.assert_ba_branch(Pg, nfixed, g))
        i1, P1, X1, s1 = oracle.local_ba(K, Pg, nfixed, Xg, obs, iters)
        assert i1 == i0 and s1[4] == s0[4], g                        # the same iterations and LM trials: the same trajectory
        dp = _rel(P1, P0.astype(np.float64) @ gc.inv(G))
        dx = _rel(X1, X0.astype(np.float64) @ G[:3, :3].T + G[:3, 3])
        assert dp <= BA_POSE_BOUND and dx <= BA_POINT_BOUND, (g, dp, dx)
    assert seen - {None} == (set("wxyz") if name != "far" else {gc.GAUGE_BRANCH[gc.BA_FAR_GAUGE]})


def test_pose_case_table_reaches_every_branch():
    """Every case of the shared table sits in the branch the table claims, and together they reach all four."""
    seen = set()
    for c in gc.pose_cases().values():
        assert c.branch is not None and gc.quat_branch(c.Tin) == c.branch, c
        seen.add(c.branch)
    assert seen == set("wxyz")
    for prefix in ("gauged-", "size-", "far-", "batch-"):            # and so does every family but the one-gauge allpre
        assert len({c.branch for c in gc.cases(prefix)}) >= 2, prefix
    assert {c.branch for c in gc.cases("gauged-")} == set("wxyz") == {c.branch for c in gc.cases("batch-")}


def test_pose_case_table_order_probe():
    rng = np.random.default_rng(123)
    for c in gc.pose_cases().values():
        n0, T0, o0, _ = oracle.pose_opt(K, c.Tin, c.obs, c.pre)
        perm = rng.permutation(len(c.obs))
        n1, T1, o1, _ = oracle.pose_opt(K, c.Tin, c.obs[perm], None if c.pre is None else c.pre[perm])
        assert n1 == n0 and np.array_equal(o1, o0[perm]), c
        assert float(np.abs(T1 - T0).max()) <= 1e-7 * max(1.0, float(np.abs(T0).max())), c


def test_far_lost_and_preset_outcomes():
    """What the far, lost and pre-set cases are in the table for, pinned on the oracle: the (0.6, 2.0) start converges to the identity start's pose
    bit for bit, the other two are lost in round one (every edge an outlier, no active edge afterwards: the input pose comes back
    through the quaternion round trip); all flags pre-set still gives 262 inliers."""
    Tt, Ti, obs = gc.problem(11, 300, 0.1)
    n0, T0, o0, s0 = oracle.pose_opt(K, Ti, obs)
    far = {c.name: c for c in gc.cases("far-")}
    n1, T1, o1, s1 = oracle.pose_opt(K, far["far-0.6-id"].Tin, obs)
    assert n1 == n0 == 262 and np.array_equal(o1, o0) and np.array_equal(T1, T0) and s1[0] > s0[0]
    for c in gc.cases("far-"):
        if "0.6" in c.name:
            continue
        n, T, o, s = oracle.pose_opt(K, c.Tin, c.obs)
        assert n == 0 and o.all() and s[0] == 10, c
        assert np.allclose(T, c.Tin, rtol=0, atol=2e-7 * max(1.0, float(np.abs(c.Tin).max()))), c
    X = np.stack([obs["X"], obs["Y"], obs["Z"]], 1).astype(np.float64)
    T15 = far["far-1.5-id"].Tin.astype(np.float64)
    assert int(((X @ T15[:3, :3].T + T15[:3, 3])[:, 2] < 0).sum()) == 11     # points behind the camera at the furthest start
    for c in gc.cases("allpre-"):
        n, T, o, _ = oracle.pose_opt(K, c.Tin, c.obs, c.pre)
        assert n == 262 and np.array_equal(o, o0), c
