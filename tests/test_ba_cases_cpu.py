"""CPU: the conditions that make tests/test_gpu_ba_weights.py mean something, established on the oracle alone.

Every window of tests/ba_cases.py runs at K_ANISO with per-edge weights. Here, without a GPU: the outlier windows really have
edges on Huber's linear branch at the result, a weight on the wrong edge moves the oracle by far more than the GPU bar, weight 0
is the same as no row, a point behind the cameras leaves the result finite, the far start contains rejected steps, and the
objective the oracle reports is the one robust_cost() computes from the definition."""
import numpy as np
import pytest

import oracle
import ba_cases as bc

K = bc.K_ANISO
WEIGHTED = [n for n in bc.case_names() if n != "unit5"]     # unit5 is the batch's unit-weight control: rolling 1.0s changes nothing


def test_k_is_anisotropic():
    assert K[0] != K[1] and K == (718.856, 652.25, 607.1928, 185.2157)
    assert abs(np.log2(K[1] / K[0]) - round(np.log2(K[1] / K[0]))) > 0.1          # no power-of-two ratio


def test_weights_are_octaves():
    """1.2^(-2o) in float32, all eight levels present, independent of keyframe and point (every keyframe sees several levels)"""
    Pi, Xi, obs, nfixed, iters = bc.case("mfma5-octaves")
    lv = np.unique(obs["inv_sigma2"])
    assert len(lv) == 8 and lv.max() == 1.0 and np.isclose(lv.min(), 1.2 ** -14, rtol=1e-6)
    for k in range(5):
        assert len(np.unique(obs["inv_sigma2"][obs["kf"] == k])) >= 6


@pytest.mark.parametrize("name", [n for n in bc.case_names() if "outliers" in n or n.startswith("tile") or n == "far"])
def test_active_huber_edges(name):
    """at the oracle's result at least 5 % of the edges have c > 5.991: the linear branch of rho, its weight delta / sqrt(c) in
    the blocks and the right-hand side, are in use"""
    Pi, Xi, obs, nfixed, iters = bc.case(name)
    io, Po, Xo, so = bc.case_oracle(name)
    c = bc.edge_chi2(K, Po, Xo, obs)
    assert (c > 5.991).mean() >= 0.05, (c > 5.991).mean()


def test_outliers_leave_points_determined():
    """at most one displaced row per point, only on points that three or more keyframes see"""
    kind, seed, nkf, npt, nfixed, per, iters = bc.CASES["mfma5-outliers"]
    _, _, clean = bc.window("octaves", seed, nkf, npt, nfixed, per)
    _, _, obs = bc.window("outliers", seed, nkf, npt, nfixed, per)
    assert np.array_equal(clean["inv_sigma2"], obs["inv_sigma2"])
    moved = (clean["u"] != obs["u"]) | (clean["v"] != obs["v"])
    deg = np.bincount(obs["pt"], minlength=npt)
    per_pt = np.bincount(obs["pt"][moved], minlength=npt)
    assert per_pt.max() == 1 and deg[per_pt > 0].min() >= 3
    assert per_pt.sum() == int(round(0.3 * (deg >= 3).sum()))
    d = np.abs(np.stack([obs["u"] - clean["u"], obs["v"] - clean["v"]], 1)[moved])
    assert d.min() > 9.99 and d.max() < 40.01


@pytest.mark.parametrize("name", WEIGHTED)
def test_rolled_weights_move_the_oracle(name):
    """every weight moved on by one edge: the oracle's poses change by at least 100 times the GPU bar (1e-6 times the largest
    pose entry). Measured: 3.7e-4 (plain8200-octaves, bar x 100 = 1e-4) to 0.32 (far)."""
    Pi, Xi, obs, nfixed, iters = bc.case(name)
    io, Po, Xo, so = bc.case_oracle(name)
    ir, Pr, Xr, sr = oracle.local_ba(K, Pi, nfixed, Xi, bc.rolled(obs), iters)
    bar = 1e-6 * max(1.0, float(np.abs(Po).max()))
    assert np.abs(Pr - Po).max() >= 100 * bar, (float(np.abs(Pr - Po).max()), bar)


@pytest.mark.parametrize("name", [n for n in bc.case_names() if "zero" in n])
def test_zero_weight_is_no_row(name):
    """weight 0 adds exact zeros to every sum: the oracle's result equals, bit for bit, the result on the window with those
    rows deleted; a free keyframe whose rows are all silenced keeps its pose (to the quaternion round trip: 1e-6)"""
    Pi, Xi, obs, nfixed, iters = bc.case(name)
    io, Po, Xo, so = bc.case_oracle(name)
    o2 = bc.without_zero_rows(obs)
    assert 0 < len(o2) < len(obs)
    i2, P2, X2, s2 = oracle.local_ba(K, Pi, nfixed, Xi, o2, iters)
    assert io == i2 and np.array_equal(Po, P2) and np.array_equal(Xo, X2) and np.array_equal(so, s2)
    if "zero_kf" in name:
        assert not (o2["kf"] == nfixed).any()
        assert np.abs(Po[nfixed] - Pi[nfixed]).max() < 1e-6
        assert np.abs(Po[nfixed + 1] - Pi[nfixed + 1]).max() > 1e-4               # ... while the others move


def test_behind_is_finite():
    Pi, Xi, obs, nfixed, iters = bc.case("mfma5-behind")
    p = bc.behind_point(obs)
    T = np.stack([bc.as_solver_pose(P) for P in Pi])
    for k in obs["kf"][obs["pt"] == p]:
        assert (T[k, :3, :3] @ Xi[p].astype(np.float64) + T[k, :3, 3])[2] < 0, "the start value is behind camera %d" % k
    io, Po, Xo, so = bc.case_oracle("mfma5-behind")
    assert np.isfinite(Po).all() and np.isfinite(Xo).all() and np.isfinite(so).all()


def test_far_contains_rejected_steps():
    io, Po, Xo, so = bc.case_oracle("far")
    assert so[4] > io, "the case is meant to contain rejected steps"


def test_kf_pass_window_crosses_a_chunk():
    Pi, Xi, obs, nfixed, iters = bc.case("kfpass")
    per_kf = np.bincount(obs["kf"], minlength=4)
    assert len(Pi) == 4 and nfixed == 2 and per_kf[2] == 600 > 512 and len(Xi) == 600


@pytest.mark.parametrize("name", bc.case_names())
def test_robust_cost_is_the_oracles_objective(name):
    """robust_cost at the start state equals stats[1] (measured: at most 6.3e-15 relative; bound 1e-9, the bar the GPU tests hold
    stats[1] to); at the returned float32 state it equals stats[2] (measured: 1e-9 to 2.5e-7, limited by the float32 output;
    bound 1e-6)."""
    Pi, Xi, obs, nfixed, iters = bc.case(name)
    io, Po, Xo, so = bc.case_oracle(name)
    assert abs(bc.robust_cost(K, Pi, Xi, obs) - so[1]) <= 1e-9 * so[1]
    assert abs(bc.robust_cost(K, Po, Xo, obs) - so[2]) <= 1e-6 * so[2]


def test_exchanged_focal_lengths_move_the_oracle():
    """fx and fy exchanged: the oracle's poses move by at least 100 times the GPU bar on a window of every path
    (measured: 1.0e-2 to 4.3e-2)"""
    Kx = (K[1], K[0], K[2], K[3])
    for name in ("mfma5-octaves", "mfma12-octaves", "large13-octaves", "kfpass"):
        Pi, Xi, obs, nfixed, iters = bc.case(name)
        io, Po, Xo, so = bc.case_oracle(name)
        ix, Px, Xx, sx = oracle.local_ba(Kx, Pi, nfixed, Xi, obs, iters)
        assert np.abs(Px - Po).max() >= 100 * 1e-6 * max(1.0, float(np.abs(Po).max())), name
