"""CPU tests of tests/pose_graph_reference.py, the numpy yardstick of tb_pose_graph_batch_dev: its Jacobians against central
differences, Log against Exp, a consistent graph, its optimum against scipy.optimize.least_squares, a start that makes LM
reject, and the drift case the operator exists for."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import gauge_cases as gc
import pose_graph_reference as pg


@pytest.mark.parametrize("norm", [0.1, 1.0])
def test_jacobians_match_central_differences(norm):
    rng = np.random.default_rng(11)
    for _ in range(4):
        Ta, Tb = pg.random_pose(rng, 1.0), pg.random_pose(rng, 1.0)
        u = rng.normal(0, 1, 6)
        u *= norm / np.linalg.norm(u)
        Z = pg.inv(pg.exp(u) @ pg.inv(Tb @ pg.inv(Ta)))      # E = exp(u)
        r, Ja, Jb = pg.jacobians(Z, Ta, Tb)
        assert abs(np.linalg.norm(r) - norm) < 1e-9
        h = 1e-6
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            na = (pg.residual(Z, pg.exp(d) @ Ta, Tb) - pg.residual(Z, pg.exp(-d) @ Ta, Tb)) / (2 * h)
            nb = (pg.residual(Z, Ta, pg.exp(d) @ Tb) - pg.residual(Z, Ta, pg.exp(-d) @ Tb)) / (2 * h)
            assert np.abs(na - Ja[:, k]).max() < 1e-6 and np.abs(nb - Jb[:, k]).max() < 1e-6


@pytest.mark.parametrize("angle", [0.0, 3e-6, 0.5 * pg.SMALL, 0.999 * pg.SMALL, 1.001 * pg.SMALL, 1.0, 3.0])
def test_log_inverts_exp_on_both_sides_of_the_small_angle_switches(angle):
    """3e-6 is below Exp's and Log's own switch (1e-5), the others straddle SMALL"""
    rng = np.random.default_rng(3)
    w = rng.normal(0, 1, 3)
    u = np.concatenate([w * (angle / np.linalg.norm(w)), rng.normal(0, 2, 3)])
    assert np.abs(pg.log(pg.exp(u)) - u).max() < 1e-12
    # the two branches of every coefficient agree at the switch
    if angle > 0:
        r = u.copy()
        J = pg.jl_inv(r)
        r2 = r.copy()
        r2[:3] *= (1 + 1e-9)
        assert np.abs(pg.jl_inv(r2) - J).max() < 1e-8


def test_consistent_graph_does_not_move():
    rng = np.random.default_rng(5)
    poses = np.stack([pg.random_pose(rng, 0.5, 3.0) for _ in range(6)]).astype(np.float32)
    poses[:, 3] = (0, 0, 0, 1)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (4, 1)]
    edges = np.array([pg.edge_between(a, b, poses[a], poses[b]) for a, b in pairs])
    out, st = pg.solve(poses, 1, edges, 10)
    assert st[1] < 1e-25 and st[2] <= st[1]       # rounding of float64 on residuals of order 1e-16
    assert np.abs(out - poses).max() < 1e-6 and np.array_equal(out[0], poses[0])


def _compose(xi, T0):
    T = np.eye(4)
    T[:3, :3] = gc.rodrigues(xi[:3])
    T[:3, 3] = xi[3:6]
    return T @ T0


SCIPY_GAUGES = {None: None, "w": gc.gauge(gc.GAUGES["gen2"][:3, :3], (3, -2, 5)), "x": gc.GAUGES["x180"], "y": gc.GAUGES["y180"],
                "z": gc.GAUGES["z180"]}


@pytest.mark.parametrize("seed,nnodes,chords,nfixed,branch", [
    (31, 6, [(0, 5)], 1, None), (32, 12, [(0, 11), (3, 9)], 1, None), (33, 20, [(0, 19), (4, 15), (16, 2)], 2, None),
    (34, 6, [(0, 5), (1, 4)], 1, "w"), (35, 6, [(0, 5)], 1, "x"), (36, 6, [(0, 5), (2, 5)], 1, "y"), (37, 6, [(0, 5)], 1, "z")])
def test_optimum_matches_scipy(seed, nnodes, chords, nfixed, branch):
    """tests/test_oracle_scipy_pin.py's settings and bounds: cost within 1e-8 relative, float32 poses within 2e-6"""
    G = SCIPY_GAUGES[branch]
    poses0, edges = pg.chain_graph(seed, nnodes, chords, G=G)
    if branch is not None:
        assert all(gc.quat_branch(T) == branch for T in poses0)
    out, st = pg.solve(poses0, nfixed, edges, 60)
    T0 = [pg.pose_in(p) for p in poses0]
    Zs = [pg.edge_Z(e) for e in edges]
    sw = np.sqrt(np.stack([[e["w_rot"]] * 3 + [e["w_trans"]] * 3 for e in edges]))

    def fun(x):
        T = [T0[k] if k < nfixed else _compose(x[6 * (k - nfixed):6 * (k - nfixed) + 6], T0[k]) for k in range(nnodes)]
        return np.concatenate([s * pg.residual(Z, T[e["a"]], T[e["b"]]) for e, Z, s in zip(edges, Zs, sw)])

    r = least_squares(fun, np.zeros(6 * (nnodes - nfixed)), jac="3-point", method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15,
                      gtol=1e-15, max_nfev=400)
    cost = 2.0 * r.cost
    assert abs(st[2] - cost) <= 1e-8 * cost, (st[2], cost)
    for k in range(nfixed, nnodes):
        T = _compose(r.x[6 * (k - nfixed):6 * (k - nfixed) + 6], T0[k])
        assert np.abs(T - out[k]).max() < 2e-6
    assert np.array_equal(out[:nfixed], poses0[:nfixed])


def test_far_start_rejects_trials():
    """the case tests/test_gpu_pose_graph.py runs for the rejection path: rejected trials, none of them decided by rounding"""
    poses0, edges, nfixed, iters = pg.rejecting_case()
    trace = []
    out, st = pg.solve(poses0, nfixed, edges, iters, trace=trace)
    assert sum(1 for t in trace if not t[3]) >= 3 and st[4] > st[0] == iters
    assert min(abs(t[2]) for t in trace) > 0.04
    assert st[2] < st[1]


def test_malformed_and_empty_graphs_keep_their_poses():
    poses0, edges = pg.chain_graph(2, 4, [(0, 3)])      # edge 1 is (1, 2)
    for field, value in (("a", 4), ("b", -1), ("a", 2), ("w_rot", np.nan), ("w_trans", np.inf), ("t", (0, np.nan, 0)), ("q", (0, 0, 0, 0)),
                         ("w_rot", -1.0)):              # ("a", 2): a == b
        bad = edges.copy()
        bad[field][1] = value
        out, st = pg.solve(poses0, 1, bad, 5)
        assert st[7] == -1 and not st[:7].any() and out.tobytes() == poses0.tobytes(), (field, value)
    out, st = pg.solve_batch(poses0[None], 1, edges[None], [len(edges) + 1], 5)      # a count above the pitch
    assert st[0, 7] == -1 and out.tobytes() == poses0.tobytes()
    out, st = pg.solve(poses0, 1, edges[:0], 5)
    assert st[7] == 0 and not st.any() and out.tobytes() == poses0.tobytes()
    out, st = pg.solve(poses0, 1, edges, 0)
    assert st[0] == 0 and st[1] == st[2] > 0 and out.tobytes() == poses0.tobytes()


# The drift case: RMS camera-centre error against the ground truth before -> after, measured with this solver (20 iterations):
#   N = 16, seed 1: 0.7265 -> 0.0886 m (ratio 8.2);   N = 32, seed 2: 0.6665 -> 0.1478 m (ratio 4.5)
# Seeds 3 (N = 32) and 4 (N = 64) give ratios of only 2.0 and 1.85 at a scipy optimum and are not used for the bound.
@pytest.mark.parametrize("N,seed,before,after", [(16, 1, 0.7265, 0.0886), (32, 2, 0.6665, 0.1478)])
def test_loop_edge_takes_out_the_drift(N, seed, before, after):
    truth, poses0, edges = pg.circuit(seed, N)
    out, st = pg.solve(poses0, 1, edges, 20)
    e0, e1 = pg.centre_rms(poses0, truth), pg.centre_rms(out, truth)
    print("drift N=%d seed=%d: %.4f -> %.4f m (ratio %.2f), chi2 %.4g -> %.4g" % (N, seed, e0, e1, e0 / e1, st[1], st[2]))
    assert abs(e0 - before) < 2e-3 and abs(e1 - after) < 2e-3
    assert e1 <= 0.5 * e0
