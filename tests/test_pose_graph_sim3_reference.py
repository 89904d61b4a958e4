"""CPU tests of tests/pose_graph_sim3_reference.py, the numpy yardstick of tb_pose_graph_sim3_batch_dev: Exp / Log across their
switches and against SE(3), Ad and ad against the matrix form, the Jacobians against central differences and the series order
they fix, a consistent graph, the optimum against scipy.optimize.least_squares, the SE(3) equivalence, a start that makes LM reject,
malformed graphs, and the scale-drift case the operator exists for."""
import numpy as np
import pytest
from scipy.linalg import expm
from scipy.optimize import least_squares

import pose_graph_reference as pg
import pose_graph_sim3_reference as s3


def _hat7(x):
    """the 4 x 4 generator of (omega, upsilon, sigma)"""
    G = np.zeros((4, 4))
    G[:3, :3] = pg.hat(x[:3]) + x[6] * np.eye(3)
    G[:3, 3] = x[3:6]
    return G


def _unit(rng, n):
    v = rng.normal(0, 1, n)
    return v / np.linalg.norm(v)


ANGLES = [0.0, 3e-6, 0.5 * s3.SMALL, 0.999 * s3.SMALL, 1.001 * s3.SMALL, 1.0, 3.0]
SIGMAS = [0.0, 1e-9, -0.5 * s3.SMALL_S, 0.999 * s3.SMALL_S, 1.001 * s3.SMALL_S, -0.999 * s3.SMALL_S, -1.001 * s3.SMALL_S, 0.7, -1.5]


@pytest.mark.parametrize("angle", ANGLES)
def test_log_inverts_exp_on_both_sides_of_every_switch(angle):
    """3e-6 is below Exp's and Log's own switch (1e-5); the others straddle SMALL, and every sigma straddles SMALL_S. Exp is also
    held to the matrix exponential of the generator, which knows no switch."""
    rng = np.random.default_rng(3)
    for sigma in SIGMAS:
        u = np.concatenate([_unit(rng, 3) * angle, rng.normal(0, 2, 3), [sigma]])
        S = s3.exp(u)
        assert np.abs(s3.log(S) - u).max() < 1e-12, (angle, sigma)
        assert np.abs(S - expm(_hat7(u))).max() < 1e-13 * max(1.0, np.abs(S).max()), (angle, sigma)


def test_exp_is_continuous_across_the_switches():
    """the two branches of every coefficient agree at the switch: a step of 1e-9 relative across it moves W by no more than the
    step's own first-order effect plus the series' 2e-11"""
    rng = np.random.default_rng(4)
    for sigma in (0.0, 0.05, 0.5, -1.0):
        d = _unit(rng, 3)
        Wa, Wb = s3.w_matrix(d * s3.SMALL * (1 - 1e-9), sigma), s3.w_matrix(d * s3.SMALL * (1 + 1e-9), sigma)
        assert np.abs(Wa - Wb).max() < 2e-11 + 1e-9, sigma
    for theta in (0.0, 0.05, 0.5, 2.0):
        d = _unit(rng, 3) * theta
        for sign in (1, -1):
            Wa, Wb = s3.w_matrix(d, sign * s3.SMALL_S * (1 - 1e-9)), s3.w_matrix(d, sign * s3.SMALL_S * (1 + 1e-9))
            assert np.abs(Wa - Wb).max() < 2e-11 + 1e-9, (theta, sign)
    # the series against the closed forms just above the switches, where both are good: 2e-11 relative
    for theta, sigma in ((0.0999999, 0.3), (0.0999999, 0.0999999), (0.05, 0.0999999), (0.0999999, -0.7)):
        A, B, C = s3.w_coeffs(theta, sigma)
        es, d = np.exp(sigma), sigma * sigma + theta * theta
        Cx = np.expm1(sigma) / sigma
        Ax = (es * (sigma * np.sin(theta) - theta * np.cos(theta)) + theta) / (theta * d)
        assert abs(A - Ax) < 2e-11 * abs(Ax) and abs(C - Cx) < 2e-11 * abs(Cx), (theta, sigma)
        if theta > 0.09:      # B's closed form cancels like theta^2: only comparable to eps / theta^2 there
            Bx = (Cx - (es * (sigma * np.cos(theta) + theta * np.sin(theta)) - sigma) / d) / (theta * theta)
            assert abs(B - Bx) < 2e-11 * abs(Bx) + 1e-13, (theta, sigma)


@pytest.mark.parametrize("angle", [0.0, 3e-6, 0.5, 1.0, 2.0, 3.0])
def test_with_sigma_zero_exp_and_log_are_se3s(angle):
    rng = np.random.default_rng(6)
    u = np.concatenate([_unit(rng, 3) * angle, rng.normal(0, 1, 3)])
    T = pg.exp(u)
    assert np.abs(s3.exp(np.concatenate([u, [0.0]])) - T).max() < 1e-14
    r = s3.log(T)
    assert np.abs(r[:6] - pg.log(T)).max() < 1e-14 and abs(r[6]) < 1e-15


def test_inverse_and_composition():
    rng = np.random.default_rng(7)
    S = s3.exp(np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 2, 3), [0.6]]))
    s, R, t = s3.parts(S)
    Si = s3.inv(S)
    assert np.abs(Si @ S - np.eye(4)).max() < 1e-14 and abs(s - np.exp(0.6)) < 1e-14
    assert np.abs(Si - s3.make(1 / s, R.T, -(R.T @ t) / s)).max() == 0
    X = rng.normal(0, 1, 3)
    assert np.abs((S @ np.append(X, 1))[:3] - (s * R @ X + t)).max() < 1e-14
    assert np.abs(s3.srt_to_matrix(s3.srt_from_matrix(S)) - S).max() < 1e-14


def test_adjoint_and_ad_against_the_matrix_form():
    rng = np.random.default_rng(8)
    for _ in range(5):
        S = s3.exp(np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 2, 3), rng.normal(0, 0.5, 1)]))
        xi, r = rng.normal(0, 1, 7), rng.normal(0, 1, 7)
        assert np.abs(S @ _hat7(xi) @ np.linalg.inv(S) - _hat7(s3.adjoint(S) @ xi)).max() < 1e-13
        assert np.abs(_hat7(r) @ _hat7(xi) - _hat7(xi) @ _hat7(r) - _hat7(s3.ad(r) @ xi)).max() < 1e-13
        assert np.abs(s3.adjoint(s3.exp(r)) - expm(s3.ad(r))).max() < 1e-12


def _central(f, h):
    """five-point central differences of f at 0 along the 7 axes"""
    J = np.zeros((7, 7))
    for k in range(7):
        d = np.zeros(7)
        d[k] = h
        J[:, k] = (-f(2 * d) + 8 * f(d) - 8 * f(-d) + f(-2 * d)) / (12 * h)
    return J


def _jacobian_errors(r, rng, orders=(s3.JL_ORDER,)):
    """worst |J - central differences| over J_a and J_b of an edge whose residual is r, for each series order"""
    Z, Sa = (s3.exp(np.concatenate([rng.normal(0, 0.8, 3), rng.normal(0, 2, 3), rng.normal(0, 0.3, 1)])) for _ in range(2))
    Sb = Z @ s3.exp(r) @ Sa
    Zi = s3.inv(Z)
    E = Zi @ Sb @ s3.inv(Sa)
    rr = s3.log(E)
    assert np.abs(rr - r).max() < 1e-11
    Jb = _central(lambda d: s3.residual(Z, Sa, s3.exp(d) @ Sb), 1e-3)
    Ja = _central(lambda d: s3.residual(Z, s3.exp(d) @ Sa, Sb), 1e-3)
    return [max(np.abs(s3.jl_inv(rr, o) @ s3.adjoint(Zi) - Jb).max(), np.abs(-s3.jl_inv(rr, o) @ s3.adjoint(E) - Ja).max()) for o in orders]


@pytest.mark.parametrize("norm", [0.1, 1.0])
def test_jacobians_match_central_differences(norm):
    rng = np.random.default_rng(11)
    for _ in range(4):
        r = _unit(rng, 7) * norm
        assert _jacobian_errors(r, rng)[0] < 1e-6
        _, Ja, Jb = s3.jacobians(np.eye(4), np.eye(4), s3.exp(r))
        assert Ja.shape == Jb.shape == (7, 7)


def test_series_order_is_the_smallest_that_gives_1e_9_over_the_domain():
    """|omega| <= 2, |upsilon| <= 5, |sigma| <= 1, every fourth draw with all three norms at the domain's edge. The reference file
    records 4.8e-10 over 4000 draws (and 3.6e-9 at two orders less); 240 draws of the same stream are run here."""
    rng = np.random.default_rng(0)
    worst = np.zeros(2)
    for i in range(240):
        f = (1.0, 1.0, 1.0) if i % 4 == 0 else rng.uniform(0, 1, 3)
        r = np.concatenate([_unit(rng, 3) * s3.JL_DOMAIN["omega"] * f[0], _unit(rng, 3) * s3.JL_DOMAIN["upsilon"] * f[1],
                            _unit(rng, 1) * s3.JL_DOMAIN["sigma"] * f[2]])
        worst = np.maximum(worst, _jacobian_errors(r, rng, (s3.JL_ORDER, s3.JL_ORDER - 2)))
    print("Jl^-1 order %d: worst %.3g; order %d: worst %.3g" % (s3.JL_ORDER, worst[0], s3.JL_ORDER - 2, worst[1]))
    assert worst[0] < 1e-9 < worst[1]
    assert worst[0] <= s3.JL_WORST * 1.0000001


def test_consistent_graph_does_not_move():
    rng = np.random.default_rng(5)
    S = [s3.exp(np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 3, 3), rng.normal(0, 0.3, 1)])) for _ in range(6)]
    nodes = np.stack([s3.srt_from_matrix(X) for X in S])
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (4, 1)]
    edges = np.array([s3.make_edge(a, b, s3.srt_to_matrix(nodes[b]) @ s3.inv(s3.srt_to_matrix(nodes[a]))) for a, b in pairs])
    for fixed_scale in (False, True):
        out, st = s3.solve(nodes, 1, edges, 10, fixed_scale)
        assert st[1] < 1e-25 and st[2] <= st[1]       # rounding of float64 on residuals of order 1e-16
        assert np.abs(out - nodes).max() < 1e-9 and out[0].tobytes() == nodes[0].tobytes()


def _scipy_optimum(nodes0, nfixed, edges, fixed_scale):
    """scipy.optimize.least_squares on the same residual with tests/test_oracle_scipy_pin.py's settings: (chi2, nodes as 4 x 4)"""
    n = len(nodes0)
    D = 6 if fixed_scale else 7
    S0 = [s3.srt_to_matrix(v) for v in nodes0]
    Zs = [s3.srt_to_matrix(e["srt"]) for e in edges]
    sw = np.sqrt(np.stack([[e["w_rot"]] * 3 + [e["w_trans"]] * 3 + [e["w_scale"]] for e in edges]))

    def node(x, k):
        if k < nfixed:
            return S0[k]
        d = np.zeros(7)
        d[:D] = x[D * (k - nfixed):D * (k - nfixed) + D]
        return s3.exp(d) @ S0[k]

    def fun(x):
        S = [node(x, k) for k in range(n)]
        return np.concatenate([w * s3.residual(Z, S[e["a"]], S[e["b"]]) for e, Z, w in zip(edges, Zs, sw)])

    r = least_squares(fun, np.zeros(D * (n - nfixed)), jac="3-point", method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                      max_nfev=400)
    return 2.0 * r.cost, [node(r.x, k) for k in range(n)]


@pytest.mark.parametrize("seed,nnodes,chords,nfixed,fixed_scale,w", [
    (31, 6, [(0, 5)], 1, False, (1.0, 1.0, 1.0)), (31, 6, [(0, 5)], 1, True, (1.0, 1.0, 1.0)),
    (32, 12, [(0, 11), (3, 9)], 1, False, (4.0, 0.5, 2.0)), (32, 12, [(0, 11), (3, 9)], 2, True, (4.0, 0.5, 2.0)),
    (33, 20, [(0, 19), (4, 15), (16, 2)], 2, False, (0.7, 3.0, 10.0)), (33, 20, [(0, 19), (4, 15), (16, 2)], 1, True, (1.0, 1.0, 1.0))])
def test_optimum_matches_scipy(seed, nnodes, chords, nfixed, fixed_scale, w):
    """cost within 1e-8 relative, nodes within 2e-6"""
    nodes0, edges = s3.chain_graph(seed, nnodes, chords, w=w)
    out, st = s3.solve(nodes0, nfixed, edges, 60, fixed_scale)
    cost, S = _scipy_optimum(nodes0, nfixed, edges, fixed_scale)
    assert abs(st[2] - cost) <= 1e-8 * cost, (st[2], cost)
    for k in range(nnodes):
        assert np.abs(s3.srt_to_matrix(out[k]) - S[k]).max() < 2e-6
    assert out[:nfixed].tobytes() == nodes0[:nfixed].tobytes()
    if fixed_scale:
        assert out[:, 7].tobytes() == nodes0[:, 7].tobytes()


@pytest.mark.parametrize("seed,nnodes,chords,nfixed,iters", [(2, 4, [(0, 3)], 1, 10), (3, 7, [(0, 6), (2, 6), (2, 6), (5, 1)], 1, 10),
                                                             (33, 20, [(0, 19), (4, 15)], 2, 4)])
def test_with_every_scale_1_and_the_scale_held_it_is_the_se3_pose_graph(seed, nnodes, chords, nfixed, iters):
    """final chi2 within 1e-9 relative and the same counts; the poses within 1e-9 of pose_graph_reference.solve's, which returns
    them as float32 -- so within 1e-9 plus that rounding, half a unit in the last place of float32. The 20-node graph stops at 4
    iterations: by the seventh both solvers sit on chi2's rounding floor, where the count of rejected trials is noise."""
    poses0, e6 = pg.chain_graph(seed, nnodes, chords, w=(2.0, 0.5))
    ref, rst = pg.solve(poses0, nfixed, e6, iters)
    nodes0, edges = s3.nodes_from_se3(poses0), s3.edges_from_se3(e6, w_scale=3.0)
    assert np.all(nodes0[:, 7] == 1.0) and np.all(edges["srt"][:, 7] == 1.0)
    out, st = s3.solve(nodes0, nfixed, edges, iters, fixed_scale=True)
    assert st[0] == rst[0] and st[4] == rst[4]
    assert abs(st[1] - rst[1]) <= 1e-9 * rst[1] and abs(st[2] - rst[2]) <= 1e-9 * rst[2], (st, rst)
    assert np.all(out[:, 7] == 1.0)
    for k in range(nnodes):
        T = s3.srt_to_matrix(out[k])
        assert np.all(np.abs(T - ref[k]) <= 1e-9 + 0.5 * np.spacing(np.abs(ref[k]).astype(np.float32)).astype(np.float64)), k


def test_far_start_rejects_trials():
    """the case tests/test_gpu_pose_graph_sim3.py runs for the rejection path: rejected trials, none of them decided by rounding"""
    nodes0, edges, nfixed, iters = s3.rejecting_case()
    trace = []
    out, st = s3.solve(nodes0, nfixed, edges, iters, trace=trace)
    assert sum(1 for t in trace if not t[3]) >= 2 and st[4] > st[0] == iters
    assert min(abs(t[2]) for t in trace) > 0.04
    assert st[2] < st[1]


def test_malformed_and_empty_graphs_keep_their_nodes():
    nodes0, edges = s3.chain_graph(2, 4, [(0, 3)])      # edge 1 is (1, 2)
    srt = edges["srt"][1].copy()

    def with_srt(i, v):
        out = srt.copy()
        out[i] = v
        return out

    for field, value in (("a", 4), ("b", -1), ("a", 2), ("w_rot", np.nan), ("w_trans", np.inf), ("w_rot", -1.0), ("w_scale", -1.0),
                         ("w_scale", np.nan), ("w_scale", np.inf), ("srt", with_srt(5, np.nan)), ("srt", with_srt(slice(0, 4), 0.0)),
                         ("srt", with_srt(7, 0.0)), ("srt", with_srt(7, -2.0)), ("srt", with_srt(7, np.inf)), ("srt", with_srt(7, np.nan))):
        bad = edges.copy()
        bad[field][1] = value
        for fixed_scale in (False, True):
            out, st = s3.solve(nodes0, 1, bad, 5, fixed_scale)
            assert st[7] == -1 and not st[:7].any() and out.tobytes() == nodes0.tobytes(), (field, value)
    for k, i, value in ((0, 7, 0.0), (2, 7, -1.0), (3, 7, np.nan), (1, 4, np.inf), (2, slice(0, 4), 0.0)):
        bad = nodes0.copy()
        bad[k, i] = value
        out, st = s3.solve(bad, 1, edges, 5)
        assert st[7] == -1 and not st[:7].any() and out.tobytes() == bad.tobytes(), (k, i, value)
    out, st = s3.solve_batch(nodes0[None], 1, edges[None], [len(edges) + 1], 5)      # a count above the pitch
    assert st[0, 7] == -1 and out.tobytes() == nodes0.tobytes()
    out, st = s3.solve(nodes0, 1, edges[:0], 5)
    assert st[7] == 0 and not st.any() and out.tobytes() == nodes0.tobytes()
    out, st = s3.solve(nodes0, 1, edges, 0)
    assert st[0] == 0 and st[1] == st[2] > 0 and out.tobytes() == nodes0.tobytes()


# The drift case (pose_graph_sim3_reference.circuit: the map scale grows by exp(N(0.01, 0.01)) per odometry edge): RMS camera-centre
# error against the ground truth before, after the SE(3) graph with the scales ignored, and after the Sim(3) graph (20 iterations):
#   N = 16, seed 1: 1.6735 -> SE(3) 1.5833 -> Sim(3) 0.1818 m (SE(3) / Sim(3) = 8.7; 8.7 at the scipy optimum)
#   N = 32, seed 2: 3.6762 -> SE(3) 3.5724 -> Sim(3) 0.2813 m (SE(3) / Sim(3) = 12.7; 12.7 at the scipy optimum)
@pytest.mark.parametrize("N,seed,before,se3,sim3", [(16, 1, 1.6735, 1.5833, 0.1818), (32, 2, 3.6762, 3.5724, 0.2813)])
def test_sim3_loop_edge_takes_out_the_scale_drift(N, seed, before, se3, sim3):
    truth, nodes0, edges, poses0, se3_edges = s3.circuit(seed, N)
    out, st = s3.solve(nodes0, 1, edges, 20)
    out6, st6 = pg.solve(poses0, 1, se3_edges, 20)
    e0, e6, e7 = s3.centre_rms(nodes0, truth), pg.centre_rms(out6, truth), s3.centre_rms(out, truth)
    print("scale drift N=%d seed=%d: %.4f -> SE(3) %.4f, Sim(3) %.4f m (ratio %.2f), chi2 %.4g -> %.4g" % (N, seed, e0, e6, e7, e6 / e7, st[1], st[2]))
    assert abs(e0 - pg.centre_rms(poses0, truth)) < 1e-6
    assert abs(e0 - before) < 2e-3 and abs(e6 - se3) < 2e-3 and abs(e7 - sim3) < 2e-3
    assert e6 / e7 >= 0.5 * (se3 / sim3)
