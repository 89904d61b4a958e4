"""CPU tests of tests/sim3_opt_reference.py, the numpy definition of tb_sim3_optimize_batch_dev: its Jacobians against central
differences, what it recovers and what it buys over the Horn refit, its optimum against scipy's, the outlier round and the
procedure's edges. Every test prints the figures it asserts on (pytest -s shows them); DESIGN.md 9p records them."""
import numpy as np
import pytest
import scipy.optimize

import pose_graph_sim3_reference as ps
import sim3_opt_cases as oc
import sim3_opt_reference as so
import sim3_reference as sr

# measured by the tests below (see each), asserted with the stated margins
JAC_WORST = 6.8e-12        # the worst relative difference between a Jacobian and its five-point central difference
JAC_FLOOR = 1.0e-10        # the same between the central differences at the steps 1e-3 and 5e-4
GAIN_ROT, GAIN_TRANS = 4.94, 3.79      # medians over the five draws of error before / error after, scale free and held together
SCIPY_GAP = 4.7e-15        # the relative gap between the final robust chi2 and scipy's optimum: the sums' rounding
OUTLIER_SEEDS = (0, 1, 2, 3, 4)      # draws of the outlier case for which the reference meets the three conditions (all five do)


def _residuals(d, S, row, K):
    """(e12, e21) of one row under Exp(d) S"""
    X1, X2, uv1, uv2, _, _ = so._fields(row)
    Q1, Q2 = so.mapped(ps.exp(d) @ S, X1, X2)
    return np.concatenate([(uv1 - so.project(Q1, K))[0], (uv2 - so.project(Q2, K))[0]])


def _central(f, h):
    """five-point central difference of f at 0 along every axis of the tangent space: [4, 7]"""
    cols = []
    for k in range(7):
        e = np.zeros(7)
        e[k] = h
        cols.append((-f(2 * e) + 8 * f(e) - 8 * f(-e) + f(-2 * e)) / (12 * h))
    return np.stack(cols, -1)


def test_jacobians_against_central_differences():
    """draws up to 0.8 rad, 2 m and 0.3 of log-scale, depths 2 to 50 m, fx != fy. The difference is relative to the largest
    entry of the Jacobian; the floor is what two step sizes of the central difference disagree by."""
    rng = np.random.default_rng(0)
    K = oc.K_ANISO
    worst = floor = 0.0
    for _ in range(200):
        d = np.concatenate([0.8 * rng.uniform(0, 1) * oc._unit(rng), 2.0 * rng.uniform(0, 1) * oc._unit(rng), [rng.uniform(-0.3, 0.3)]])
        S = ps.exp(d)
        X2 = oc.points(rng, 1, K, 2.0, 50.0)
        X1, _ = so.mapped(S, X2, X2)
        X1 = X1 + rng.normal(0, 0.05, 3)
        if X1[0, 2] < 1.0 or so.mapped(S, X1, X2)[1][0, 2] < 1.0:
            continue
        row = so.make_rows(X1, X2, so.project(X1, K) + rng.normal(0, 2, 2), so.project(X2, K) + rng.normal(0, 2, 2))
        Xa, Xb = so._fields(row)[:2]
        J1, J2 = so.jacobians(S, Xa, Xb, K)
        J = np.concatenate([J1[0], J2[0]])
        f = lambda x: _residuals(x, S, row, K)
        Na, Nb = _central(f, 1e-3), _central(f, 5e-4)
        scale = np.abs(J).max()
        worst = max(worst, np.abs(J - Nb).max() / scale)
        floor = max(floor, np.abs(Na - Nb).max() / scale)
    print("jacobians: worst %.2e, floor %.2e" % (worst, floor))
    assert worst <= min(10 * JAC_WORST, 1e-6)
    assert floor <= 10 * JAC_FLOOR


@pytest.mark.parametrize("fixed", [False, True])
def test_noise_free_rows_recover_the_truth(fixed):
    """float32 rows without noise, from a perturbed seed: test_sim3_reference's noise-free bounds, 1e-6, 1e-6 rad, 1e-5 m"""
    for draw in range(3):
        T = oc.sc.truth(1.0, 0.3, 2.0) if fixed else oc.sc.truth()
        rows, _, T = oc.problem(500 + draw, 200, T=T, pix=0.0, disp=0.0)
        srt0 = oc.perturbed(T, draw, 0.02, 0.1, 0.0 if fixed else 0.02)
        o = so.optimize(oc.K, rows, 200, srt0, fixed_scale=fixed)
        es, er, et = oc.errors(o["srt"], T)
        print("noise-free draw %d fixed %d: scale %.1e rotation %.1e rad translation %.1e m" % (draw, fixed, es, er, et))
        assert o["stats"][7] == 0 and o["inliers"] == 200
        assert es < 1e-6 and er < 1e-6 and et < 1e-5
        if fixed:
            assert o["srt"][7:].tobytes() == srt0[7:].tobytes()


def gain_case(draw, fixed):
    """the depth-noise rows (200 rows at 5 to 40 m, 0.5 px pixel noise, the depth noise of a 0.5 px disparity error, 0.1 rad and
    1.1 m), seeded by sim3_reference's result on the same rows with its mask as the active rows"""
    rows, _, T = oc.problem(1000 + draw, 200)
    r = sr.ransac(oc.K, oc.sim3_rows(rows), 200, fixed_scale=fixed, seed=draw)
    return rows, T, r


def test_the_gain_over_the_horn_refit():
    ratios, table = [], []
    for fixed in (False, True):
        for draw in range(5):
            rows, T, r = gain_case(draw, fixed)
            o = so.optimize(oc.K, rows, 200, r["srt"], active=r["inlier"], fixed_scale=fixed)
            b, a = oc.errors(r["srt"], T), oc.errors(o["srt"], T)
            table.append((fixed, draw) + b + a)
            ratios.append((b[1] / a[1], b[2] / a[2]))
            assert o["stats"][7] == 0 and o["inliers"] >= 0.9 * r["consensus"]
    for t in table:
        print("gain fixed %d draw %d: before scale %.1e rot %.1e trans %.1e | after scale %.1e rot %.1e trans %.1e" % t)
    rot, trans = np.median([r[0] for r in ratios]), np.median([r[1] for r in ratios])
    print("gain: median ratio rotation %.2f translation %.2f; worst %.2f %.2f" % (rot, trans, min(r[0] for r in ratios), min(r[1] for r in ratios)))
    assert rot >= 0.5 * GAIN_ROT and trans >= 0.5 * GAIN_TRANS


def test_against_scipy_least_squares():
    """a case with nBad = 0: the final robust chi2 against scipy's optimum of the same Huber cost, run to convergence"""
    rows, _, T = oc.problem(1003, 200, pix=0.3, disp=0.2)
    srt0 = oc.perturbed(T, 3, 0.005, 0.05, 0.005)
    o = so.optimize(oc.K, rows, 200, srt0)
    assert o["stats"][4] == 0 and o["stats"][7] == 0
    idx = np.arange(200)
    S0 = ps.srt_to_matrix(o["srt"])

    def res(d):
        c1, c2, _, _ = so.row_chi2(ps.exp(d) @ S0, rows[idx], oc.K)
        return np.sqrt(np.concatenate([so.huber(c1, so.TH2)[0], so.huber(c2, so.TH2)[0]]))

    sol = scipy.optimize.least_squares(res, np.zeros(7), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    best = float((sol.fun ** 2).sum())
    gap = (o["stats"][2] - best) / best
    print("scipy: ours %.12f scipy %.12f gap %.2e" % (o["stats"][2], best, gap))
    assert abs(o["stats"][2] - so.cost(S0, rows, idx, oc.K)) < 1e-9 * best
    assert gap <= 10 * SCIPY_GAP


@pytest.mark.parametrize("fixed", [False, True])
def test_the_outlier_round(fixed):
    """30 % of the rows displaced by metres, every row active: nBad > 0 so the second round is the 10-iteration one, no displaced
    row in the final mask, at least 95 % of the good ones in it"""
    for draw in OUTLIER_SEEDS:
        rows, good, T = oc.problem(1100 + draw, 200, outliers=0.3, pix=0.3, disp=0.3)
        srt0 = oc.perturbed(T, draw, 0.005, 0.05, 0.0 if fixed else 0.005)
        trace = []
        o = so.optimize(oc.K, rows, 200, srt0, fixed_scale=fixed, trace=trace)
        rounds = [t[0] for t in trace]
        print("outliers draw %d fixed %d: nBad %d, iterations %d, inliers %d of %d good, errors %s" %
              (draw, fixed, o["stats"][4], o["stats"][0], o["mask"][good].sum(), good.sum(), oc.errors(o["srt"], T)))
        assert o["stats"][4] > 0 and o["stats"][7] == 0 and 1 in rounds
        assert len({t[1] for t in trace if t[0] == 1}) <= so.ITERS_BAD and o["stats"][0] <= so.ITERS_FIRST + so.ITERS_BAD
        assert not o["mask"][~good].any()
        assert o["mask"][good].sum() >= 0.95 * good.sum()


def test_fewer_than_min_keep_rows_left():
    rows, good, T = oc.problem(1200, 40, outliers=0.8)      # 8 good rows
    srt0 = oc.perturbed(T, 0, 0.002, 0.02, 0.0)
    o = so.optimize(oc.K, rows, 40, srt0, fixed_scale=True)
    print("min_keep: stats %s" % o["stats"])
    assert o["stats"][7] == so.FLAG_STOPPED and o["stats"][0] == so.ITERS_FIRST and o["stats"][4] >= 31
    assert o["inliers"] == 0 and not o["mask"].any() and o["srt"].tobytes() == srt0.tobytes()
    assert np.array_equal(o["S12"], so.s12_f32(ps.srt_to_matrix(srt0)))
    # below min_keep before the first round: nothing runs
    a = np.zeros(40, np.uint8)
    a[:9] = 1
    o = so.optimize(oc.K, rows, 40, srt0, active=a)
    assert o["stats"][7] == so.FLAG_STOPPED and o["stats"][0] == 0 and o["stats"][3] == 0 and o["srt"].tobytes() == srt0.tobytes()
    # min_keep 9 lets the same rows run
    assert so.optimize(oc.K, rows[:9], 9, srt0, min_keep=9, th2=1e9)["stats"][7] == 0


def test_malformed_seeds_and_clamped_counts():
    rows, _, T = oc.problem(1201, 50, pitch=64)
    srt0 = oc.perturbed(T, 1)
    for bad in ([0, 0, 0, 0] + list(srt0[4:]), list(srt0[:5]) + [np.nan] + list(srt0[6:]), list(srt0[:7]) + [0.0], list(srt0[:7]) + [-2.0],
                list(srt0[:7]) + [np.inf], [np.inf] + list(srt0[1:])):
        o = so.optimize(oc.K, rows, 50, bad)
        assert o["stats"][7] == so.FLAG_MALFORMED and not o["stats"][:7].any() and o["inliers"] == 0 and not o["mask"].any()
        assert o["srt"].tobytes() == np.array(bad, np.float64).tobytes() and np.array_equal(o["S12"], np.eye(4, dtype=np.float32))
    assert so.optimize(oc.K, rows, -5, srt0)["stats"][7] == so.FLAG_STOPPED
    full = so.optimize(oc.K, rows, 64, srt0, iters_first=2, iters_clean=2)
    over = so.optimize(oc.K, rows, 900, srt0, iters_first=2, iters_clean=2)
    assert full["srt"].tobytes() == over["srt"].tobytes() and full["inliers"] == over["inliers"]
    # an unnormalised quaternion is the same seed
    scaled = srt0.copy()
    scaled[:4] *= -2.5
    a, b = so.optimize(oc.K, rows, 50, srt0, iters_first=2, iters_clean=2), so.optimize(oc.K, rows, 50, scaled, iters_first=2, iters_clean=2)
    assert np.allclose(a["srt"], b["srt"], rtol=0, atol=1e-12) and a["inliers"] == b["inliers"]


def test_dropped_rows():
    rows, _, T = oc.problem(1202, 100)
    srt0 = oc.perturbed(T, 2, 0.002, 0.02, 0.002)
    clean = so.optimize(oc.K, rows, 100, srt0)
    rows["X1"][7] = np.nan
    rows["v2"][11] = np.inf
    rows["inv_sigma2_1"][13] = np.nan
    rows["Z1"][17] = 0.0
    rows["Z2"][19] = -rows["Z2"][19]
    rows["X1"][23], rows["Y1"][23], rows["Z1"][23] = 0.0, 0.0, 0.001      # in front of camera 1, behind camera 2 under the seed
    a = np.ones(100, np.uint8)
    a[[19, 30]] = 0                                                      # a row that is not active is not counted as dropped
    o = so.optimize(oc.K, rows, 100, srt0, active=a)
    print("dropped: %d, inliers %d (clean %d)" % (o["stats"][5], o["inliers"], clean["inliers"]))
    assert o["stats"][5] == 5 and o["stats"][7] == 0 and not o["mask"][[7, 11, 13, 17, 19, 23, 30]].any()
    assert np.isfinite(o["srt"]).all() and np.isfinite(o["stats"]).all() and o["inliers"] >= clean["inliers"] - 7
    assert np.allclose(o["srt"], clean["srt"], atol=2e-2)


def test_the_sum_rule_and_huber():
    """total() is the butterfly of 256 slots; huber() is g2o's kernel, continuous at delta"""
    v = np.random.default_rng(3).normal(0, 1, 700)
    idx = np.arange(700)
    assert abs(so.total(v, idx) - v.sum()) < 1e-12 and so.total(v[:0], idx[:0]) == 0.0
    part = np.array([v[t::256].sum() if False else sum(v[t::256], 0.0) for t in range(256)])
    pair = part.copy()
    d = 1
    while d < 256:
        pair = pair + pair[np.arange(256) ^ d]
        d *= 2
    assert so.total(v, idx) == pair[0]
    rho, w = so.huber(np.array([0.0, 4.0, 10.0, 10.000001, 40.0]), 10.0)
    assert np.allclose(rho[:3], [0, 4, 10]) and abs(rho[3] - 10.000001) < 1e-9 and np.isclose(rho[4], 2 * np.sqrt(400.0) - 10)
    assert np.allclose(w[:3], 1.0) and np.isclose(w[4], 0.5)
