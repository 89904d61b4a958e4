"""CPU tests of the two-view definition (tests/two_view_reference.py, the definition tb_two_view_batch_dev is held to) on the
constructed cases of tests/two_view_cases.py: ground truth, an independent build of the same pipeline on numpy.linalg.svd / eigh,
the failure cases, batch invariance and the exclusions.

Measured on the twelve forward cases (DESIGN.md 9m has the table): the worst Frobenius rotation error against ground truth is
1.158e-2 and the worst 1 - cosine of the translation direction 2.03e-4; against the independent build 7.11e-13 and 2.2e-16. The
bounds below are twice those."""
import numpy as np
import pytest

import two_view_cases as tc
import two_view_reference as tv

ROT_BOUND = 2.32e-2
COS_BOUND = 1.0 - 4.06e-4
ROT_BOUND_INDEPENDENT = 1.43e-12
COS_BOUND_INDEPENDENT = 1.0 - 4.5e-16
SEED = 3
FORWARD = [(d, noise, out) for d in (2.5, 5.0) for noise in (0.1, 0.3) for out in (0.0, 0.2, 0.3)]


def independent(K, xy0, xy1, prm):
    """the same pipeline on numpy.linalg: null vectors by SVD, the refit by eigh, the decomposition by SVD, cheirality by the depths of
    an SVD triangulation. The samples are the definition's (tv.sample; test_the_sampling_rule_by_hand pins that rule on its own) and
    the consensus rule is restated in matrix form."""
    fx, fy, cx, cy = K
    Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    n = len(xy0)
    p0 = np.concatenate([xy0.astype(np.float64), np.ones((n, 1))], 1)
    p1 = np.concatenate([xy1.astype(np.float64), np.ones((n, 1))], 1)
    q0, q1 = p0 @ Ki.T, p1 @ Ki.T
    A = np.einsum("ni,nj->nij", q1, q0).reshape(n, 9)
    idx, ok = tv.sample(prm["seed"], prm["hypotheses"], n)

    def mask_of(E):
        F = Ki.T @ E @ Ki
        l1, l0 = p0 @ F.T, p1 @ F
        d = np.sum(p1 * l1, 1)
        return (d * d / (l1[:, 0] ** 2 + l1[:, 1] ** 2) <= prm["chi2_epi"]) & (d * d / (l0[:, 0] ** 2 + l0[:, 1] ** 2) <= prm["chi2_epi"])

    best, bh, bE = -1, -1, None
    for h in range(prm["hypotheses"]):
        if not ok[h]:
            continue
        _, s, vt = np.linalg.svd(A[idx[h]])
        if s[7] <= 1e-12 * s[0]:
            continue
        E = vt[8].reshape(3, 3)
        c = int(mask_of(E).sum())
        if c > best:
            best, bh, bE = c, h, E
    m = mask_of(bE)
    if prm["refit"]:
        bE = np.linalg.eigh(A[m].T @ A[m])[1][:, 0].reshape(3, 3)
        m = mask_of(bE)
    U, _, Vt = np.linalg.svd(bE)
    U = -U if np.linalg.det(U) < 0 else U
    Vt = -Vt if np.linalg.det(Vt) < 0 else Vt
    W = np.array([[0, -1.0, 0], [1, 0, 0], [0, 0, 1]])
    cands = [(U @ W @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W.T @ Vt, -U[:, 2])]
    score = []
    for R, t in cands:
        P0, P1 = np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R, t[:, None]])
        cnt = 0
        for a, b in zip(q0[m], q1[m]):
            X = np.linalg.svd(np.stack([a[0] * P0[2] - P0[0], a[1] * P0[2] - P0[1], b[0] * P1[2] - P1[0], b[1] * P1[2] - P1[1]]))[2][3]
            X = X[:3] / X[3]
            cnt += bool(X[2] > 0 and (R @ X + t)[2] > 0)
        score.append(cnt)
    c = int(np.argmax(score))
    return dict(h=bh, R=cands[c][0], t=cands[c][1], mask=m)


@pytest.fixture(scope="module")
def forward():
    """the twelve forward cases, each solved once: (problem, result)"""
    out = {}
    for case in FORWARD:
        prob = tc.problem(1, kind="forward", d=case[0], noise=case[1], outliers=case[2])
        out[case] = (prob, tv.two_view(tc.K, prob[0], prob[1], prm=tv.params(seed=SEED)))
    return out


@pytest.mark.parametrize("case", FORWARD)
def test_forward_drive_initialises_near_the_truth(forward, case):
    (xy0, xy1, good, R, t), r = forward[case]
    inl = r["inlier"].astype(bool)
    rot, cos = tc.pose_error(r["R"], r["t"], R, t)
    print("case", case, "true inliers kept %.4f" % ((inl & good).sum() / good.sum()), "outliers among the consensus %.4f" %
          ((inl & ~good).sum() / inl.sum()), "rotation %.3e" % rot, "1 - cos %.3e" % (1 - cos))
    assert r["status"] == tv.OK
    assert (inl & good).sum() >= 0.95 * good.sum() and (inl & ~good).sum() <= 0.02 * inl.sum()
    assert rot <= ROT_BOUND and cos >= COS_BOUND
    assert r["consensus"] == inl.sum() and r["good"][r["winner"][1]] >= 0.9 * r["consensus"]
    assert (r["point_flags"] == 1).sum() == r["tri"][r["winner"][1]] == r["written"].sum() >= 50
    # the points, through the pose that came back, lie in front of both cameras at the unit baseline
    X = r["points"][r["written"]].astype(np.float64)
    assert (X[:, 2] > 0).all() and ((X @ r["Tcw1_64"][:3, :3].T + r["Tcw1_64"][:3, 3])[:, 2] > 0).all()
    assert abs(np.linalg.norm(r["Tcw1_64"][:3, 3]) - 1.0) < 1e-12


@pytest.mark.parametrize("case", FORWARD)
def test_the_definition_agrees_with_an_independent_build(forward, case):
    (xy0, xy1, _, _, _), r = forward[case]
    i = independent(tc.K, xy0, xy1, tv.params(seed=SEED))
    rot, cos = tc.pose_error(r["R"], r["t"], i["R"], i["t"])
    print("case", case, "rotation %.3e" % rot, "1 - cos %.3e" % (1 - cos))
    assert r["winner"][0] == i["h"] and np.array_equal(r["inlier"].astype(bool), i["mask"])
    assert rot <= ROT_BOUND_INDEPENDENT and cos >= COS_BOUND_INDEPENDENT


def test_the_refit_sweep_count_is_the_smallest_that_reaches_eigh(forward):
    """REFIT_SWEEPS is the smallest count at which the refitted E agrees with numpy.linalg.eigh's to 1e-12 relative on the forward cases"""
    worst = {}
    keep = tv.REFIT_SWEEPS
    try:
        for case in FORWARD:
            xy0, xy1 = forward[case][0][:2]
            r0 = tv.two_view(tc.K, xy0, xy1, prm=tv.params(seed=SEED, refit=0))
            mask = r0["inlier"].astype(bool)
            rows = [xy0[:, 0].astype(np.float64), xy0[:, 1].astype(np.float64), xy1[:, 0].astype(np.float64), xy1[:, 1].astype(np.float64)]
            x0, y0 = tv.normalise(rows[0], rows[1], tc.K)
            x1, y1 = tv.normalise(rows[2], rows[3], tc.K)
            a = np.stack(tv.epipolar_row(x0, y0, x1, y1), -1)[mask]
            e = np.linalg.eigh(a.T @ a)[1][:, 0]
            for sweeps in (keep - 1, keep):
                tv.REFIT_SWEEPS = sweeps
                E = np.array(tv.refit(rows, mask, tc.K))
                E = -E if np.dot(E, e) < 0 else E
                worst[sweeps] = max(worst.get(sweeps, 0.0), float(np.abs(E - e).max() / np.abs(e).max()))
    finally:
        tv.REFIT_SWEEPS = keep
    print("refit against eigh, worst relative difference by sweeps", worst)
    assert worst[keep] <= 1e-12 < worst[keep - 1]


def test_half_a_metre_is_too_little_parallax():
    xy0, xy1, _, _, _ = tc.problem(1, kind="forward", d=0.5, noise=0.1)
    r = tv.two_view(tc.K, xy0, xy1, prm=tv.params(seed=SEED))
    assert r["status"] == tv.FEW_POINTS and not r["written"].any() and r["Tcw1_64"] is None
    assert np.array_equal(r["Tcw1"], np.eye(4, dtype=np.float32)) and r["consensus"] >= 0.95 * len(xy0)


def test_identical_point_sets_are_void():
    xy0, xy1, _, _, _ = tc.problem(1, kind="none", noise=0.0)
    assert np.array_equal(xy0, xy1)
    r = tv.two_view(tc.K, xy0, xy1, prm=tv.params(seed=SEED))
    assert r["status"] == tv.VOID and r["winner"] == (-1, -1) and r["consensus"] == 0 and (r["counts"] == -1).all()


def test_pure_rotation_is_refused():
    xy0, xy1, _, _, _ = tc.problem(1, kind="rotation", d=0.03, noise=0.1)
    r = tv.two_view(tc.K, xy0, xy1, prm=tv.params(seed=SEED))
    assert r["status"] != tv.OK and not r["written"].any()


def test_sideways_is_refused_or_right():
    xy0, xy1, _, R, t = tc.problem(1, kind="sideways", d=1.0, noise=0.1)
    r = tv.two_view(tc.K, xy0, xy1, prm=tv.params(seed=SEED))
    if r["status"] == tv.OK:
        rot, cos = tc.pose_error(r["R"], r["t"], R, t)
        print("sideways: rotation %.3e, 1 - cos %.3e" % (rot, 1 - cos))
        assert rot <= ROT_BOUND and cos >= COS_BOUND


def _same(a, b):
    for k in ("status", "consensus", "winner"):
        assert a[k] == b[k], k
    for k in ("Tcw1", "points", "written", "point_flags", "inlier", "good", "tri"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_a_problem_gives_the_same_bits_alone_and_inside_a_batch():
    probs = [tc.problem(s, 256, "forward", 2.5, 0.1, o) for s, o in ((1, 0.0), (2, 0.3), (3, 0.2))]
    xy0, xy1 = np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs])
    prm = tv.params(seed=SEED)
    batch = tv.two_view_batch(tc.K, xy0, xy1, prm=prm)
    swapped = tv.two_view_batch(tc.K, xy0[::-1], xy1[::-1], prm=prm)
    for p in range(3):
        _same(batch[p], tv.two_view(tc.K, xy0[p], xy1[p], prm=prm))
        _same(batch[p], swapped[2 - p])
    a, b = tv.sample(SEED, 64, 256), tv.sample(SEED, 256, 256)       # a sample depends on (seed, h, n) only
    assert np.array_equal(a[0], b[0][:64]) and np.array_equal(a[1], b[1][:64])
    assert all(len(set(r)) == 8 and min(r) >= 0 and max(r) < 256 for r, ok in zip(*b) if ok)


def test_the_sampling_rule_by_hand():
    """the rule the header states -- draw k of hypothesis h is mix(seed + (16 h + k + 1) * 0x9E3779B97F4A7C15), high 32 bits times n
    shifted right by 32, eight distinct candidates within 16 draws -- restated on Python integers, and four samples written out"""
    mask = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    def by_hand(seed, h, n):
        out = []
        for k in range(16):
            d = ((mix((seed + (16 * h + k + 1) * 0x9E3779B97F4A7C15) & mask) >> 32) * n) >> 32
            if d not in out and len(out) < 8:
                out.append(d)
        return out

    literal = {(3, 0, 520): [58, 364, 318, 37, 112, 330, 70, 462], (3, 255, 520): [364, 336, 456, 390, 102, 33, 361, 115],
               (11, 7, 9): [7, 5, 3, 0, 6, 4], (0, 1, 8): [3, 6, 1, 5, 7, 2, 4]}
    for (seed, h, n), rows in literal.items():
        idx, ok = tv.sample(seed, h + 1, n)
        assert by_hand(seed, h, n) == rows
        assert [int(i) for i in idx[h] if i >= 0] == rows and bool(ok[h]) == (len(rows) == 8), (seed, h, n)
    for h in range(40):
        idx, ok = tv.sample(5, 40, 300)
        assert [int(i) for i in idx[h] if i >= 0] == by_hand(5, h, 300), h


def test_exclusions():
    xy0, xy1, _, _, _ = tc.problem(4, 256, "forward", 2.5, 0.1, 0.0)
    prm = tv.params(seed=SEED)
    for n in (0, 7, -3):
        r = tv.two_view(tc.K, xy0, xy1, n, prm=prm)
        assert r["status"] == tv.VOID and not r["inlier"].any() and np.array_equal(r["Tcw1"], np.eye(4, dtype=np.float32))
    skip = np.ones(256, np.uint8)
    skip[:7] = 0
    assert tv.two_view(tc.K, xy0, xy1, skip=skip, prm=prm)["status"] == tv.VOID      # seven candidates
    assert tv.two_view(tc.K, xy0, xy1, 8, prm=prm)["status"] not in (tv.OK, tv.VOID) # eight rows: a pose, too few points
    _same(tv.two_view(tc.K, xy0, xy1, 256 + 40, prm=prm), tv.two_view(tc.K, xy0, xy1, prm=prm))   # a count above the pitch is clamped
    # a skip mask: the result is that of the rows that are left, at their places
    skip = np.zeros(256, np.uint8)
    skip[::5] = 1
    keep = skip == 0
    a = tv.two_view(tc.K, xy0, xy1, skip=skip, prm=prm)
    b = tv.two_view(tc.K, xy0[keep], xy1[keep], prm=prm)
    assert a["status"] == b["status"] == tv.OK and a["winner"] == b["winner"] and not a["inlier"][~keep].any()
    assert np.array_equal(a["inlier"][keep], b["inlier"]) and a["Tcw1"].tobytes() == b["Tcw1"].tobytes()
    assert a["points"][keep].tobytes() == b["points"].tobytes() and not a["point_flags"][~keep].any()
    # rows that are not finite are never in the consensus and never make a NaN
    bad0, bad1 = xy0.copy(), xy1.copy()
    bad0[5, 0] = np.nan
    bad1[9, 1] = np.inf
    bad1[13] = np.nan
    r = tv.two_view(tc.K, bad0, bad1, prm=prm)
    assert r["status"] == tv.OK and not r["inlier"][[5, 9, 13]].any() and np.isfinite(r["Tcw1"]).all() and np.isfinite(r["points"]).all()
    assert (r["counts"] == -1).sum() > 0                                             # some samples drew such a row: void, not NaN
    r = tv.two_view(tc.K, np.full_like(xy0, np.nan), xy1, prm=prm)
    assert r["status"] == tv.VOID
