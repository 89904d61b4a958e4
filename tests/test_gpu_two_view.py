"""GPU tests of tb_two_view_batch_dev / tb_two_view against the definition in tests/two_view_reference.py on the constructed
problems of tests/two_view_cases.py: every output bit for bit (Tcw1 and the points as float32 bits), untouched outputs keep
their sentinel. Pitch 256 is one staging chunk, pitch 640 two and a half."""
import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi

import two_view_cases as tc
import two_view_reference as tv

pytestmark = pytest.mark.gpu

PITCH = 256
SEED = 11
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _run(ctx, xy0, xy1, counts=None, skip=None, w0=None, w1=None, Tcw0=None, K=tc.K, **kw):
    """the batched entry -> dict of host arrays; outputs pre-filled so that an unwritten entry shows"""
    P, pitch = xy0.shape[:2]
    d = [_dev(xy0, np.float32), _dev(xy1, np.float32), _dev(counts, np.int32), _dev(skip, np.uint8), _dev(w0, np.float32),
         _dev(w1, np.float32), None if Tcw0 is None else _dev(np.asarray(Tcw0, np.float32).reshape(P, 16), np.float32)]
    full = lambda shape, v, t: torch.full(shape, v, dtype=t, device="cuda")
    T = full((P, 16), SENTINEL, torch.float32)
    pts = full((P, pitch, 3), SENTINEL, torch.float32)
    pf, inl = full((P, pitch), 99, torch.uint8), full((P, pitch), 99, torch.uint8)
    cons, status = full((P,), -9, torch.int32), full((P,), -9, torch.int32)
    win, good, tri = full((P, 2), -9, torch.int32), full((P, 4), -9, torch.int32), full((P, 4), -9, torch.int32)
    torch.cuda.synchronize()
    ctx.check(ctx.two_view_dev(P, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), pitch, K, _ptr(d[3]), _ptr(d[4]), _ptr(d[5]), _ptr(d[6]),
                               T.data_ptr(), pts.data_ptr(), pf.data_ptr(), inl.data_ptr(), cons.data_ptr(), win.data_ptr(),
                               good.data_ptr(), tri.data_ptr(), status.data_ptr(), **kw))
    ctx.synchronize()
    return dict(Tcw1=T.cpu().numpy().reshape(P, 4, 4), points=pts.cpu().numpy(), point_flags=pf.cpu().numpy(), inlier=inl.cpu().numpy(),
                consensus=cons.cpu().numpy(), winner=win.cpu().numpy(), good=good.cpu().numpy(), tri=tri.cpu().numpy(),
                status=status.cpu().numpy())


def _check(got, refs):
    for p, r in enumerate(refs):
        tag = "problem %d" % p
        assert got["status"][p] == r["status"], tag
        assert tuple(got["winner"][p]) == r["winner"] and got["consensus"][p] == r["consensus"], tag
        assert np.array_equal(got["good"][p], r["good"]) and np.array_equal(got["tri"][p], r["tri"]), tag
        assert np.array_equal(got["inlier"][p], r["inlier"]), tag
        assert np.array_equal(got["point_flags"][p], r["point_flags"]), tag
        assert np.array_equal(got["Tcw1"][p].view(np.uint32), r["Tcw1"].view(np.uint32)), tag
        want = np.where(r["written"][:, None], r["points"], np.float32(SENTINEL))
        assert np.array_equal(got["points"][p].view(np.uint32), want.view(np.uint32)), tag


@pytest.fixture(scope="module")
def batch_a():
    """three problems at pitch 256: 256 rows with 30 % outliers, 200 rows under a skip mask, the 0.5 m baseline"""
    a = tc.problem(1, PITCH, "forward", 2.5, 0.3, 0.3)
    b = tc.problem(2, 200, "forward", 5.0, 0.1, 0.2, pitch=PITCH)
    c = tc.problem(3, PITCH, "forward", 0.5, 0.1, 0.0)
    xy0, xy1 = np.stack([a[0], b[0], c[0]]), np.stack([a[1], b[1], c[1]])
    counts = np.array([PITCH, 200, PITCH], np.int32)
    skip = np.zeros((3, PITCH), np.uint8)
    skip[1, ::7] = 1
    skip[1, 190:] = 3
    Tcw0 = np.stack([tc.tcw0(), np.eye(4, dtype=np.float32), tc.tcw0()])
    return xy0, xy1, counts, skip, Tcw0


@pytest.mark.parametrize("hyp,refit", [(64, 0), (64, 1), (256, 0), (256, 1)])
def test_batch_matches_the_definition(ctx, batch_a, hyp, refit):
    xy0, xy1, counts, skip, Tcw0 = batch_a
    prm = tv.params(hypotheses=hyp, refit=refit, seed=SEED, baseline=2.5)
    ref = tv.two_view_batch(tc.K, xy0, xy1, counts, skip, None, None, Tcw0, prm)
    got = _run(ctx, xy0, xy1, counts, skip, None, None, Tcw0, hypotheses=hyp, refit=refit, seed=SEED, baseline=2.5)
    _check(got, ref)
    assert not got["inlier"][1][skip[1] != 0].any() and not got["inlier"][1, 200:].any()
    assert got["status"][1] == 0 and got["status"][2] == 4
    assert np.array_equal(got["Tcw1"][2], Tcw0[2])                   # a failed problem hands Tcw0 back
    assert (got["points"][2] == SENTINEL).all()                      # and leaves the points alone
    if refit:   # the minimal estimate alone fails the reprojection gate at 0.3 px noise (status 2): the refit is part of the operator
        assert got["status"][0] == 0
        assert (got["point_flags"][0] == 1).sum() == got["tri"][0][got["winner"][0][1]] >= 50


def test_counts_around_the_minimum_identical_points_and_nan_rows(ctx):
    base = tc.problem(4, PITCH, "forward", 2.5, 0.1, 0.0)
    same = tc.problem(5, PITCH, "none", 0.0, 0.0, 0.0)
    nan0, nan1 = base[0].copy(), base[1].copy()
    nan0[5, 0] = np.nan
    nan1[9, 1] = np.inf
    nan1[13] = np.nan
    xy0 = np.stack([base[0], base[0], base[0], same[0], nan0, base[0]])
    xy1 = np.stack([base[1], base[1], base[1], same[1], nan1, base[1]])
    counts = np.array([0, 7, 8, PITCH, PITCH, PITCH + 50], np.int32)
    prm = tv.params(seed=SEED)
    ref = tv.two_view_batch(tc.K, xy0, xy1, counts, None, None, None, None, prm)
    got = _run(ctx, xy0, xy1, counts, seed=SEED)
    _check(got, ref)
    for p in (0, 1, 3):
        assert got["status"][p] == 1 and tuple(got["winner"][p]) == (-1, -1) and got["consensus"][p] == 0
        assert not got["inlier"][p].any() and not got["point_flags"][p].any() and not got["good"][p].any()
        assert np.array_equal(got["Tcw1"][p], np.eye(4, dtype=np.float32))
    assert got["status"][2] != 0
    assert got["status"][4] == 0 and not got["inlier"][4][[5, 9, 13]].any()
    assert got["status"][5] == 0                                     # a count above the pitch is clamped
    for k in ("status", "consensus", "inlier", "Tcw1", "points"):
        assert got[k][5].tobytes() == _run(ctx, xy0[5:], xy1[5:], None, seed=SEED)[k][0].tobytes(), k   # counts null = the pitch


def test_more_rows_than_threads_weights_and_no_tcw0(ctx):
    a = tc.problem(6, 600, "forward", 5.0, 0.1, 0.3, pitch=640)
    xy0, xy1 = a[0][None], a[1][None]
    rng = np.random.default_rng(0)
    w0 = (np.float32(1.2) ** (-2 * rng.integers(0, 4, (1, 640)))).astype(np.float32)
    w1 = (np.float32(1.2) ** (-2 * rng.integers(0, 4, (1, 640)))).astype(np.float32)
    counts = np.array([600], np.int32)
    prm = tv.params(seed=SEED + 1)
    ref = tv.two_view_batch(tc.K, xy0, xy1, counts, None, w0, w1, None, prm)
    got = _run(ctx, xy0, xy1, counts, None, w0, w1, None, seed=SEED + 1)
    _check(got, ref)
    assert got["status"][0] == 0 and got["consensus"][0] > 380 and (got["point_flags"][0] == 1).sum() >= 50
    assert not got["inlier"][0, 600:].any()


def test_a_problem_alone_and_inside_a_batch_and_twice(ctx, batch_a):
    xy0, xy1, counts, skip, Tcw0 = batch_a
    alone = _run(ctx, xy0[1:2], xy1[1:2], counts[1:2], skip[1:2], None, None, Tcw0[1:2], seed=SEED)
    inside = _run(ctx, xy0, xy1, counts, skip, None, None, Tcw0, seed=SEED)
    again = _run(ctx, xy0[1:2], xy1[1:2], counts[1:2], skip[1:2], None, None, Tcw0[1:2], seed=SEED)
    for k in alone:
        assert alone[k][0].tobytes() == inside[k][1].tobytes() == again[k][0].tobytes(), k


def test_host_form_equals_the_batched_one(ctx, batch_a):
    xy0, xy1, counts, skip, Tcw0 = batch_a
    prm = tv.params(seed=SEED, baseline=2.5)
    for p in (0, 1, 2):
        n = int(counts[p])
        r = tv.two_view(tc.K, xy0[p, :n], xy1[p, :n], n, skip[p, :n], None, None, Tcw0[p], prm)
        h = ctx.two_view(xy0[p, :n], xy1[p, :n], tc.K, skip=skip[p, :n], Tcw0=Tcw0[p], seed=SEED, baseline=2.5)
        assert h["status"] == r["status"] and h["winner"] == r["winner"] and h["consensus"] == r["consensus"], p
        assert np.array_equal(h["good"], r["good"]) and np.array_equal(h["tri"], r["tri"]), p
        assert np.array_equal(h["inlier"], r["inlier"]) and np.array_equal(h["point_flags"], r["point_flags"]), p
        assert np.array_equal(h["Tcw1"].view(np.uint32), r["Tcw1"].view(np.uint32)), p
        assert np.array_equal(h["points"].view(np.uint32), r["points"].view(np.uint32)), p
    assert ctx.two_view(xy0[0, :0], xy1[0, :0], tc.K)["status"] == 1


def test_nullable_outputs_and_argument_checks(ctx, batch_a):
    xy0, xy1, counts, _, _ = batch_a
    a, b, c = _dev(xy0, np.float32), _dev(xy1, np.float32), _dev(counts, np.int32)
    A, B, Cn = a.data_ptr(), b.data_ptr(), c.data_ptr()
    assert ctx.two_view_dev(3, A, B, Cn, PITCH, tc.K) == capi.TB_OK       # every output null
    ctx.synchronize()
    assert ctx.two_view_dev(1, 0, B, Cn, PITCH, tc.K) == capi.TB_EINVAL
    assert ctx.two_view_dev(1, A, 0, Cn, PITCH, tc.K) == capi.TB_EINVAL
    assert ctx.two_view_dev(1, A, B, Cn, 0, tc.K) == capi.TB_EINVAL
    assert ctx.two_view_dev(-1, A, B, Cn, PITCH, tc.K) == capi.TB_EINVAL
    for bad in (dict(hypotheses=0), dict(hypotheses=1025), dict(chi2_epi=float("nan")), dict(chi2_epi=-1.0), dict(chi2_max=-1.0),
                dict(cos_parallax_max=float("inf")), dict(min_good_ratio=0.0), dict(min_good_ratio=1.5), dict(ambiguity_ratio=0.0),
                dict(ambiguity_ratio=float("nan")), dict(min_points=-1), dict(baseline=0.0), dict(baseline=float("inf"))):
        assert ctx.two_view_dev(1, A, B, Cn, PITCH, tc.K, **bad) == capi.TB_EINVAL, bad
    assert ctx.two_view_dev(1, A, B, Cn, PITCH, (0.0, 360.0, 320.0, 120.0)) == capi.TB_EINVAL
    assert ctx.two_view_dev(65536, A, B, Cn, PITCH, tc.K) == capi.TB_EUNSUPPORTED
    assert ctx.two_view_dev(1, A, B, Cn, capi.TB_TWO_VIEW_MAX_PITCH + 1, tc.K) == capi.TB_EUNSUPPORTED
    assert ctx.two_view_dev(0, A, B, Cn, PITCH, tc.K) == capi.TB_OK
