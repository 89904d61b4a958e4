"""GPU tests of tb_linear_triangle_batch_dev / tb_linear_triangle against the definition in tests/triangulate_reference.py on
the constructed cases of tests/triangulate_cases.py: npairs = 3, pitch = 256, counts = (0, 65, 200) -- an empty pair, a partial
wavefront, a tail across a wavefront boundary --, a skip mask, poses away from the identity, every gate. Points bit for bit."""
import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi

import triangulate_cases as tc
import triangulate_reference as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    c = tc.build()
    rng = np.random.default_rng(3)
    c["s0"] = rng.choice(np.array([1.0, 0.64, 0.4096], np.float32), (tc.NPAIRS, tc.PITCH))
    c["s1"] = rng.choice(np.array([1.0, 0.64, 0.4096], np.float32), (tc.NPAIRS, tc.PITCH))
    return c


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_batch(ctx, c, counts, s0, s1, skip, K=tc.K, **prm):
    d = {k: _dev(c[k]) for k in ("xy0", "xy1", "Tcw0", "Tcw1")}
    opt = [None if a is None else _dev(a) for a in (counts, s0, s1, skip)]
    pts = torch.full((tc.NPAIRS, tc.PITCH, 3), -7.0, dtype=torch.float32, device="cuda")
    flags = torch.full((tc.NPAIRS, tc.PITCH), 99, dtype=torch.uint8, device="cuda")
    tally = torch.full((tc.NPAIRS, 6), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    q = lambda t: 0 if t is None else t.data_ptr()
    rc = ctx.linear_triangle_batch_dev(tc.NPAIRS, q(d["xy0"]), q(d["xy1"]), q(opt[0]), tc.PITCH, q(d["Tcw0"]), q(d["Tcw1"]), K,
                                       q(opt[1]), q(opt[2]), q(opt[3]), q(pts), q(flags), q(tally), **prm)
    ctx.check(rc)
    ctx.synchronize()
    return pts.cpu().numpy(), flags.cpu().numpy(), tally.cpu().numpy()


def _check(got, exp):
    pts, flags, tally = got
    epts, eflags, etally = exp
    assert np.array_equal(flags, eflags)
    assert np.array_equal(tally, etally)
    ok = eflags == tr.ACCEPTED
    assert np.array_equal(pts[ok].view(np.uint32), epts[ok].view(np.uint32))
    assert (pts[~ok] == -7.0).all()   # written only where accepted


def test_batch_matches_the_definition(ctx, cases):
    c = cases
    exp = tr.triangulate_batch(c["xy0"], c["xy1"], c["counts"], c["Tcw0"], c["Tcw1"], tc.K, skip=c["skip"])
    got = _run_batch(ctx, c, c["counts"], None, None, c["skip"])
    _check(got, exp)
    s = c["slots"]
    for p in (1, 2):
        assert [got[1][p, s[k]] for k in ("nonfinite", "depth", "parallax", "reprojection")] == [2, 3, 4, 5]
    assert got[2][1, 1] > 30 and got[2][2, 1] > 100


def test_batch_with_sigmas_without_counts_and_skip(ctx, cases):
    c = cases
    exp = tr.triangulate_batch(c["xy0"], c["xy1"], None, c["Tcw0"], c["Tcw1"], tc.K, c["s0"], c["s1"], None, 0.9999, 3.0)
    got = _run_batch(ctx, c, None, c["s0"], c["s1"], None, cos_parallax_max=0.9999, chi2_max=3.0)
    _check(got, exp)
    assert (got[1] > 0).all() and (got[2][:, 0] == 0).all()


def test_identical_poses(ctx):
    a, b, T0, T1 = tc.identical_pair()
    ef, _, _ = tr.triangulate_points(a, b, T0, T1, tc.K)
    pts, flags, tally = ctx.linear_triangle(a, b, T0, T1, tc.K)
    assert np.array_equal(flags, ef) and not (flags == tr.ACCEPTED).any() and (pts == 0).all()
    assert np.array_equal(tally, np.bincount(ef, minlength=6))


def test_host_form_equals_the_batched_one(ctx, cases):
    c = cases
    bp, bf, bt = _run_batch(ctx, c, c["counts"], c["s0"], c["s1"], c["skip"])
    for p in range(tc.NPAIRS):
        n = int(c["counts"][p])
        pts, flags, tally = ctx.linear_triangle(c["xy0"][p, :n], c["xy1"][p, :n], c["Tcw0"][p], c["Tcw1"][p], tc.K, c["s0"][p, :n],
                                                c["s1"][p, :n], c["skip"][p, :n])
        assert np.array_equal(flags, bf[p, :n])
        ok = flags == tr.ACCEPTED
        assert np.array_equal(pts[ok].view(np.uint32), bp[p, :n][ok].view(np.uint32)) and (pts[~ok] == 0).all()
        assert np.array_equal(tally[1:], bt[p, 1:]) and tally[0] == (flags == 0).sum()


def test_argument_checks(ctx):
    z = torch.zeros(64, dtype=torch.float32, device="cuda").data_ptr()
    assert ctx.linear_triangle_batch_dev(1, 0, z, 0, 4, z, z, tc.K, 0, 0, 0, z, z, z) == capi.TB_EINVAL
    assert ctx.linear_triangle_batch_dev(1, z, z, 0, 0, z, z, tc.K, 0, 0, 0, z, z, z) == capi.TB_EINVAL
    assert ctx.linear_triangle_batch_dev(1, z, z, 0, 4, z, z, (0.0, 1.0, 0.0, 0.0), 0, 0, 0, z, z, z) == capi.TB_EINVAL
    assert ctx.linear_triangle_batch_dev(1, z, z, 0, 4, z, z, tc.K, 0, 0, 0, z, z, z, chi2_max=float("nan")) == capi.TB_EINVAL
    assert ctx.linear_triangle_batch_dev(0, z, z, 0, 4, z, z, tc.K, 0, 0, 0, z, z, z) == capi.TB_OK
