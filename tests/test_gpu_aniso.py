"""GPU tests (pytest -m gpu): every entry point that takes a camera, at fx != fy.

Every other camera in the suite has fx == fy, so an fx written where fy belongs (fy occurs a hundred times in csrc/) could not
fail a test. Each operator here runs one or two of its smallest existing shapes, rebuilt at K_ANISO = (718.856, 652.25, 607.1928,
185.2157) (tests/aniso_cases.py), through the C ABI against its existing reference at its existing bar. That each reference
recovers the truth at fx != fy and notices fx and fy exchanged is tests/test_aniso_references.py's business (CPU); the local BA
at fx != fy is tests/test_gpu_ba_weights.py's, which uses K_ANISO throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from trackingbench_slam_amd import capi

import aniso_cases as ac
import gauge_cases as gc
import pnp_reference as pr
import sim3_reference as sr
import triangulate_reference as tr
import two_view_reference as tv
import test_gpu_pnp as gpnp
import test_gpu_projection as gproj
import test_gpu_sim3 as gsim3
import test_gpu_triangulate as gtri
import test_gpu_two_view as gtv
import test_gpu_vo as gvo

pytestmark = pytest.mark.gpu
K = ac.K_ANISO


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _close(a, b, tol=1e-6):
    assert np.allclose(a, b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max()))), float(np.abs(a - b).max())


def test_pose_opt(ctx):
    """tb_pose_opt and tb_pose_opt_batch_dev: n = 9 (below the n < 10 round break) and n = 300 with 15 % outliers, the latter
    also in the y180 gauge; against oracle.pose_opt at 1e-6 with equal outlier flags; the batch equals the single calls bit
    for bit (tests/test_gpu_gauge.py's rule: both entry points run one kernel)"""
    P, pitch = len(ac.POSE), 300
    obs = np.zeros((P, pitch), capi.OBS)
    Tin = np.zeros((P, 16), np.float32)
    alone = []
    for p, (seed, n, gname) in enumerate(ac.POSE):
        _, T, o = ac.pose_case(seed, n, gname)
        assert gc.quat_branch(T) == gc.GAUGE_BRANCH[gname]
        no, To, oo, so = oracle.pose_opt(K, T, o)
        ng, Tg, og, sg = ctx.pose_opt(K, T, o)
        assert ng == no and np.array_equal(og, oo), (seed, n, gname)
        _close(Tg, To)
        assert np.isclose(sg[1], so[1], rtol=1e-6, atol=1e-9)
        obs[p, :n] = o
        Tin[p] = T.reshape(16)
        alone.append((ng, Tg, og))
    dev = torch.device("cuda", 0)
    counts = np.array([n for _, n, _ in ac.POSE], np.int32)
    dObs = torch.from_numpy(obs.view(np.uint8).reshape(P, pitch, capi.OBS.itemsize)).to(dev)
    dTin, dCnt = torch.from_numpy(Tin).to(dev), torch.from_numpy(counts).to(dev)
    dFl = torch.zeros((P, pitch), dtype=torch.uint8, device=dev)
    dTout = torch.full((P, 16), float("nan"), dtype=torch.float32, device=dev)
    dInl = torch.full((P,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    Kd = np.ascontiguousarray(K, np.float64)
    vp = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(capi.lib().tb_pose_opt_batch_dev(ctx._h, P, Kd.ctypes.data_as(C.c_void_p), vp(dTin), vp(dObs), vp(dCnt), pitch, vp(dFl),
                                               vp(dTout), vp(dInl), None))
    ctx.synchronize()
    Tout, inl, fl = dTout.cpu().numpy(), dInl.cpu().numpy(), dFl.cpu().numpy()
    for p, (ng, Tg, og) in enumerate(alone):
        n = int(counts[p])
        assert inl[p] == ng and np.array_equal(fl[p, :n], og) and Tout[p].tobytes() == np.ascontiguousarray(Tg).tobytes(), p


def test_linear_triangle(ctx):
    """tb_linear_triangle_batch_dev on the module's own batch at K_ANISO: flags, tally and accepted points bit for bit"""
    c = ac.triangulate_case()
    exp = tr.triangulate_batch(c["xy0"], c["xy1"], c["counts"], c["Tcw0"], c["Tcw1"], K, skip=c["skip"])
    got = gtri._run_batch(ctx, c, c["counts"], None, None, c["skip"], K=K)
    gtri._check(got, exp)
    assert got[2][1, 1] > 30 and got[2][2, 1] > 100


def test_pnp_ransac(ctx):
    """tb_pnp_ransac_batch_dev: n = 65 and CHUNK + 1 rows, 50 % outliers, 256 hypotheses, at the module's K with K_ANISO's
    ratio: bit for bit, with the margin check"""
    obs = np.stack([ac.pnp_case(i)[0] for i in range(2)])
    counts = np.array(ac.RANSAC_N, np.int32)
    ref = pr.ransac_batch(ac.K_PNP, obs, counts, 256, pr.CHI2_MAX, ac.RANSAC_SEED)
    got = gpnp._run(ctx, obs, counts, seed=ac.RANSAC_SEED, K=ac.K_PNP)
    gpnp._check(got, ref)
    assert (got["consensus"] >= 0.4 * counts).all()


@pytest.mark.parametrize("fixed", [False, True])
def test_sim3_ransac(ctx, fixed):
    """tb_sim3_ransac_batch_dev: n = 65 and CHUNK + 1 rows, scale free and fixed, noise at which the chi2 gate is in use: bit
    for bit, with sr.margin"""
    rows = np.stack([ac.sim3_case(i, fixed)[0] for i in range(2)])
    counts = np.array(ac.RANSAC_N, np.int32)
    ref = sr.ransac_batch(K, rows, counts, hypotheses=256, fixed_scale=fixed, seed=ac.RANSAC_SEED)
    got = gsim3._run(ctx, rows, counts, fixed_scale=fixed, seed=ac.RANSAC_SEED, K=K)
    gsim3._check(got, ref)
    assert (got["flags"] == 0).all() and (got["consensus"] >= 0.2 * counts).all()
    if fixed:
        assert (got["srt"][:, 7] == 1.0).all()


def test_two_view(ctx):
    """tb_two_view_batch_dev: a forward-motion problem that initialises and one that is refused (half a metre of baseline):
    every output bit for bit"""
    cases = [ac.two_view_case("initialises"), ac.two_view_case("refused")]
    xy0, xy1 = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    counts = np.array([256, 256], np.int32)
    ref = tv.two_view_batch(K, xy0, xy1, counts, None, None, None, None, tv.params(seed=ac.TWO_VIEW_SEED))
    got = gtv._run(ctx, xy0, xy1, counts, K=K, seed=ac.TWO_VIEW_SEED)
    gtv._check(got, ref)
    assert got["status"][0] == tv.OK and got["status"][1] == tv.FEW_POINTS


def test_search_by_projection_both_overloads(ctx):
    """the CAMERA record at fx != fy: match lists exact"""
    c = ac.projection_case(1)
    tail = (c["k2"], c["mp"], c["mp_desc"], c["sf"], 8.0)
    mo = oracle.search_by_projection(*ac.projection_args(c), *tail)
    assert len(mo) > 100
    gproj._same(ctx.search_by_projection(*ac.projection_args(c), *tail), mo)
    c = dict(ac.projection_case(2))
    c["k1"] = c["k1"].copy()
    c["k1"]["octave"][::2] = 0
    tail = (c["mp"], c["mp_desc"], c["sf"], 3.0, 0.8)
    mo = oracle.search_by_projection_map(*ac.projection_args(c), *tail)
    assert len(mo) > 50
    gproj._same(ctx.search_by_projection_map(*ac.projection_args(c), *tail), mo)


@pytest.mark.parametrize("seed,w,h,n", ac.FLOW_PAIRS)
def test_stereo_depths_and_opflow(ctx, seed, w, h, n):
    """LocalBA::AddMapPointsByStereo and Matcher::searchByOPFlow with a camera whose fy differs from fx: exact. The stage's
    definition reads the image size alone (test_stereo_depth_is_the_definition_and_ignores_the_focal_lengths), so what this
    pins is that the kernels do not read a focal length either."""
    L, R, cam, keys = ac.flow_case(seed, w, h, n)
    ocur, oidx = oracle.search_by_opflow(R, L, cam, keys, equalized=True, reject=True)
    cur, m = ctx.search_by_opflow(R, L, cam, keys, equalized=True, reject=True)
    assert np.array_equal(cur.view(np.uint32), ocur.view(np.uint32))
    assert len(oidx) >= 5 and np.array_equal(m["queryIdx"], oidx) and np.array_equal(m["trainIdx"], oidx)
    odepth = oracle.add_map_points_by_stereo(R, L, cam, keys, ac.FLOW_BF)
    depth, nd = ctx.add_map_points_by_stereo(R, L, cam, keys, ac.FLOW_BF)
    assert nd == len(oidx) and np.array_equal(depth.view(np.uint32), odepth.view(np.uint32))


def test_vo_loop(ctx):
    """the optical-flow VO loop on two 5-frame sequences rendered at K_ANISO, a keyframe every third frame: every step against
    tests/vo_reference.py through test_gpu_vo._step_parity (keys, map points and observation rows bit for bit, the pose at
    1e-6) -- the back-projection of new map points and the pose solver inside the loop both see fx != fy"""
    gvo._step_parity(ac.vo_sequences(), ac.VO_FRAMES, ac.VO_KEYFRAME_EVERY, K=K)
