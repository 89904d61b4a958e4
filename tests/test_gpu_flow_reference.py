"""GPU tests (pytest -m gpu) of the optical-flow and stereo path against references outside the oracle, and on strided inputs.

1. k_pyr_down / k_lk_track against pyramidal Lucas-Kanade in float64 from the method's definition (tests/lk_reference.py): the
   two assertions and the recorded values of tests/test_lk_reference.py, applied to the kernels directly.
2. The C ABI's tracks, stereo depths, pose and VO keyframe against the reference's disparity fixture and KITTI's calibration: the
   statistics and bounds of tests/stereo_fixture.py (tests/test_oracle_disparity.py applies them to the oracle).
3. Every flow / CLAHE / stereo / VO entry point on images with a row stride above the width and an image pitch above stride * h,
   padding bytes 255: bit for bit what the same call gives on tight images (which tests/test_gpu_flow.py and tests/test_gpu_vo.py
   pin to the oracle).

Only tests/golden/ is read."""
import ctypes as C

import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import StereoVO

import lk_reference
import stereo_fixture as sf

pytestmark = pytest.mark.gpu

W, H = sf.CROP_W, sf.CROP_H
STRIDES = (336, 341)          # a multiple of 16, and an odd one


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def _camera(K, w, h):
    c = np.zeros(1, capi.CAMERA)
    c["fx"], c["fy"], c["cx"], c["cy"], c["width"], c["height"] = K[0], K[1], K[2], K[3], w, h
    return c


# ---- 1. the kernels against float64 Lucas-Kanade

@pytest.mark.parametrize("name", sorted(lk_reference.CASES))
def test_lk_against_float64_definition(ctx, name):
    a, b, pts = lk_reference.inputs(name, ctx)
    nxt, st, _, top = ctx.optical_flow_pyr_lk(a, b, pts)
    assert top == 3
    lk_reference.check(name, a, b, pts, nxt, st)


def test_lk_batch_against_float64_definition(ctx):
    """One batched call: L -> R and R -> L of the full pair, 150 and 140 points in slots of 150."""
    cases = [("full_LR",) + lk_reference.inputs("full_LR", ctx), ("full_RL",) + lk_reference.inputs("full_RL", ctx)]
    cap = max(len(c[3]) for c in cases)
    counts = np.array([len(c[3]) for c in cases], np.int32)
    assert counts[0] != counts[1]
    pts = np.zeros((2, cap, 2), np.float32)
    for i, c in enumerate(cases):
        pts[i, :counts[i]] = c[3]
    out, st, _ = _lk_batch(ctx, [c[1] for c in cases], [c[2] for c in cases], sf.W, sf.W * sf.H, pts, counts)
    for i, (name, a, b, p) in enumerate(cases):
        lk_reference.check(name, a, b, p, out[i, :counts[i]], st[i, :counts[i]])


# ---- 2. the disparity fixture and KITTI's calibration

@pytest.fixture(scope="module")
def scene(ctx):
    L, R = sf.pair()
    keys = sf.level0_keys(ctx, L)
    nxt, st, _, _ = ctx.optical_flow_pyr_lk(L, R, keys)
    return dict(L=L, R=R, D=sf.disparity(), keys=keys, nxt=nxt, st=st, cam=_camera(sf.K, sf.W, sf.H))


def test_lk_disparity(scene):
    """x - x' of the L -> R tracks against the fixture. Measured (oracle = kernels): 291 of 298 keys, median |error| 0.5425 px,
    83.5 % within 2 px, median |dy| 0.3746 px."""
    assert len(scene["keys"]) == 298
    sf.check_lk_disparity(sf.lk_disparity_stats(scene["D"], scene["keys"], scene["nxt"], scene["st"]))


def test_stereo_depths_host_and_batch(ctx, scene):
    """tb_add_map_points_by_stereo and its batched device form (the pair at slots 0 and 2, a shortened key list in between)
    against bf / d. Measured: 158 depths, median relative error 3.18 %, 82.3 % within 10 %."""
    L, R, D, keys, cam = (scene[k] for k in ("L", "R", "D", "keys", "cam"))
    depth, nd = ctx.add_map_points_by_stereo(R, L, cam, keys, sf.BF)
    sf.check_depths(sf.stereo_depth_stats(D, keys, depth))
    assert nd == int((depth > 0).sum())
    P = len(keys)
    kk = np.zeros((3, P, 2), np.float32)
    kk[:] = keys
    counts = np.array([P, 40, P], np.int32)
    cur, st, dep = _stereo_batch(ctx, [R, R, R], [L, L, L], sf.W, sf.W * sf.H, cam, kk, counts, sf.W, sf.H)
    for slot in (0, 2):
        assert np.array_equal(dep[slot].view(np.uint32), depth.view(np.uint32)), slot
        sf.check_depths(sf.stereo_depth_stats(D, keys, dep[slot]))
    assert (dep[1, 40:] == -1).all() and (dep[1, :40] > 0).any()


def test_pose_opt_recovers_the_stereo_baseline(ctx, scene):
    """k_pose on rows whose true answer comes from outside the project: the left keys at the fixture's depth, observed at their LK
    tracks in the right image; from the identity the pose must come back as t = (-b, 0, 0), b = bf / fx of KITTI's calibration.
    Measured: 289 rows, 240 inliers, |t - t0| = 5.45 mm, rotation 0.0442 deg."""
    rows = sf.baseline_rows(scene["D"], scene["keys"], scene["nxt"], scene["st"])
    assert len(rows) >= 250
    n, T, _, _ = ctx.pose_opt(sf.K, np.eye(4, dtype=np.float32), rows)
    sf.check_baseline(sf.baseline_stats(T, n, len(rows)))


def test_vo_keyframe_and_baseline_step(ctx, scene):
    """The VO loop's keyframe block: Z of the map points spawned at Tcw = I against bf / d (measured on tests/vo_reference.py: 502
    keys, 239 valid, median relative error 3.10 %, 86.6 % within 10 %). Then the right image as the next left frame: the pose must
    come back as t = (-b, 0, 0) (measured (-0.54184, 0.01457, 0.01154), 236 inliers of 239 rows). The second step's map points
    were made from the same L -> R tracks, so it pins k_vo_kf_spawn, the row builder and k_pose inside the loop to the
    calibration; it does not pin the tracker."""
    L, R, D = scene["L"], scene["R"], scene["D"]
    vo = StereoVO(1, target=500, bf=sf.BF, context=ctx)
    try:
        vo.reset(np.eye(4, dtype=np.float32)[None])
        vo.step(_dev(L[None]), _dev(R[None]))
        xy, kc = vo.keys()
        mp, mv = vo.map_points()
        n = int(kc.cpu().numpy()[0])
        keys, mp, mv = xy.cpu().numpy()[0, :n], mp.cpu().numpy()[0, :n], mv.cpu().numpy()[0, :n] > 0
        assert n >= 400
        sf.check_depths(sf.stereo_depth_stats(D, keys, np.where(mv, mp[:, 2], -1.0)), sf.VO_MEDIAN_REL, sf.VO_WITHIN_10PCT, 180)
        vo.step(_dev(R[None]))
        rows = int(vo.obs()[1].cpu().numpy()[0])
        sf.check_baseline(sf.baseline_stats(vo.Tcw().cpu().numpy()[0], int(vo.n_inliers().cpu().numpy()[0]), rows),
                          sf.VO_T_ERR_M, sf.VO_ROT_DEG)
    finally:
        vo.close()
        torch.cuda.synchronize()
        ctx.set_stream(None)      # back on the context's own stream: the loop's stream goes with the loop


# ---- 3. strided and pitched inputs

def _lk_batch(ctx, A, B, stride, pitch, pts, counts):
    h, w = A[0].shape
    n, cap = pts.shape[:2]
    dA, dB, dp, dc = _dev(sf.pitched(A, stride, pitch)), _dev(sf.pitched(B, stride, pitch)), _dev(pts), _dev(counts)
    out = torch.full((n, cap, 2), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n, cap), 9, dtype=torch.uint8, device="cuda")
    er = torch.full((n, cap), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.optical_flow_pyr_lk_batch_dev(n, dA.data_ptr(), dB.data_ptr(), w, h, stride, pitch, dp.data_ptr(), dc.data_ptr(), cap,
                                      out.data_ptr(), st.data_ptr(), er.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()


def _opflow_batch(ctx, F1, F2, stride, pitch, cam, pts, counts):
    h, w = F1[0].shape
    n, cap = pts.shape[:2]
    d1, d2, dp, dc = _dev(sf.pitched(F1, stride, pitch)), _dev(sf.pitched(F2, stride, pitch)), _dev(pts), _dev(counts)
    cur = torch.zeros((n, cap, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, cap, 4), dtype=torch.int32, device="cuda")
    oc = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.search_by_opflow_batch_dev(n, d1.data_ptr(), d2.data_ptr(), w, h, stride, pitch, cam, dp.data_ptr(), dc.data_ptr(), cap,
                                   cur.data_ptr(), st.data_ptr(), out.data_ptr(), cap, oc.data_ptr(), equalized=True, reject=True)
    ctx.synchronize()
    return cur.cpu().numpy(), st.cpu().numpy(), out.cpu().numpy(), oc.cpu().numpy()


def _stereo_batch(ctx, S, Cur, stride, pitch, cam, keys, counts, w, h):
    n, cap = keys.shape[:2]
    d1, d2, dk, dc = _dev(sf.pitched(S, stride, pitch)), _dev(sf.pitched(Cur, stride, pitch)), _dev(keys), _dev(counts)
    cur = torch.zeros((n, cap, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    dep = torch.zeros((n, cap), dtype=torch.float32, device="cuda")
    camr = np.ascontiguousarray(cam, capi.CAMERA)
    torch.cuda.synchronize()
    ctx.check(capi.lib().tb_add_map_points_by_stereo_batch_dev(
        ctx._h, n, _vp(d1), _vp(d2), w, h, int(stride), C.c_size_t(pitch), _np(camr), _vp(dk), _vp(dc), cap, C.c_float(sf.BF),
        _vp(cur), _vp(st), _vp(dep)))
    ctx.synchronize()
    return cur.cpu().numpy(), st.cpu().numpy(), dep.cpu().numpy()


@pytest.fixture(scope="module")
def crops(ctx):
    """The 333 x 211 crop of the pair (and a second crop for the VO loop's second sequence), a camera for it, and a batch of two
    point lists: ORB keys of the crop plus points around and beyond its borders, ragged."""
    L, R = sf.pair()
    cl, cr = sf.crop(L), sf.crop(R)
    cl2, cr2 = sf.crop(L, 454, 100), sf.crop(R, 454, 100)
    rng = np.random.default_rng(4)
    edge = np.stack([rng.uniform(-5, W + 5, 90), rng.uniform(-5, H + 5, 90)], 1).astype(np.float32)
    kl = np.concatenate([sf.inner_keys(ctx, cl, 150, margin=0), edge])
    kr = np.concatenate([sf.inner_keys(ctx, cr, 120, margin=0), edge[:50]])
    cap = max(len(kl), len(kr))
    pts = np.zeros((2, cap, 2), np.float32)
    pts[0, :len(kl)] = kl
    pts[1, :len(kr)] = kr
    return dict(cl=cl, cr=cr, cl2=cl2, cr2=cr2, cam=_camera(sf.crop_K(), W, H), pts=pts,
                counts=np.array([len(kl), len(kr)], np.int32))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("stride", STRIDES)
def test_strided_lk_batch(ctx, crops, stride):
    """tb_optical_flow_pyr_lk_batch_dev: L -> R and R -> L of the crop; next points, status and error as bytes."""
    A, B = [crops["cl"], crops["cr"]], [crops["cr"], crops["cl"]]
    tight = _lk_batch(ctx, A, B, W, W * H, crops["pts"], crops["counts"])
    assert tight[1][0, :crops["counts"][0]].sum() > 100 and tight[1][1, :crops["counts"][1]].sum() > 80
    _same(_lk_batch(ctx, A, B, stride, stride * H + 77, crops["pts"], crops["counts"]), tight)


@pytest.mark.parametrize("stride", STRIDES)
def test_strided_search_by_opflow_batch(ctx, crops, stride):
    """tb_search_by_opflow_batch_dev, equalized = 1 (k_clahe_* write an image of the same stride and pitch), reject = 1."""
    F1, F2 = [crops["cr"], crops["cl"]], [crops["cl"], crops["cr"]]
    tight = _opflow_batch(ctx, F1, F2, W, W * H, crops["cam"], crops["pts"], crops["counts"])
    assert tight[3][0] > 50
    _same(_opflow_batch(ctx, F1, F2, stride, stride * H + 77, crops["cam"], crops["pts"], crops["counts"]), tight)


@pytest.mark.parametrize("stride", STRIDES)
def test_strided_stereo_depths_batch(ctx, crops, stride):
    """tb_add_map_points_by_stereo_batch_dev: tracked points, status and depths as bytes."""
    S, Cur = [crops["cr"], crops["cr2"]], [crops["cl"], crops["cl2"]]
    tight = _stereo_batch(ctx, S, Cur, W, W * H, crops["cam"], crops["pts"], crops["counts"], W, H)
    assert (tight[2][0] > 0).sum() > 30
    _same(_stereo_batch(ctx, S, Cur, stride, stride * H + 77, crops["cam"], crops["pts"], crops["counts"], W, H), tight)


@pytest.mark.parametrize("stride", STRIDES)
def test_strided_clahe(ctx, crops, stride):
    """tb_clahe_dev and tb_clahe with dst_stride != stride: the image columns equal the tight call's, the destination's padding
    keeps its sentinel."""
    img = crops["cl"]
    tight = ctx.clahe(img)
    dst_stride, sentinel = stride + 5, 0xA5
    src = sf.strided(img, stride)
    d_src = _dev(src)
    d_dst = torch.full((H, dst_stride), sentinel, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.check(capi.lib().tb_clahe_dev(ctx._h, _vp(d_src), W, H, stride, C.c_double(3.0), 8, 8, _vp(d_dst), dst_stride))
    ctx.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got[:, :W], tight) and (got[:, W:] == sentinel).all()
    host = np.full((H, dst_stride), sentinel, np.uint8)
    ctx.check(capi.lib().tb_clahe(ctx._h, _np(src), W, H, stride, C.c_double(3.0), 8, 8, _np(host), dst_stride))
    assert np.array_equal(host[:, :W], tight) and (host[:, W:] == sentinel).all()


@pytest.mark.parametrize("stride", STRIDES)
def test_strided_lk_host_form(ctx, crops, stride):
    """tb_optical_flow_pyr_lk on strided host arrays."""
    n = int(crops["counts"][0])
    pts = np.ascontiguousarray(crops["pts"][0, :n])
    tight = ctx.optical_flow_pyr_lk(crops["cl"], crops["cr"], pts)
    a, b = sf.strided(crops["cl"], stride), sf.strided(crops["cr"], stride)
    out, st, er, top = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32), C.c_int(-1)
    ctx.check(capi.lib().tb_optical_flow_pyr_lk(ctx._h, _np(a), _np(b), W, H, stride, _np(pts), n, 21, 3, _np(out), _np(st), _np(er),
                                               C.byref(top)))
    assert top.value == tight[3] == 3
    _same((out, st, er), tight[:3])


def _vo_params():
    return capi.VOParams(W, H, 5, 0.8, 300, 80.0, 30.0, (C.c_double * 4)(*sf.crop_K()), sf.BF, 10)


def _vo_state(ctx, vo):
    """The loop's state after a step, cut at the counts, as numpy arrays per sequence."""
    d = vo.state_dev()
    P, S = d["key_pitch"], vo.nseq
    ctx.synchronize()

    def get(key, shape, typestr):
        return torch.as_tensor(capi._DevView(d[key], shape, typestr), device=torch.device("cuda", 0)).cpu().numpy().copy()
    Tcw, kc, oc, ni = get("Tcw", (S, 16), "<f4"), get("key_counts", (S,), "<i4"), get("obs_counts", (S,), "<i4"), get("n_inliers", (S,), "<i4")
    xy, mp, mv = get("keys_xy", (S, P, 2), "<f4"), get("map_points", (S, P, 3), "<f4"), get("mp_valid", (S, P), "|u1")
    obs, outl = get("obs", (S, P, 6), "<f4"), get("outlier", (S, P), "|u1")
    out = [Tcw, kc, oc, ni]
    for s in range(S):
        k, o = int(kc[s]), int(oc[s])
        out += [xy[s, :k], mv[s, :k], mp[s, :k][mv[s, :k] > 0], obs[s, :o], outl[s, :o]]
    return out


def _vo_run(ctx, crops, stride, pitch, ragged):
    """Two frames of a 2-sequence loop: frame 0 is the keyframe on (left, right), frame 1 presents the right images as the next
    left frames. ragged: through tb_vo_step_ragged_dev, frame 1 with a keyframe forced for sequence 1 only."""
    lefts, rights = [crops["cl"], crops["cl2"]], [crops["cr"], crops["cr2"]]
    vo = capi.VO(ctx, _vo_params(), 2)
    try:
        T0 = _dev(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1)))
        torch.cuda.synchronize()
        vo.reset_dev(T0.data_ptr())
        states = []
        for t, (a, b) in enumerate(((lefts, rights), (rights, lefts))):
            da, db = _dev(sf.pitched(a, stride, pitch)), _dev(sf.pitched(b, stride, pitch))
            torch.cuda.synchronize()
            if ragged:
                rc = vo.step_ragged_dev(da.data_ptr(), db.data_ptr(), stride, pitch, None, [False, True] if t else None)
            else:
                rc = vo.step_dev(da.data_ptr(), db.data_ptr() if t == 0 else None, stride, pitch)
            ctx.check(rc)
            states.append(_vo_state(ctx, vo))
        return states
    finally:
        vo.close()


@pytest.mark.parametrize("ragged", [False, True])
def test_strided_vo_steps(ctx, crops, ragged):
    """tb_vo_step_dev / tb_vo_step_ragged_dev through the C ABI (StereoVO.step makes its tensors contiguous): pose, keys, map
    points, valid flags, rows, outlier flags and inlier counts of both frames as bytes, for both strides."""
    tight = _vo_run(ctx, crops, W, W * H, ragged)
    kc, oc, ni = tight[0][1], tight[1][2], tight[1][3]
    assert (kc > 50).all() and oc[0] > 10 and ni[0] > 5, (kc, oc, ni)
    for stride in STRIDES:
        got = _vo_run(ctx, crops, stride, stride * H + 77, ragged)
        for t in range(2):
            _same(got[t], tight[t])


def test_vo_step_refuses_short_stride_or_pitch(ctx, crops):
    """stride < width or pitch < stride * height: TB_EINVAL from both entry points, before anything is launched."""
    vo = capi.VO(ctx, _vo_params(), 2)
    try:
        T0 = _dev(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1)))
        slab = _dev(sf.pitched([crops["cl"], crops["cl2"]], 336, 336 * H + 77))
        torch.cuda.synchronize()
        vo.reset_dev(T0.data_ptr())
        p = slab.data_ptr()
        for stride, pitch in ((W - 1, W * H), (336, 336 * H - 1), (W, (W - 1) * H)):
            assert vo.step_dev(p, p, stride, pitch) == capi.TB_EINVAL, (stride, pitch)
            assert vo.step_ragged_dev(p, p, stride, pitch) == capi.TB_EINVAL, (stride, pitch)
        assert (vo.frames()[0] == -1).all()
        ctx.check(vo.step_dev(p, p, 336, 336 * H + 77))      # the same slab with its true geometry is accepted
        ctx.synchronize()
    finally:
        vo.close()
