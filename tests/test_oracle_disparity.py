"""The oracle's flow / stereo / pose path against numbers that do not come from this project: the reference's disparity fixture
(tests/golden/kitti00_disparity_1241x376.pgm.gz) and KITTI's calibration (tests/stereo_fixture.py, where every statistic is written
once). tests/test_gpu_flow_reference.py applies the same statistics and bounds to the C ABI's output.

Each bound is the oracle's own value, measured when the test was written, rounded away from it to the next 0.05 px or 5 percentage
points; the pose bounds are twice the measured error (room for a legitimate change of which rows are kept). The fixture is
quantised to 1 px, so the median LK disparity error is also held to 1 px whatever was measured."""
import hashlib

import numpy as np
import pytest

import oracle

import stereo_fixture as sf
import vo_reference as vr


@pytest.fixture(scope="module")
def scene():
    L, R = sf.pair()
    D = sf.disparity()
    keys = sf.level0_keys(oracle, L)
    nxt, st, _, _ = oracle.optical_flow_pyr_lk(L, R, keys)
    return dict(L=L, R=R, D=D, keys=keys, nxt=nxt, st=st, cam=oracle.camera(*sf.K, sf.W, sf.H))


def test_disparity_fixture_is_the_reference_image():
    D = sf.disparity()
    assert D.shape == (sf.H, sf.W) and D.min() == 1 and D.max() == 120
    # pixel SHA-1 of the reference's data/disparity.png (tools/gen_golden.py says how the PGM was made)
    assert hashlib.sha1(D.tobytes()).hexdigest() == "8d6e423f9008b59f9d9b9dbb75d37887a192a6ed"
    assert abs(sf.BASELINE - 0.53717) < 1e-5


def test_lk_disparity(scene):
    """L -> R tracks of the 298 level-0 keys: x - x' against the fixture. Measured: 291 keys, median |error| 0.5425 px, 83.5 %
    within 2 px, median |dy| 0.3746 px."""
    assert len(scene["keys"]) == 298
    sf.check_lk_disparity(sf.lk_disparity_stats(scene["D"], scene["keys"], scene["nxt"], scene["st"]))


def test_stereo_depths(scene):
    """AddMapPointsByStereo's depths against bf / d. Measured: 158 depths, median relative error 3.18 %, 82.3 % within 10 %."""
    depth = oracle.add_map_points_by_stereo(scene["R"], scene["L"], scene["cam"], scene["keys"], sf.BF)
    sf.check_depths(sf.stereo_depth_stats(scene["D"], scene["keys"], depth))


def test_pose_opt_recovers_the_stereo_baseline(scene):
    """Rows: the left keys at the fixture's depth (Tcw = I), observed at their LK tracks in the right image. PoseOptimization from
    the identity must find the right camera: t = (-b, 0, 0) with b = bf / fx from KITTI's calibration, R = I. The one check
    where the pose solver's true answer comes from outside the project. Measured: 289 rows, 240 inliers,
    t = (-0.54025, 0.00224, 0.00389) (|t - t0| = 5.45 mm), rotation 0.0442 deg."""
    rows = sf.baseline_rows(scene["D"], scene["keys"], scene["nxt"], scene["st"])
    assert len(rows) >= 250
    n, T, _, _ = oracle.pose_opt(sf.K, np.eye(4, dtype=np.float32), rows)
    sf.check_baseline(sf.baseline_stats(T, n, len(rows)))


def test_vo_keyframe_and_baseline_step():
    """The VO loop's keyframe block (tests/vo_reference.py, target 500, bf from the calibration): the depths Z of the map points
    it spawns at Tcw = I against bf / d. Measured: 502 keys, 239 valid, median relative error 3.10 %, 86.6 % within 10 %.

    Then the right image is presented as the next left frame: the pose must come back as t = (-b, 0, 0). Measured:
    (-0.54184, 0.01457, 0.01154), 236 inliers of 239 rows. The map points of that step were made from the same L -> R tracks the
    step then repeats (with CLAHE on the other side), so it pins spawn_points, the row builder and the pose solver inside the loop
    to the calibration; it does not pin the tracker (test_lk_disparity and tests/test_lk_reference.py do)."""
    L, R = sf.pair()
    D = sf.disparity()
    P = vr.Params(target=500, bf=sf.BF)
    s, _ = vr.step(vr.initial_state(np.eye(4, dtype=np.float32)), L, R, P)
    assert len(s["keys"]) >= 400
    Z = np.where(s["valid"], s["mp"][:, 2], -1.0)
    sf.check_depths(sf.stereo_depth_stats(D, s["keys"], Z), sf.VO_MEDIAN_REL, sf.VO_WITHIN_10PCT, 180)
    s2, info = vr.step(s, R, None, P)
    sf.check_baseline(sf.baseline_stats(s2["Tcw"], info["n_inliers"], len(info["obs"])), sf.VO_T_ERR_M, sf.VO_ROT_DEG)
