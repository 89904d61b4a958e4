"""CPU test of the VO composition with the searchByNN tracker (tests/vo_lsh_reference.py): 640 x 240, 600 keys, seeds 0 and 1 of
the slow synthetic drive (0.1 m / frame), 7 frames, a keyframe every 3. The structural facts are asserted; matches / rows /
inliers per frame are printed beside the searchByBF tracker's on the same frames (DESIGN.md quotes them)."""
import numpy as np
import pytest

from trackingbench_slam_amd import synth_seq

import vo_desc_reference as vd
import vo_lsh_reference as vl

W, H, K, TARGET, EVERY, T = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 3, 7
SEEDS = (0, 1)


@pytest.fixture(scope="module")
def runs():
    P = vl.Params(width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY)
    out = {}
    for seed in SEEDS:
        L, R, G = synth_seq.sequence(seed, T, width=W, height=H, K=K, speed=0.1)
        out[seed] = (vl.run(L, R, G[0], P, vl.Tracker()), vd.run(L, R, G[0], P, vd.Tracker("bf")))
    return out


def test_structure_of_every_frame(runs):
    tracked = 0
    for seed, ((states, infos), (bstates, binfos)) in runs.items():
        for t in range(T):
            s, i, b = states[t], infos[t], binfos[t]
            print("seed %d frame %d%s: lsh %3d matches %3d rows %3d inliers | bf %3d matches %3d rows %3d inliers" % (
                seed, t, " kf" if i["keyframe"] else "   ", len(i["matches"]), len(i["obs"]), i["n_inliers"], len(b["matches"]),
                len(b["obs"]), b["n_inliers"]))
            m = i["matches"]
            assert i["keyframe"] == (t % EVERY == 0)
            if t == 0:
                assert len(m) == 0 and len(i["obs"]) == 0 and s["kf"]["frame"] == 0
                continue
            prev = states[t - 1]
            kf = prev["kf"]
            # each queryIdx at most once, ascending; indices inside the two frames
            assert (np.diff(m["queryIdx"]) > 0).all()
            assert len(m) == 0 or (m["queryIdx"].max() < len(s["orb"]) and m["trainIdx"].max() < len(kf["orb"]) and m["trainIdx"].min() >= 0)
            assert (m["distance"] < 30).all()
            # rows only through keyframe entries with a map point: one row per such match, in key order
            through = m[kf["valid"][m["trainIdx"]]]
            assert len(i["obs"]) == len(through)
            assert np.array_equal(i["obs"]["u"], s["orb"]["x"][through["queryIdx"]])
            assert np.array_equal(np.stack([i["obs"][k] for k in "XYZ"], -1), kf["mp"][through["trainIdx"]])
            if len(i["obs"]) < 3:     # fewer than 3 rows hold the pose
                assert i["n_inliers"] == 0
                assert np.array_equal(s["Tcw"].view(np.uint32), np.asarray(prev["Tcw"], np.float32).view(np.uint32))
            else:
                tracked += 1
            if not i["keyframe"]:     # the frame carries exactly the matched points
                assert s["valid"].sum() == len(through) and s["kf"]["frame"] == kf["frame"]
    assert tracked >= 1, "some frame tracks with at least 3 rows"


def test_tracker_defaults_and_explicit_bits():
    tr = vl.Tracker()
    assert (tr.ratio, tr.min_th, tr.min_level, tr.max_level, tr.multi_probe_level) == (10.0, 30.0, 0, 5, 2) and tr.bits.shape == (20, 10)
    assert np.array_equal(vl.Tracker(bits=tr.bits, seed=5).bits, tr.bits)
    assert not np.array_equal(vl.Tracker(seed=5).bits, tr.bits)
