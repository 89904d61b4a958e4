"""The reference's disparity fixture (data/disparity.png -> tests/golden/kitti00_disparity_1241x376.pgm.gz) with KITTI's calibration,
and the statistics the flow / stereo / pose path is held to against them. Every statistic is written once here; the CPU tests
(tests/test_oracle_disparity.py) feed it the oracle's output, the GPU tests (tests/test_gpu_flow_reference.py) the C ABI's.

The disparity image is aligned with the left image: pixel (v, u) is the disparity, in whole pixels (1..120, none zero), of left
pixel (u, v). The reference's test_projection.cpp reads it as depth = fx * baseline / disparity. Neither the image nor the
calibration comes from this project, which is what makes them a yardstick for it.

The file is a binary P5 PGM in the layout of the two image fixtures next to it, gzip-wrapped: its pixels hold no zero byte, so
git would take the plain file for text and show it as 5800 lines of diff.
"""
import gzip
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

W, H = 1241, 376
FX = FY = 718.856
CX, CY = 607.1928, 185.2157
K = (FX, FY, CX, CY)
BF = 386.1448
BASELINE = BF / FX          # 0.53717 m

OBS = np.dtype([("u", "<f4"), ("v", "<f4"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("inv_sigma2", "<f4")])

# the 333 x 211 crop of the pair the float64 LK tests and the stride tests use: pyramid levels 167x106, 84x53, 42x27
CROP_X, CROP_Y, CROP_W, CROP_H = 300, 150, 333, 211


def read_pgm(path):
    """Binary P5, maxval 255 (gzip-wrapped when the name ends in .gz); numpy and the standard library only."""
    with (io.BytesIO(gzip.open(path, "rb").read()) if path.endswith(".gz") else open(path, "rb")) as f:
        assert f.readline().strip() == b"P5"
        w, h = map(int, f.readline().split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(), np.uint8).reshape(h, w).copy()


def pair():
    return read_pgm(os.path.join(GOLDEN, "kitti00_left_1241x376.pgm")), read_pgm(os.path.join(GOLDEN, "kitti00_right_1241x376.pgm"))


def disparity():
    return read_pgm(os.path.join(GOLDEN, "kitti00_disparity_1241x376.pgm.gz"))


def crop(img, x=CROP_X, y=CROP_Y):
    return np.ascontiguousarray(img[y:y + CROP_H, x:x + CROP_W])


def crop_K(x=CROP_X, y=CROP_Y):
    """The calibration of a crop: the principal point moves with the origin."""
    return (FX, FY, CX - x, CY - y)


def level0_keys(backend, img, nlevels=5, target=1000):
    """[n, 2] float32 (x, y) of the level-0 ORB keys of img; backend = the oracle module or a capi.Context (same calls)."""
    lv, sf = backend.pyramid(img, nlevels, 0.8)
    k, _, _ = backend.orb_extract(lv, sf, target, 80, 30)
    return np.ascontiguousarray(np.stack([k["x"], k["y"]], 1)[k["octave"] == 0], np.float32)


def inner_keys(backend, img, count, margin=30, nlevels=8, target=2000):
    """About `count` ORB keys (all levels, evenly thinned in extraction order) at least `margin` px from every border."""
    lv, sf = backend.pyramid(img, nlevels, 0.8)
    k, _, _ = backend.orb_extract(lv, sf, target, 80, 30)
    h, w = img.shape
    ok = (k["x"] >= margin) & (k["x"] <= w - 1 - margin) & (k["y"] >= margin) & (k["y"] <= h - 1 - margin)
    xy = np.unique(np.stack([k["x"], k["y"]], 1)[ok].astype(np.float32), axis=0)
    return np.ascontiguousarray(xy[:: max(1, len(xy) // count)][:count])


def at_keys(disp, keys):
    """The fixture's value at the rounded key, as float64."""
    u = np.clip(np.rint(keys[:, 0]).astype(int), 0, disp.shape[1] - 1)
    v = np.clip(np.rint(keys[:, 1]).astype(int), 0, disp.shape[0] - 1)
    return disp[v, u].astype(np.float64)


def in_frame(pts, w=W, h=H):
    return (pts[:, 0] >= 0) & (pts[:, 0] < w) & (pts[:, 1] >= 0) & (pts[:, 1] < h)


def lk_disparity_stats(disp, keys, nxt, status):
    """L -> R tracks against the fixture: dict(n, median_err px, within_2px share, median_dy px) over the keys with status 1 and
    the tracked point inside the frame."""
    nxt = np.asarray(nxt, np.float64)
    sel = (np.asarray(status) > 0) & in_frame(nxt)
    err = np.abs((keys[sel, 0].astype(np.float64) - nxt[sel, 0]) - at_keys(disp, keys[sel]))
    dy = np.abs(nxt[sel, 1] - keys[sel, 1])
    return dict(n=int(sel.sum()), median_err=float(np.median(err)), within_2px=float((err <= 2.0).mean()),
                median_dy=float(np.median(dy)))


def stereo_depth_stats(disp, keys, depth):
    """Depths (> 0 = made) against bf / d: dict(n, median_rel, within_10pct share)."""
    depth = np.asarray(depth, np.float64)
    sel = depth > 0
    ref = BF / at_keys(disp, keys[sel])
    rel = np.abs(depth[sel] - ref) / ref
    return dict(n=int(sel.sum()), median_rel=float(np.median(rel)), within_10pct=float((rel <= 0.10).mean()))


def baseline_rows(disp, keys, nxt, status):
    """Pose-optimisation rows whose true answer is the stereo baseline: the left key back-projected (Tcw = I) at the fixture's
    depth, observed at its LK track in the right image. Keys with fixture >= 2 and the track inside the frame."""
    nxt = np.asarray(nxt, np.float32)
    d = at_keys(disp, keys)
    sel = (np.asarray(status) > 0) & in_frame(nxt) & (d >= 2)
    z = BF / d[sel]
    rows = np.zeros(int(sel.sum()), OBS)
    rows["u"], rows["v"] = nxt[sel, 0], nxt[sel, 1]
    rows["X"] = (keys[sel, 0].astype(np.float64) - CX) / FX * z
    rows["Y"] = (keys[sel, 1].astype(np.float64) - CY) / FY * z
    rows["Z"] = z
    rows["inv_sigma2"] = 1.0
    return rows


def baseline_stats(Tcw, n_inliers=0, n_rows=1):
    """A pose that should be the right camera's, Tcw = [I | (-b, 0, 0)]: dict(t_err m, rot_deg, inlier_share)."""
    T = np.asarray(Tcw, np.float64).reshape(4, 4)
    t_err = float(np.linalg.norm(T[:3, 3] - np.array([-BASELINE, 0.0, 0.0])))
    ang = float(np.degrees(np.arccos(np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
    return dict(t_err=t_err, rot_deg=ang, inlier_share=float(n_inliers) / max(int(n_rows), 1), t=T[:3, 3].copy())


# ---- the bounds, shared by the CPU and the GPU tests (the kernels are bit-equal to the oracle today: both see the same values)
# measured with the oracle (level-0 ORB keys, 5 levels, N = 1000: 298 keys) -> bound
LK_MEDIAN_ERR_PX = 0.55      # 0.5425 px over 291 keys
LK_WITHIN_2PX = 0.80         # 83.5 %
LK_MEDIAN_DY_PX = 0.40       # 0.3746 px
DEPTH_MEDIAN_REL = 0.05      # 3.18 % over 158 depths
DEPTH_WITHIN_10PCT = 0.80    # 82.3 %
POSE_T_ERR_M = 2 * 0.005453  # t = (-0.54025, 0.00224, 0.00389) against (-0.53717, 0, 0); 289 rows, 240 inliers
POSE_ROT_DEG = 2 * 0.04423
POSE_INLIER_SHARE = 0.75     # 83.0 %
VO_MEDIAN_REL = 0.05         # 3.10 % over 239 valid map points of 502 keys
VO_WITHIN_10PCT = 0.85       # 86.6 %
VO_T_ERR_M = 2 * 0.019164    # t = (-0.54184, 0.01457, 0.01154); 239 rows, 236 inliers
VO_ROT_DEG = 2 * 0.08393


def check_lk_disparity(s):
    print("LK disparity:", s)
    assert s["n"] >= 250
    assert s["median_err"] <= 1.0                      # the fixture's resolution
    assert s["median_err"] <= LK_MEDIAN_ERR_PX
    assert s["within_2px"] >= LK_WITHIN_2PX
    assert s["median_dy"] <= LK_MEDIAN_DY_PX           # a rectified pair: the flow is horizontal


def check_depths(s, median_rel=DEPTH_MEDIAN_REL, within=DEPTH_WITHIN_10PCT, n_min=120):
    print("stereo depths:", s)
    assert s["n"] >= n_min
    assert s["median_rel"] <= median_rel
    assert s["within_10pct"] >= within


def check_baseline(s, t_err=POSE_T_ERR_M, rot=POSE_ROT_DEG, share=POSE_INLIER_SHARE):
    print("recovered baseline:", s)
    assert s["t_err"] <= t_err
    assert s["rot_deg"] <= rot
    assert s["inlier_share"] >= share


def strided(img, stride, fill=255):
    """img [h, w] in a [h, stride] buffer whose padding bytes are `fill`."""
    h, w = img.shape
    buf = np.full((h, stride), fill, np.uint8)
    buf[:, :w] = img
    return buf


def pitched(imgs, stride, pitch, fill=255):
    """A flat uint8 slab: image p at byte p * pitch with row stride `stride`; every other byte is `fill`."""
    h, w = imgs[0].shape
    assert stride >= w and pitch >= stride * h
    slab = np.full(len(imgs) * pitch, fill, np.uint8)
    for p, img in enumerate(imgs):
        slab[p * pitch:p * pitch + stride * h].reshape(h, stride)[:, :w] = img
    return slab
