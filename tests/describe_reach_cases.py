"""Inputs and reach arithmetic of the descriptor kernel's tests (tests/test_describe_reach_cpu.py, tests/test_gpu_describe_reach.py).

The kernel (csrc/k_describe.hip) blurs a 37 x 37 patch from a 43 x 43 source patch at (kx - 21, ky - 21): interior keypoints copy
aligned dwords (four sub-dword phases of kx - 21), keypoints within 21 px of a level border take the reflect-101 path, and every
rotated, rounded BRIEF tap must stay within 18 px. The image sets below are chosen so that the ORACLE's keypoints alone hit each
of these cases; `coverage` measures that from oracle output."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS, SCALE, TARGET, INI_TH, MIN_TH = 4, 0.8, 400, 20, 7
# (width, height, seeds): the second width is no multiple of 4
SETS = {"w200": (200, 160, (1, 2, 3)), "w203": (203, 157, (4, 5, 6))}


def pattern():
    """bit_pattern_31_ as an int array [256][4] = (x0, y0, x1, y1), from the kernel's own include file."""
    txt = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "orb_pattern.inc")).read()
    vals = [int(t) for t in re.findall(r"-?\d+", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))]
    assert len(vals) == 1024
    return np.array(vals, np.int32).reshape(256, 4)


def rotated_taps(angle_deg):
    """Rounded (row, column) of all 512 taps for float32 angles [n] in the kernel's operation order: a = cosf(angle * (pi / 180)),
    b = sinf(...); row = rn(x b + y a), column = rn(x a - y b), every product and sum rounded to float32. cos / sin are the
    double-precision functions rounded to float32 (the kernel's match glibc's correctly rounded cosf / sinf).
    Returns (rows, cols, raw_max): int arrays [n][512] and the largest |coordinate| before rounding."""
    f = np.float32
    ang = np.asarray(angle_deg, f)
    rad = (ang * f(3.1415926535897932384626433832795 / f(180.0))).astype(f)
    a = np.cos(rad.astype(np.float64)).astype(f)[:, None]
    b = np.sin(rad.astype(np.float64)).astype(f)[:, None]
    p = pattern().reshape(512, 2).astype(f)
    x, y = p[None, :, 0], p[None, :, 1]
    r = ((x * b).astype(f) + (y * a).astype(f)).astype(f)
    c = ((x * a).astype(f) - (y * b).astype(f)).astype(f)
    raw_max = float(max(np.abs(r).max(), np.abs(c).max()))
    return np.rint(r).astype(np.int32), np.rint(c).astype(np.int32), raw_max


def image(seed, w, h):
    """Blobs and diagonal ramps on a mid-grey ground, dense enough that FAST fires up to every level border, plus a saturated and
    an all-zero rectangle (each with corners of its own: the blocks survive the pyramid's resize as 255 / 0)."""
    rs = np.random.RandomState(1000 + seed)
    img = np.full((h, w), 128.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(w * h // 60):
        cx, cy = rs.uniform(0, w), rs.uniform(0, h)
        r = rs.uniform(1.5, 4.0)
        amp = rs.uniform(50, 120) * (1 if rs.uniform() < 0.5 else -1)
        x0, x1 = max(int(cx - 3 * r), 0), min(int(cx + 3 * r) + 1, w)
        y0, y1 = max(int(cy - 3 * r), 0), min(int(cy + 3 * r) + 1, h)
        d2 = (xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2
        img[y0:y1, x0:x1] += amp * np.exp(-d2 / (2 * r * r))
    img += 20.0 * np.sin((xx + yy) * (2 * np.pi / 37.0)) + 20.0 * np.sin((xx - yy) * (2 * np.pi / 29.0))   # diagonal ramps
    img = np.clip(np.rint(img + rs.randint(-2, 3, (h, w))), 0, 255)
    bx, by = int(rs.randint(30, w - 90)), int(rs.randint(30, h - 70))
    img[by:by + 34, bx:bx + 34] = 255
    img[by + 4:by + 38, bx + 40:bx + 74] = 0
    return img.astype(np.uint8)


def _has_flat_7x7(lv, kx, ky, value):
    """Is there a pixel within the keypoint's 37 x 37 blur window whose whole 7 x 7 neighbourhood (inside the level) is `value`?"""
    h, w = lv.shape
    y0, y1, x0, x1 = max(ky - 21, 0), min(ky + 22, h), max(kx - 21, 0), min(kx + 22, w)
    m = (lv[y0:y1, x0:x1] == value)
    if m.shape[0] < 7 or m.shape[1] < 7:
        return False
    s = np.cumsum(np.cumsum(np.pad(m.astype(np.int32), ((1, 0), (1, 0))), 0), 1)
    box = s[7:, 7:] - s[:-7, 7:] - s[7:, :-7] + s[:-7, :-7]
    return bool((box == 49).any())


def coverage(levels_list, sf, kps_list):
    """What the oracle's keypoints of an image set exercise. levels_list[i] = pyramid of image i, kps_list[i] = its keypoint records.
    Returns a dict: 'phase' = set of (kx - 21) & 3; 'border' = {side: set of distances to that level border} over keypoints;
    'row18', 'col18' = number of keypoints with a tap whose rounded row / column is +-18; 'max_tap' = largest |rounded coordinate|;
    'saturated', 'zero' = number of keypoints with a flat 7 x 7 of 255 / 0 under their blur window."""
    cov = {"phase": set(), "border": {s: set() for s in ("left", "right", "top", "bottom")}, "row18": 0, "col18": 0, "max_tap": 0,
           "saturated": 0, "zero": 0}
    for lv, k in zip(levels_list, kps_list):
        if len(k) == 0:
            continue
        rows, cols, _ = rotated_taps(k["angle"])
        cov["row18"] += int((np.abs(rows).max(axis=1) == 18).sum())
        cov["col18"] += int((np.abs(cols).max(axis=1) == 18).sum())
        cov["max_tap"] = max(cov["max_tap"], int(np.abs(rows).max()), int(np.abs(cols).max()))
        for i in range(len(k)):
            l = int(k["octave"][i])
            s = np.float32(sf[l]) if l else np.float32(1)
            kx, ky = int(round(float(k["x"][i]) / float(s))), int(round(float(k["y"][i]) / float(s)))
            h, w = lv[l].shape
            cov["phase"].add((kx - 21) & 3)
            cov["border"]["left"].add(kx); cov["border"]["right"].add(w - 1 - kx)
            cov["border"]["top"].add(ky); cov["border"]["bottom"].add(h - 1 - ky)
            cov["saturated"] += _has_flat_7x7(lv[l], kx, ky, 255)
            cov["zero"] += _has_flat_7x7(lv[l], kx, ky, 0)
    return cov


def check_coverage(cov):
    assert cov["phase"] == {0, 1, 2, 3}, cov["phase"]
    for side, d in cov["border"].items():
        assert min(d) >= 19, (side, min(d))                      # EDGE_THRESHOLD
        assert d & {19, 20}, (side, "reflect path", sorted(d)[:6])
        assert 21 in d and 22 in d, (side, "moved interior boundary", sorted(d)[:6])
    assert cov["row18"] > 0 and cov["col18"] > 0 and cov["max_tap"] == 18, (cov["row18"], cov["col18"], cov["max_tap"])
    assert cov["saturated"] > 0 and cov["zero"] > 0, (cov["saturated"], cov["zero"])
