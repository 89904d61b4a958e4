"""Pyramidal Lucas-Kanade in float64, written from the definition of the method (Bouguet, "Pyramidal implementation of the
Lucas Kanade feature tracker", 2000) with numpy / scipy -- the yardstick of tests/test_lk_reference.py (the oracle) and
tests/test_gpu_flow_reference.py (k_pyr_down, k_lk_track). It shares no code and no number format with oracle/oracle_flow.cpp:
no 8-bit pyramid levels, no fixed-point weights, no integer window sums, no oscillation rule.

    pyramid      [1 4 6 4 1] x [1 4 6 4 1] / 256 with reflect-101 borders, unrounded, every second pixel ((n + 1) // 2); no level
                 that is not larger than the window is built
    derivatives  Scharr / 32: ([3 10 3] / 16 across) x ([-1 0 1] / 2 along), reflect-101 borders
    sampling     bilinear (scipy.ndimage.map_coordinates, order 1, mode 'mirror' = reflect-101)
    window       win x win samples centred on the point: offsets -(win - 1) / 2 .. (win - 1) / 2
    per level    G = sum [Ix Iy]^T [Ix Iy]; lambda_min(G) / win^2 < 1e-4: the level is skipped (at level 0: not tracked);
                 up to 30 steps d = G^-1 sum (I - J(. + v)) [Ix Iy]^T, v += d, until |d|^2 <= 1e-4
    levels       max_level levels above level 0; the flow found at a level is doubled into the next finer one
"""
import numpy as np
from scipy import ndimage

_K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
_SMOOTH = np.array([3.0, 10.0, 3.0]) / 16.0
_DIFF = np.array([-1.0, 0.0, 1.0]) / 2.0


def pyr_down(img):
    """One pyramid level: the 5x5 binomial filter, then every second row and column. float64 in and out."""
    a = ndimage.correlate1d(np.asarray(img, np.float64), _K5, axis=0, mode="mirror")
    a = ndimage.correlate1d(a, _K5, axis=1, mode="mirror")
    return a[::2, ::2].copy()


def pyramid(img, win=21, max_level=3):
    levels = [np.asarray(img, np.float64)]
    for _ in range(max_level):
        h, w = levels[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    """(dI/dx, dI/dy) per unit pixel."""
    gx = ndimage.correlate1d(ndimage.correlate1d(img, _SMOOTH, axis=0, mode="mirror"), _DIFF, axis=1, mode="mirror")
    gy = ndimage.correlate1d(ndimage.correlate1d(img, _SMOOTH, axis=1, mode="mirror"), _DIFF, axis=0, mode="mirror")
    return gx, gy


def _sample(img, x, y):
    return ndimage.map_coordinates(img, [y, x], order=1, mode="mirror")


def track(prev, nxt, pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
    """prev, nxt: images [h, w]; pts [n, 2] (x, y) in prev. Returns (next_pts [n, 2] float64, tracked [n] bool): tracked =
    the level-0 matrix passed the eigenvalue test and the point ended inside the image."""
    prev, nxt = np.asarray(prev, np.float64), np.asarray(nxt, np.float64)
    assert prev.ndim == 2 and prev.shape == nxt.shape
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    n = len(pts)
    P, Q = pyramid(prev, win, max_level), pyramid(nxt, win, max_level)
    r = (win - 1) / 2.0
    oy, ox = np.meshgrid(np.arange(win) - r, np.arange(win) - r, indexing="ij")
    ox, oy = ox.ravel()[None, :], oy.ravel()[None, :]
    flow = np.zeros((n, 2))
    tracked = np.ones(n, bool)
    for level in range(len(P) - 1, -1, -1):
        I, J = P[level], Q[level]
        gx, gy = scharr(I)
        p = pts / float(1 << level)
        wx, wy = p[:, 0:1] + ox, p[:, 1:2] + oy
        Iw, Ix, Iy = _sample(I, wx, wy), _sample(gx, wx, wy), _sample(gy, wx, wy)
        a, b, c = (Ix * Ix).sum(1), (Ix * Iy).sum(1), (Iy * Iy).sum(1)
        lam = 0.5 * (a + c - np.sqrt((a - c) ** 2 + 4.0 * b * b))
        good = lam / float(win * win) >= min_eig
        if level == 0:
            tracked &= good
        det = np.where(good, a * c - b * b, 1.0)
        active = good.copy()
        for _ in range(max_iter):
            k = np.nonzero(active)[0]
            if not len(k):
                break
            diff = Iw[k] - _sample(J, wx[k] + flow[k, 0:1], wy[k] + flow[k, 1:2])
            b1, b2 = (diff * Ix[k]).sum(1), (diff * Iy[k]).sum(1)
            dx = (c[k] * b1 - b[k] * b2) / det[k]
            dy = (a[k] * b2 - b[k] * b1) / det[k]
            flow[k, 0] += dx
            flow[k, 1] += dy
            active[k] = dx * dx + dy * dy > eps * eps
        if level:
            flow *= 2.0
    out = pts + flow
    h, w = prev.shape
    tracked &= (out[:, 0] >= 0) & (out[:, 0] <= w - 1) & (out[:, 1] >= 0) & (out[:, 1] <= h - 1)
    return out, tracked


# ---- the comparison tests/test_lk_reference.py (oracle) and tests/test_gpu_flow_reference.py (kernels) apply to a tracker
FAR_PX, FAR_CAP = 0.02, 0.05
# input -> (median distance in px, share beyond FAR_PX) measured with the oracle over the jointly tracked points (146, 138, 134 and
# 140 of them); the kernels are bit-equal to the oracle, so the same figures hold for them. Bounds: 4x the median, and FAR_CAP.
CASES = {
    "full_LR": (1.727e-4, 0.0274),
    "full_RL": (1.303e-4, 0.0),
    "crop_LR": (6.174e-5, 0.0075),
    "crop_RL": (7.667e-5, 0.0),
}


def inputs(name, backend):
    """(prev image, next image, about 150 ORB keys of prev at least 30 px from every border) of CASES[name]: the reference's stereo
    pair or its 333 x 211 crop, left -> right or right -> left. backend: whose ORB extractor picks the keys (stereo_fixture)."""
    import stereo_fixture as sf
    L, R = sf.pair()
    if name.startswith("crop"):
        L, R = sf.crop(L), sf.crop(R)
    a, b = (L, R) if name.endswith("LR") else (R, L)
    return a, b, sf.inner_keys(backend, a, 150 if name.endswith("LR") else 140)


def check(name, a, b, pts, got, status):
    """`got`, `status`: a tracker's next points and status flags on inputs(name). Over the points both sides track: the median
    distance to the float64 result is at most 4x the recorded one, and at most FAR_CAP of them lie further than FAR_PX away."""
    ref, ok = track(a, b, pts)
    both = ok & (np.asarray(status) > 0)
    assert both.sum() >= 0.85 * len(pts), (name, int(both.sum()))
    d = np.linalg.norm(np.asarray(got, np.float64)[both] - ref[both], axis=1)
    median, far = float(np.median(d)), float((d > FAR_PX).mean())
    print("%s: %d points, %d jointly tracked, median %.3e px, p90 %.3e px, %.2f %% beyond %.2f px" % (
        name, len(pts), both.sum(), median, np.percentile(d, 90), 100 * far, FAR_PX))
    assert median <= 4 * CASES[name][0], (name, median)
    assert far <= FAR_CAP, (name, far)
