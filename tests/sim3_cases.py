"""Constructed 3D-3D problems for the Sim(3) tests (tests/test_sim3_reference.py, tests/test_gpu_sim3.py): rows built from a known
(s, R, t) -- s = 1.3, 0.3 rad about a tilted axis, 2 m -- with the points 5-40 m in front of both cameras and KITTI's K, and the
row contents that exercise the solver's and the score's edges. Every draw comes from numpy's default_rng(seed), so a seed names
a problem."""
import numpy as np

import sim3_reference as sr

K = (718.856, 718.856, 607.1928, 185.2157)
W, H = 1241, 376
CHUNK = 256      # S3_CHUNK of k_sim3.hip: the rows one LDS chunk holds
S_TRUE, ANGLE_TRUE, DIST_TRUE = 1.3, 0.3, 2.0


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def truth(s=S_TRUE, angle=ANGLE_TRUE, dist=DIST_TRUE):
    """(s, R12, t12): X1 = s R12 X2 + t12"""
    R = rodrigues((0.2, 1.0, 0.1), angle)
    t = dist * np.array([0.6, -0.1, 0.3]) / np.linalg.norm([0.6, -0.1, 0.3])
    return float(s), R, t


def points(rng, n, K=K):
    """n points in camera-2 coordinates, inside the image, 5-40 m away -- and in front of camera 1 under truth()"""
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    z = rng.uniform(5.0, 40.0, n)
    return np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)


def problem(seed, n, pitch=None, outliers=0.5, noise=0.0005, T=None, kind="scene", octaves=False, K=K):
    """(rows ROW [pitch], good bool [pitch], (s, R, t)): n rows, round(n * (1 - outliers)) of them in a random order true
    correspondences with isotropic Gaussian noise of `noise` times the depth on every coordinate; the others pair two unrelated
    random points. kind: "scene", "collinear" (every point of set 2 on one line), "behind" (set 2 behind its camera)."""
    rng = np.random.default_rng(seed)
    pitch = n if pitch is None else pitch
    s, R, t = truth() if T is None else T
    X2 = points(rng, n, K)
    if kind == "collinear":
        X2 = np.array([1.0, -0.5, 10.0]) + rng.uniform(0.0, 20.0, n)[:, None] * np.array([0.3, 0.1, 1.0])
    if kind == "behind":
        X2 = -X2
    X1 = s * X2 @ R.T + t
    if noise:
        X1 = X1 + rng.normal(0, 1, (n, 3)) * (noise * np.abs(X1[:, 2:3]))
        X2 = X2 + rng.normal(0, 1, (n, 3)) * (noise * np.abs(X2[:, 2:3]))
    ngood = int(round(n * (1.0 - outliers)))
    good = np.zeros(n, bool)
    good[rng.permutation(n)[:ngood]] = True
    X1 = np.where(good[:, None], X1, points(rng, n, K))
    w1 = w2 = None
    if octaves:
        w1 = (np.float32(1.2) ** (-2 * rng.integers(0, 8, n))).astype(np.float32)
        w2 = (np.float32(1.2) ** (-2 * rng.integers(0, 8, n))).astype(np.float32)
    rows = sr.make_rows(X1, X2, w1, w2, pitch)
    g = np.zeros(pitch, bool)
    g[:n] = good
    return rows, g, (s, R, t)


DRAWS = 5


def clean(draw):
    """the noise-free case: 200 exact rows rounded to float32, no outliers"""
    return problem(draw, 200, outliers=0.0, noise=0.0)


def noisy(draw):
    """the noisy case: 200 rows, noise of 0.05 % of the depth on every coordinate, half the rows replaced by random points"""
    return problem(10 + draw, 200)


def cases():
    """every case of the CPU tests as (name, rows, good, truth, RANSAC seed)"""
    out = [("clean%d" % d,) + clean(d) + (d,) for d in range(DRAWS)]
    return out + [("noisy%d" % d,) + noisy(d) + (d,) for d in range(DRAWS)]


def errors(res, T):
    """(relative scale error, rotation angle error in rad, translation error in m) of a reference / library result's srt"""
    s, R, t = T
    q = res["srt"][:4]
    Rq = np.array(sr.rotation([np.float64(v) for v in q]), np.float64)
    c = (np.trace(Rq @ R.T) - 1.0) / 2.0
    skew = Rq @ R.T - (Rq @ R.T).T
    ang = np.arctan2(np.linalg.norm([skew[2, 1], skew[0, 2], skew[1, 0]]) / 2.0, c)
    return abs(res["srt"][7] / s - 1.0), abs(float(ang)), float(np.linalg.norm(res["srt"][4:7] - t))
