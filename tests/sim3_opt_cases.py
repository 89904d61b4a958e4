"""Constructed problems for the OptimizeSim3 tests (tests/test_sim3_opt_reference.py, tests/test_gpu_sim3_opt.py): stereo points
seen by two cameras a known (s, R, t) apart, as pixel rows. Every draw comes from numpy's default_rng(seed), so a seed names a
problem."""
import numpy as np

import pose_graph_sim3_reference as ps
import sim3_cases as sc
import sim3_opt_reference as so

K = sc.K
K_ANISO = (718.856, 652.3, 607.1928, 185.2157)     # fx != fy
BF = 0.54 * K[0]                                   # KITTI's stereo baseline times fx
W, H = sc.W, sc.H


def truth(s=1.0, angle=0.1, dist=1.1):
    """(s, R12, t12) of the gain case: 0.1 rad and 1.1 m"""
    return sc.truth(s, angle, dist)


def matrix(T):
    return ps.make(*T)


def points(rng, n, K, zmin=5.0, zmax=40.0, half=None):
    """n points in camera coordinates zmin to zmax m away, anywhere in the image or (half) within `half` pixels of its centre"""
    if half is None:
        uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    else:
        uv = np.stack([rng.uniform(K[2] - half, K[2] + half, n), rng.uniform(K[3] - half, K[3] + half, n)], -1)
    z = rng.uniform(zmin, zmax, n)
    return np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)


def stereo_point(rng, X, K, pix, disp):
    """what a stereo camera makes of the point X: its pixel with N(0, pix) noise, its depth with the error of a disparity error
    N(0, disp) px at the baseline BF / fx, and the point back-projected from the two: (uv [n, 2], X [n, 3])"""
    n = len(X)
    uv = so.project(X, K) + rng.normal(0, 1, (n, 2)) * pix
    z = X[:, 2] + rng.normal(0, 1, n) * disp * X[:, 2] ** 2 / BF
    return uv, np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)


def problem(seed, n, pitch=None, T=None, pix=0.5, disp=0.5, outliers=0.0, octaves=False, K=K, zmin=5.0, zmax=40.0, half=None):
    """(rows OBS_ROW [pitch], good bool [pitch], (s, R, t)): n rows of stereo points; round(n * outliers) of them, in a random
    order, have their camera-1 point and pixel displaced by 2 to 6 m sideways"""
    rng = np.random.default_rng(seed)
    pitch = n if pitch is None else pitch
    s, R, t = truth() if T is None else T
    X2 = points(rng, n, K, zmin, zmax, half)
    X1 = s * X2 @ R.T + t
    good = np.ones(n, bool)
    nbad = int(round(n * outliers))
    good[rng.permutation(n)[:nbad]] = False
    shift = rng.uniform(2.0, 6.0, n) * rng.choice([-1.0, 1.0], n)
    X1 = X1 + np.where(good, 0.0, shift)[:, None] * np.array([1.0, 0.3, 0.0])
    uv1, M1 = stereo_point(rng, X1, K, pix, disp)
    uv2, M2 = stereo_point(rng, X2, K, pix, disp)
    w1 = w2 = None
    if octaves:
        w1 = (np.float32(1.2) ** (-2 * rng.integers(0, 4, n))).astype(np.float32)
        w2 = (np.float32(1.2) ** (-2 * rng.integers(0, 4, n))).astype(np.float32)
    rows = so.make_rows(M1, M2, uv1, uv2, w1, w2, pitch)
    g = np.zeros(pitch, bool)
    g[:n] = good
    return rows, g, (s, R, t)


def perturbed(T, seed, rot=0.02, trans=0.1, scale=0.02):
    """the srt record of Exp(a random tangent vector of those sizes) T"""
    rng = np.random.default_rng(seed)
    d = np.concatenate([rot * _unit(rng), trans * _unit(rng), [scale * rng.choice([-1.0, 1.0])]])
    return ps.srt_from_matrix(ps.exp(d) @ matrix(T))


def _unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def sim3_rows(rows):
    """the tb_sim3_row view of pixel rows: the first six fields and the two weights"""
    import sim3_reference as sr
    out = np.zeros(len(rows), sr.ROW)
    for f in sr.FIELDS:
        out[f] = rows[f]
    return out


def errors(srt, T):
    """(relative scale error, rotation error in rad, translation error in m) of an srt record"""
    return sc.errors(dict(srt=np.asarray(srt, np.float64)), T)


FAR = dict(zmin=70.0, zmax=80.0, half=60.0, disp=0.3)   # a distant, narrow scene: see far()


def far(seed, n, pitch=None, outliers=0.0, K=K, octaves=False, T=None, pert=(0.002, 0.2, 0.02)):
    """(rows, good, truth, seed srt): a scene 70 to 80 m away within 60 px of the image centre, where rotation, translation and
    scale are hard to tell apart: the smallest eigenvalue of H is below 1e-6 of its largest diagonal entry, under LM's lambda0, so
    the damped steps are short and the default iteration counts end before chi2 reaches its rounding floor. That is what lets a
    GPU test compare iteration and trial counts exactly. The seed is the truth perturbed by `pert`."""
    T = sc.truth(1.1, 0.02, 0.5) if T is None else T
    rows, good, T = problem(seed, n, pitch, T=T, outliers=outliers, K=K, octaves=octaves, **FAR)
    return rows, good, T, perturbed(T, seed, *pert)
