"""Constructed 3D-2D problems for the P3P-RANSAC tests (tests/test_pnp_reference.py, tests/test_gpu_pnp.py): the far-seed
fixture of DESIGN.md 9l -- K = (360, 360, 320, 120), points 3-40 m in front of the camera, 0.5 px noise, uniformly random
outlier pixels -- and the row contents that exercise the solver's and the score's edges. Every draw comes from numpy's
default_rng(seed), so a seed names a problem."""
import numpy as np

from trackingbench_slam_amd.capi import OBS

K = (360.0, 360.0, 320.0, 120.0)
W, H = 640, 240
CHUNK = 256      # PNP_CHUNK of k_pnp.hip: the rows one LDS chunk holds


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def pose(yaw=0.3, pitch=-0.1, t=(1.5, -0.4, 2.0)):
    """a Tcw away from the identity, rounded to float32 (what the library is handed)"""
    T = np.eye(4)
    T[:3, :3] = rot_y(yaw) @ rot_x(pitch)
    T[:3, 3] = t
    return T.astype(np.float32).astype(np.float64)


def moved(T, yaw, d):
    """T moved by rot_y(yaw) and d * (0.6, 0, 0.8) metres: the far seed"""
    M = np.eye(4)
    M[:3, :3] = rot_y(yaw)
    M[:3, 3] = d * np.array([0.6, 0.0, 0.8])
    return (M @ T).astype(np.float32)


def project(T, Xw, K=K):
    pc = Xw @ T[:3, :3].T + T[:3, 3]
    return np.stack([pc[:, 0] / pc[:, 2] * K[0] + K[2], pc[:, 1] / pc[:, 2] * K[1] + K[3]], -1), pc[:, 2]


def problem(seed, n, pitch=None, outliers=0.5, noise=0.5, T=None, kind="scene", octaves=False, K=K):
    """(obs OBS [pitch], good bool [pitch], Tcw float64): n rows, the first round(n * (1 - outliers)) in a random order true
    observations. kind: "scene" (depths 3-40 m), "coplanar" (world points on one plane), "behind" (every point behind the camera,
    its row the pinhole projection all the same)."""
    rng = np.random.default_rng(seed)
    pitch = n if pitch is None else pitch
    T = pose() if T is None else np.asarray(T, np.float64)
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    z = rng.uniform(3.0, 40.0, n)
    if kind == "behind":
        z = -z
    pc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)
    if kind == "coplanar":   # the plane 0.2 x + 0.1 y + z = 15 of the camera frame
        ray = np.stack([(uv[:, 0] - K[2]) / K[0], (uv[:, 1] - K[3]) / K[1], np.ones(n)], -1)
        pc = ray * (15.0 / (ray @ np.array([0.2, 0.1, 1.0])))[:, None]
    Xw = ((pc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    px, _ = project(T, Xw.astype(np.float64), K)
    px = px + rng.normal(0, noise, (n, 2)) if noise else px
    ngood = int(round(n * (1.0 - outliers)))
    good = np.zeros(n, bool)
    good[rng.permutation(n)[:ngood]] = True
    bad = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    px = np.where(good[:, None], px, bad)
    obs = np.zeros(pitch, OBS)
    obs["u"][:n], obs["v"][:n] = px[:, 0], px[:, 1]
    obs["X"][:n], obs["Y"][:n], obs["Z"][:n] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    obs["inv_sigma2"][:n] = (np.float32(1.2) ** (-2 * rng.integers(0, 8, n))).astype(np.float32) if octaves else 1.0
    g = np.zeros(pitch, bool)
    g[:n] = good
    return obs, g, T


def far_seed(seed, K=K):
    """the issue's fixture: 200 rows, 60 of them good, 0.5 px noise; the stored seed 3 m / 0.2 rad from the truth"""
    obs, good, T = problem(seed, 200, outliers=0.7, K=K)
    return obs, good, T, moved(T, 0.2, 3.0)
