"""Constructed cases of the linear triangulation (tests/triangulate_reference.py), shared by the CPU and the GPU tests.

Three pose pairs at pitch 256 with counts (0, 65, 200): an empty pair, a partial wavefront, and a tail across a wavefront
boundary. The poses are away from the identity (a yaw of 0.4 / 2.6 rad and a world origin metres away). Pair 1 and pair 2 hold
random scene points seen with exact float32 pixels, a skip mask, and the gate cases at fixed slots:
  slot 3   code 3: a point behind both cameras (its pixels are the projection of a point at negative depth)
  slot 5   code 5: view 1's pixel moved 5 px across the epipolar line (the baseline is along x, so across = along v)
  slot 7   code 4: a point 4000 m away -- the 0.6 m baseline is far below the parallax gate
  slot 9   code 2: non-finite pixels (NaN in, NaN out)
Pair 2's baseline is 1.5 m. identical_pair() is a pose pair with IDENTICAL poses and identical rays (no baseline: A has rank 2,
the null vector is whatever the sweeps leave, and no point may be accepted).
"""
import numpy as np

K = (718.856, 718.856, 607.1928, 185.2157)
NPAIRS, PITCH = 3, 256
COUNTS = (0, 65, 200)
F32 = np.float32


def _pose(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry
    T[:3, 3] = t
    return T.astype(F32)


def _move(T, dx):
    """The same camera moved dx metres along its own x axis: Tcw' = [I | (-dx, 0, 0)] Tcw"""
    M = np.eye(4)
    M[0, 3] = -dx
    return (M @ T.astype(np.float64)).astype(F32)


def project(T, X, K=K):
    T = T.astype(np.float64)
    Xc = X @ T[:3, :3].T + T[:3, 3]
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], -1), Xc[:, 2]


def _world(T, xc):
    T = T.astype(np.float64)
    return (xc - T[:3, 3]) @ T[:3, :3]


def build(seed=11, K=K):
    """dict(xy0, xy1 [3][256][2] float32, counts, Tcw0, Tcw1 [3][4][4] float32, skip [3][256] uint8, X [3][256][3] float64 = the
    true points where there is one, slots = the gate cases' slots)"""
    rng = np.random.default_rng(seed)
    T0 = np.stack([_pose(0.0, 0.0, (0, 0, 0)), _pose(0.4, 0.05, (3.0, -1.0, 12.0)), _pose(2.6, -0.03, (-20.0, 2.0, 7.5))])
    T1 = np.stack([_move(T0[0], 0.6), _move(T0[1], 0.6), _move(T0[2], 1.5)])
    xy0 = np.zeros((NPAIRS, PITCH, 2), F32); xy1 = np.zeros((NPAIRS, PITCH, 2), F32)
    X = np.zeros((NPAIRS, PITCH, 3))
    skip = (rng.random((NPAIRS, PITCH)) < 0.15).astype(np.uint8)
    for p in range(NPAIRS):
        # points in front of camera 0, 4..30 m away, inside the image
        z = rng.uniform(4.0, 30.0, PITCH)
        u = rng.uniform(60, 1180, PITCH); v = rng.uniform(20, 350, PITCH)
        xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], -1)
        xc[3, 2] = -8.0; xc[3, 0] = 1.0; xc[3, 1] = 0.5                 # behind the cameras
        xc[7] = [(u[7] - K[2]) / K[0] * 4000.0, (v[7] - K[3]) / K[1] * 4000.0, 4000.0]   # no parallax
        X[p] = _world(T0[p], xc)
        a, _ = project(T0[p], X[p], K); b, _ = project(T1[p], X[p], K)
        xy0[p], xy1[p] = a.astype(F32), b.astype(F32)
        xy1[p, 5, 1] += F32(5.0)
        xy0[p, 9] = np.nan
        skip[p, [3, 5, 7, 9]] = 0
    return dict(xy0=xy0, xy1=xy1, counts=np.array(COUNTS, np.int32), Tcw0=T0, Tcw1=T1, skip=skip, X=X,
                slots=dict(depth=3, reprojection=5, parallax=7, nonfinite=9))


def identical_pair():
    """One pose pair with IDENTICAL poses and identical rays: 16 point pairs, no baseline at all"""
    T = _pose(0.4, 0.05, (3.0, -1.0, 12.0))
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(60, 1180, 16), rng.uniform(20, 350, 16)], -1).astype(F32)
    return xy, xy.copy(), T, T.copy()
