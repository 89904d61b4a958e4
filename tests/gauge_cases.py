"""World gauges: the shared cases of tests/test_oracle_gauge.py (CPU) and tests/test_gpu_gauge.py (GPU).

A gauge is a rigid transform G = [R_G | t_G] of the world frame: map points become X' = R_G X + t_G, poses Tcw' = Tcw G^-1,
pixels and weights stay. Every residual is unchanged, so an optimum moves to the old one times G^-1 and the outlier flags stay;
the arithmetic, however, runs at whatever orientation G puts it -- in particular in any branch of the quaternion extraction
(po_quat_from_R of csrc/tb_se3.h, quat_from_R of oracle/oracle_pose.cpp; Eigen's Quaternion(Matrix3)) we choose.

Everything here is computed in float64 and rounded to float32 once at the end. The pose cases form ONE table (pose_cases()):
the CPU module probes every entry for conditioning (an edge permutation must not move the oracle), the GPU module runs them.
"""
import functools

import numpy as np

from trackingbench_slam_amd import synth

K = (718.856, 718.856, 607.1928, 185.2157)
F32 = np.float32


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def gauge(R, t):
    """4x4 float64 [R | t]"""
    G = np.eye(4)
    G[:3, :3] = np.asarray(R, np.float64)
    G[:3, 3] = np.asarray(t, np.float64)
    return G


def quat_branch(R):
    """The branch Eigen's Quaternion(Matrix3) takes on the rotation block of R (3x3 or 4x4): "w" (trace > 0) or the largest
    diagonal entry "x" / "y" / "z", ties to the lower index."""
    R = np.asarray(R, np.float64)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "w"
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return "xyz"[i]


IDENTITY = gauge(np.eye(3), (0, 0, 0))
GAUGES = {
    "x180": gauge(np.diag([1.0, -1.0, -1.0]), (3, -2, 5)),
    "y180": gauge(np.diag([-1.0, 1.0, -1.0]), (3, -2, 5)),
    "z180": gauge(np.diag([-1.0, -1.0, 1.0]), (3, -2, 5)),
    "perm120": gauge([[0, 0, 1], [1, 0, 0], [0, 1, 0]], (1, 2, 3)),          # trace 0 and all diagonals tie
    "x170": gauge(rodrigues((2.967, 0.1, -0.05)), (10, -4, 7)),
    "y175": gauge(rodrigues((0.05, 3.054, 0.08)), (-20, 1, 30)),
    "z160": gauge(rodrigues((0.1, -0.1, 2.79)), (5, 5, -5)),
    "gen2": gauge(rodrigues((1.2, -1.1, 0.9)), (100, -50, 20)),              # a large rotation that stays in "w", a large translation
}
# the branch a pose NEAR THE IDENTITY falls in after the gauge. perm120 ties: an exact identity lands in "x" (ties go to the lower
# index, trace 0 is not > 0), a pose a little off the identity anywhere -- such cases assert nothing and count for no coverage.
GAUGE_BRANCH = {"id": "w", "x180": "x", "y180": "y", "z180": "z", "perm120": None, "x170": "x", "y175": "y", "z160": "z", "gen2": "w"}


def get(name):
    return IDENTITY if name == "id" else GAUGES[name]


def inv(G):
    Gi = np.eye(4)
    Gi[:3, :3] = G[:3, :3].T
    Gi[:3, 3] = -G[:3, :3].T @ G[:3, 3]
    return Gi


def gauge_poses(T, G):
    """Tcw' = Tcw G^-1 for one pose or a stack, float32"""
    return (np.asarray(T, np.float64) @ inv(G)).astype(F32)


def ungauge_poses(T, G):
    """Tcw = Tcw' G, float64"""
    return np.asarray(T, np.float64) @ G


def gauge_points(X, G):
    """X' = R_G X + t_G for [n, 3] points, float32"""
    return (np.asarray(X, np.float64) @ G[:3, :3].T + G[:3, 3]).astype(F32)


def ungauge_points(X, G):
    return (np.asarray(X, np.float64) - G[:3, 3]) @ G[:3, :3]


def gauge_pose_problem(Tin, obs, G):
    """(Tcw_in, obs) of a pose problem under G"""
    o = obs.copy()
    X = gauge_points(np.stack([obs["X"], obs["Y"], obs["Z"]], 1), G)
    o["X"], o["Y"], o["Z"] = X[:, 0], X[:, 1], X[:, 2]
    return gauge_poses(Tin, G), o


def gauge_ba(poses, pts, G):
    """(poses, pts) of a BA window under G"""
    return gauge_poses(poses, G), gauge_points(pts, G)


def gauge_projection(case, G):
    """A synth.projection_case under G: Tcw, mp["pos"] and mp["normal"] move, everything else is shared"""
    c = dict(case)
    c["Tcw"] = gauge_poses(case["Tcw"], G)
    mp = case["mp"].copy()
    mp["pos"] = gauge_points(case["mp"]["pos"], G)
    mp["normal"] = (case["mp"]["normal"].astype(np.float64) @ G[:3, :3].T).astype(F32)
    c["mp"] = mp
    return c


# ---------------------------------------------------------------------------------------------------------------- pose cases
class PoseCase:
    """One input of tb_pose_opt: Tin [4, 4] float32, obs (oracle.OBS), pre (flags or None), the gauge's name and the branch
    of the quaternion extraction Tin must fall in (None: not pinned)."""

    def __init__(self, name, Tin, obs, pre, gname, branch):
        self.name, self.Tin, self.obs, self.pre, self.gname, self.branch = name, Tin, obs, pre, gname, branch

    def __repr__(self):
        return self.name


GAUGED_PROBLEMS = ((1, 300, 0.15), (3, 50, 0.3), (4, 9, 0.0), (6, 700, 0.5))      # seed, n, outlier fraction
EQUIVARIANCE_PROBLEMS = GAUGED_PROBLEMS + ((7, 10, 0.0), (8, 257, 0.1))           # the CPU equivariance family
SIZES = (10, 11, 255, 256, 257, 512, 513)                                         # the n < 10 break, the 256-lane stride
SIZE_GAUGES = ("id", "y175")
FAR_STARTS = ((0.6, 2.0), (1.0, 3.0), (1.5, 4.0))                                 # converges, lost, lost (11 points behind the camera)
# the identity and one gauge per other branch: a lost start returns its input pose through the quaternion round trip, so these are
# the pose cases in which a slip in a branch of the extraction shows in the output itself (a start that converges only begins
# somewhere else and reaches the same optimum)
FAR_GAUGES = ("id", "x170", "y180", "z160")
# the far starts are far from the identity before any gauge: their branches are what quat_branch says, written down here
FAR_BRANCH = {"id": "w", "x170": "x", "y180": "y", "z160": "z"}
BATCH_PITCH = 300
BATCH_COUNTS = (0, 2, 3, 9, 10, 256, 257, BATCH_PITCH, BATCH_PITCH + 5)
BATCH_GAUGES = ("x180", "y180", "z180", "perm120", "x170", "y175", "z160", "y180", "gen2")
BATCH_LOST = 7                                                                    # problem 7 is the (1.0, 3.0) lost start
FAR_BRANCH_BATCH = "y"                                                            # ... which under its gauge, y180, sits in "y"


def problem(seed, n, frac, K=K):
    return synth.pose_problem(seed, n, K, noise_px=0.4, outlier_frac=frac)


def far_start(Tt, a, d):
    """[rodrigues(a (0.5, 0.7, -0.5)) | (d, -d/2, d/3)] Tt"""
    return (gauge(rodrigues(a * np.array([0.5, 0.7, -0.5])), (d, -d / 2, d / 3)) @ Tt.astype(np.float64)).astype(F32)


def _mk(name, Tin, obs, pre, gname, branch=False):
    T, o = gauge_pose_problem(Tin, obs, get(gname))
    return PoseCase(name, T, o, pre, gname, GAUGE_BRANCH[gname] if branch is False else branch)


def batch_problem(p):
    """Problem p of the direct batch call: (Tin, obs with BATCH_COUNTS[p] rows), ungauged"""
    n = BATCH_COUNTS[p]
    if p == BATCH_LOST:
        Tt, _, obs = problem(11, n, 0.1)
        return far_start(Tt, 1.0, 3.0), obs
    Tt, Ti, obs = problem(40 + p, max(n, 1), 0.0 if n < 12 else 0.1)
    return Ti, obs[:n]


@functools.lru_cache(maxsize=None)
def pose_cases():
    """name -> PoseCase: every pose problem the GPU module runs (the batch's problems cut at the pitch)."""
    out = []
    for seed, n, frac in GAUGED_PROBLEMS:
        _, Ti, obs = problem(seed, n, frac)
        for g in GAUGES:
            # Ti is the exact identity: under perm120 it lands in "x" exactly
            br = "x" if g == "perm120" else GAUGE_BRANCH[g]
            out.append(_mk("gauged-s%d-%s" % (seed, g), Ti, obs, None, g, br))
            out.append(_mk("gauged-s%d-%s-pre" % (seed, g), Ti, obs, (np.arange(n) % 7 == 0).astype(np.uint8), g, br))
    for i, n in enumerate(SIZES):
        _, Ti, obs = problem(20 + i, n, 0.0 if n < 12 else 0.1)
        for g in SIZE_GAUGES:
            out.append(_mk("size-%d-%s" % (n, g), Ti, obs, None, g))
    Tt, Ti, obs = problem(11, 300, 0.1)
    for a, d in FAR_STARTS:
        for g in FAR_GAUGES:
            out.append(_mk("far-%.1f-%s" % (a, g), far_start(Tt, a, d), obs, None, g, FAR_BRANCH[g]))
    for g in ("id", "z180"):
        out.append(_mk("allpre-%s" % g, Ti, obs, np.ones(300, np.uint8), g))
    for p, n in enumerate(BATCH_COUNTS):
        if n >= 3:
            Tin, o = batch_problem(p)
            g = BATCH_GAUGES[p]
            br = FAR_BRANCH_BATCH if p == BATCH_LOST else ("x" if g == "perm120" else GAUGE_BRANCH[g])
            out.append(_mk("batch-%d" % p, Tin, o[:BATCH_PITCH], None, g, br))
    return {c.name: c for c in out}


def cases(prefix):
    return [c for n, c in pose_cases().items() if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------------------------------ BA cases
# name -> (seed, nkf, npt, nfixed, obs_per_pt, pose_noise, pt_noise, iters)
BA_WINDOWS = {"mfma": (1, 5, 200, 2, 5, 0.02, 0.05, 10),        # up to 10 free keyframes: the MFMA-tiled path
              "large": (31, 13, 300, 2, 6, 0.02, 0.05, 6),      # 11 free keyframes: the large-window path
              "far": (50, 3, 40, 1, 3, 3.0, 12.0, 8)}           # a start far from the optimum: rejected LM steps
BA_FAR_GAUGE = "z160"
BA_BATCH_GAUGES = ("x180", "y175", "z160", "gen2")


@functools.lru_cache(maxsize=None)
def ba_window(name, K=K):
    """(poses_init, pts_init, obs, nfixed, iters) of a named window, ungauged"""
    seed, nkf, npt, nfixed, per, pn, xn, iters = BA_WINDOWS[name]
    _, Pi, _, Xi, obs = synth.ba_problem(seed, nkf, npt, K, obs_per_pt=per, pose_noise=pn, pt_noise=xn)
    return Pi, Xi, obs, nfixed, iters


def assert_ba_branch(P, nfixed, gname):
    """Every free keyframe of the gauged window sits in the gauge's branch; returns it (None: not pinned)"""
    want = GAUGE_BRANCH[gname]
    if want is not None:
        for k in range(nfixed, len(P)):
            assert quat_branch(P[k]) == want, (gname, k, quat_branch(P[k]))
    return want
