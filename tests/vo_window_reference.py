"""CPU composition of the window BA in the optical-flow VO loop -- the yardstick of a tb_vo_window_ba_enable loop (include/tb_capi.h;
trackingbench_slam_amd/vo.py, StereoVO(window_ba=...)).

The loop is tests/vo_reference.py's step. Between two keyframes key i of every frame is the same physical point, so the frames
from one keyframe to the next are a local-BA window over the first keyframe's stereo points. On top of vo_reference's state a
state carries the segment log `seg` (None before frame 0):

    kf_t     the frame index of the segment's keyframe (slot 0)
    keys     list of [n, 2] float32, one per logged slot: slot 0 the keyframe's keys, slot j the keys tracked at frame kf_t + j
    ok       list of [n] bool: slot 0 = spawned; slot j = spawned & valid & !outlier[row], all False when the pose was held
    poses    list of [4, 4] float32: the keyframe's pose, then every frame's optimised pose
    pts      [n, 3] float32: the keyframe's map points
    spawned  [n] bool: the keyframe made a stereo point at this key in its own step (depth > 0 and finite)

A keyframe step t > 0 logs its own slot, builds the window, runs oracle.local_ba on a copy of the segment, adopts the refined
pose of the last slot (or keeps the tracked one, bit for bit) and spawns the keyframe's points there (vo_reference.step's
spawn_Tcw); then the next segment starts. One sequence per state; a state can be injected, segment included.
"""
import numpy as np

import oracle
import vo_reference as vr

F32 = np.float32
DEFAULTS = dict(iters=10, fixed=1, min_obs=2, min_points=3)


def tracking_params(P):
    """P with a keyframe period no frame t > 0 meets: vo_reference.step then runs the tracking half alone."""
    return vr.Params(P.width, P.height, P.K, P.bf, P.nlevels, P.scale, P.target, P.init_th, P.min_th, keyframe_every=1 << 30)


def rows_of(valid):
    """row(i): key i's rank among the valid keys (the order PoseOptimization's rows are emitted in); -1 where not valid"""
    valid = np.asarray(valid, bool)
    return np.where(valid, np.cumsum(valid) - 1, -1)


def log_ok(spawned, valid, outlier):
    """ok of a tracked frame: spawned & valid & !outlier[row]; fewer than 3 rows held the pose and nothing is an inlier"""
    spawned, valid = np.asarray(spawned, bool), np.asarray(valid, bool)
    n = len(valid)
    if int(valid.sum()) < 3:
        return np.zeros(n, bool)
    row = rows_of(valid)
    outl = np.zeros(n, bool)
    outl[valid] = np.asarray(outlier, np.uint8)[row[valid]] != 0
    return spawned[:n] & valid & ~outl


def build_window(keys, ok, min_obs=2):
    """keys: sequence of [n, 2] per slot, ok: sequence of [n] bool per slot -> (obs as oracle.BA_OBS, number of points):
    every point with at least min_obs ok slots contributes them, grouped by ascending point and, within a point, ascending slot"""
    ok = np.stack([np.asarray(o, bool) for o in ok], 0)             # [N, n]
    cnt = ok.sum(0)
    pts = np.flatnonzero(cnt >= min_obs)
    obs = np.zeros(int(cnt[pts].sum()), oracle.BA_OBS)
    e = 0
    for i in pts:
        for j in np.flatnonzero(ok[:, i]):
            obs[e] = (j, i, keys[j][i, 0], keys[j][i, 1], 1.0)
            e += 1
    return obs, len(pts)


def refine(K, poses, pts, obs, prm=DEFAULTS):
    """oracle.local_ba on a copy of the segment -> (poses [N, 4, 4], pts [n, 3], stats [8]); no observation: nothing moves"""
    poses = np.asarray(poses, F32).reshape(-1, 4, 4).copy()
    pts = np.asarray(pts, F32).reshape(-1, 3).copy()
    if len(obs) == 0 or len(pts) == 0:
        return poses, pts, np.zeros(8)
    _, poses, pts, stats = oracle.local_ba(K, poses, prm["fixed"], pts, obs, prm["iters"])
    return poses, pts, stats


def adopt(Tcw, refined_last, n_points, stats, min_points=3):
    """(the pose the keyframe spawns at, adopted): the refined last slot when the window has min_points points, the BA accepted its
    input and the pose is finite; otherwise the tracked pose with every bit"""
    refined_last = np.asarray(refined_last, F32).reshape(4, 4)
    if n_points >= min_points and stats[7] != -1 and np.isfinite(refined_last).all():
        return refined_last.copy(), True
    return np.asarray(Tcw, F32).reshape(4, 4).copy(), False


def segment_start(t, keys, depth, mp, Tcw):
    d = np.asarray(depth, F32)
    spawned = (d > 0) & np.isfinite(d)
    return dict(kf_t=t, keys=[np.asarray(keys, F32).copy()], ok=[spawned.copy()], poses=[np.asarray(Tcw, F32).reshape(4, 4).copy()],
                pts=np.asarray(mp, F32).copy(), spawned=spawned)


def initial_state(Tcw0):
    s = vr.initial_state(Tcw0)
    s["seg"] = None
    return s


def step(state, left, right, P, prm=DEFAULTS):
    """Frame state['t'] of one sequence with the window BA. info adds, on a keyframe step t > 0, window = dict(obs, n_points,
    poses / pts (the segment as logged), refined_poses / refined_pts, stats, adopted, tracked_Tcw)."""
    prm = dict(DEFAULTS, **prm)
    t = state["t"]
    keyframe = t % P.keyframe_every == 0
    base = {k: v for k, v in state.items() if k != "seg"}
    seg = state.get("seg")
    if t == 0:
        new, info = vr.step(base, left, right, P)
        new["seg"] = segment_start(0, new["keys"], info["depth"], new["mp"], new["Tcw"])
        return new, info
    # the tracking half alone: the keys, the carried points and the optimised pose
    trk, tinfo = vr.step(base, left, right, tracking_params(P))
    seg = dict(seg, keys=list(seg["keys"]), ok=list(seg["ok"]), poses=list(seg["poses"]))
    j = t - seg["kf_t"]
    assert j == len(seg["keys"]), "the segment log has one slot per frame since its keyframe"
    seg["keys"].append(trk["keys"].copy())
    seg["ok"].append(log_ok(seg["spawned"], trk["valid"], tinfo["outlier"]))
    seg["poses"].append(trk["Tcw"].copy())
    if not keyframe:
        trk["seg"] = seg
        return trk, tinfo
    obs, npts = build_window(seg["keys"], seg["ok"], prm["min_obs"])
    rp, rx, stats = refine(P.K, np.stack(seg["poses"]), seg["pts"], obs, prm)
    Tcw, adopted = adopt(trk["Tcw"], rp[-1], npts, stats, prm["min_points"])
    # the whole step again with the keyframe block, spawning at the adopted pose (the tracking half repeats itself exactly)
    new, info = vr.step(base, left, right, P, spawn_Tcw=Tcw)
    new["Tcw"] = Tcw
    info["window"] = dict(obs=obs, n_points=npts, poses=np.stack(seg["poses"]), pts=seg["pts"], refined_poses=rp, refined_pts=rx,
                          stats=stats, adopted=adopted, tracked_Tcw=trk["Tcw"], seg=seg)
    new["seg"] = segment_start(t, new["keys"], info["depth"], new["mp"], Tcw)
    return new, info


def run(left, right, Tcw0, P, T=None, prm=DEFAULTS):
    """Free run of one sequence over frames 0..T-1 -> (list of states after every frame, list of infos)."""
    T = len(left) if T is None else T
    s = initial_state(Tcw0)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, left[t], right[t], P, prm)
        states.append(s); infos.append(info)
    return states, infos
