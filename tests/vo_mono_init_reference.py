"""CPU composition of the mono loop that starts without a right image (include/tb_capi.h, tb_vo_mono_init) over
tests/vo_mono_reference.py and tests/two_view_reference.py -- the yardstick of StereoVO(mono=True, init=True).

Frame 0 runs ORB only: the key list is the ORB list, no key has a map point, the pose is the reset pose. While a sequence is
not initialised a tracking step is LK alone (alive &= status) and the pose stays the reset pose bit for bit; a keyframe step
t > 0 runs the two-view operator on (kf_keys, keys, skip = !alive, Tcw0 = kf_Tcw). Status 0 with at least min_tracks alive keys:
the pose becomes Tcw1, key i takes points[i] where point_flags[i] == 1, the sequence is initialised. Either way vo_mono_reference's
merge follows (with no survivor it yields a fresh ORB list: the re-seed). An initialised sequence is vo_mono_reference's, untouched.
"""
import numpy as np

import oracle
import two_view_reference as tv
import vo_mono_reference as vm

F32 = np.float32
MIN_TRACKS = 100


def initial_state(Tcw0):
    s = vm.initial_state(Tcw0)
    s.update(initialised=False, init_frame=-1, attempts=0)
    return s


def _orb_xy(left, P, capacity):
    levels, sf = oracle.pyramid(left, P.nlevels, P.scale)
    kps, _, _ = oracle.orb_extract(levels, sf, P.target, P.init_th, P.min_th)
    return np.stack([kps["x"], kps["y"]], -1).astype(F32).reshape(-1, 2)[:capacity]


def step(state, left, P, M, prm=None, min_tracks=MIN_TRACKS, tri_Tcw=None):
    """Frame state['t'] of one sequence; no right image anywhere. Returns (new state, info). On an attempt info["two_view"] is
    two_view_reference's dict. tri_Tcw: the pose an initialised sequence's keyframe triangulates at (the GPU's optimised pose)."""
    t = state["t"]
    extra = dict(initialised=state["initialised"], init_frame=state["init_frame"], attempts=state["attempts"])
    if state["initialised"]:
        new, info = vm.step({k: v for k, v in state.items() if k not in extra}, left, None, P, M, tri_Tcw=tri_Tcw)
        new.update(extra)
        return new, info
    img = np.ascontiguousarray(left, np.uint8)
    if t == 0:
        keys = _orb_xy(left, P, M.capacity)
        n = len(keys)
        new = dict(t=1, Tcw=state["Tcw"].copy(), keys=keys, mp=np.zeros((n, 3), F32), valid=np.zeros(n, bool), last_img=img,
                   kf_keys=keys.copy(), kf_Tcw=state["Tcw"].copy(), alive=np.ones(n, bool), **extra)
        return new, dict(keyframe=True, n_inliers=0)
    keyframe = t % P.keyframe_every == 0
    cur, idx = oracle.search_by_opflow(left, state["last_img"], P.cam, state["keys"], True, True)
    keys = np.asarray(cur, F32).reshape(-1, 2).copy()
    n = len(keys)
    status = np.zeros(n, bool)
    status[idx] = True
    alive = state["alive"][:n] & status
    Tcw = state["Tcw"].copy()
    mp, valid = np.zeros((n, 3), F32), np.zeros(n, bool)
    kf_keys, kf_Tcw = state["kf_keys"], state["kf_Tcw"]
    info = dict(keyframe=keyframe, n_inliers=0)
    if keyframe:
        prm = tv.params() if prm is None else prm
        r = tv.two_view(P.K, kf_keys[:n], keys, n, (~alive).astype(np.uint8), None, None, kf_Tcw, prm)
        extra["attempts"] += 1
        info["two_view"] = r
        info["alive_count"] = int(alive.sum())
        if r["status"] == tv.OK and alive.sum() >= min_tracks:
            Tcw = r["Tcw1"].copy()
            acc = r["point_flags"] == 1
            mp = np.where(acc[:, None], r["points"], mp).astype(F32)
            valid = acc.copy()
            extra.update(initialised=True, init_frame=t)
        info["pre"] = dict(keys=keys.copy(), mp=mp.copy(), valid=valid.copy())
        orb_xy = _orb_xy(left, P, 1 << 30)
        keys, mp, valid, nsurv, nadd = vm.merge(keys, mp, valid, orb_xy, P.width, P.height, M)
        info.update(survivors=nsurv, added=nadd)
        kf_keys, kf_Tcw, alive = keys.copy(), Tcw.copy(), np.ones(len(keys), bool)
    new = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, last_img=img, kf_keys=kf_keys, kf_Tcw=kf_Tcw, alive=alive, **extra)
    return new, info


def run(left, Tcw0, P, M, prm=None, min_tracks=MIN_TRACKS, T=None):
    """Free run of one sequence over frames 0..T-1 -> (states, infos)"""
    T = len(left) if T is None else T
    s = initial_state(Tcw0)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, left[t], P, M, prm, min_tracks)
        states.append(s); infos.append(info)
    return states, infos


def baseline(G, a, b):
    """the distance between the camera centres of the ground-truth poses G[a] and G[b]"""
    c = lambda T: -T[:3, :3].T @ T[:3, 3]
    return float(np.linalg.norm(c(np.asarray(G[a], np.float64)) - c(np.asarray(G[b], np.float64))))
