"""CPU composition of the mono mode of the optical-flow VO loop (include/tb_capi.h, tb_vo_mono) over the oracle's entry points,
tests/vo_reference.py and tests/triangulate_reference.py -- the yardstick of StereoVO(mono=True).

Frame 0 is vo_reference's stereo keyframe. A tracking frame is vo_reference's, plus alive &= status. A keyframe at t > 0 reads
no right image: the keys LK has held since the last keyframe are triangulated from (kf_keys, kf_Tcw) and (keys, Tcw), and the
keys that have a map point are merged with the frame's ORB keys. A state can be injected, and the pose the triangulation runs at
can be given (tri_Tcw: the GPU's optimised pose), so one step can be compared with the GPU's bit for bit.
"""
import numpy as np

import oracle
import triangulate_reference as tri
import vo_reference as vr

F32 = np.float32


class MonoParams:
    def __init__(self, cos_parallax_max=tri.COS_PARALLAX_MAX, chi2_max=tri.CHI2_MAX, cell=8, capacity=2048):
        self.cos_parallax_max, self.chi2_max, self.cell, self.capacity = float(cos_parallax_max), float(chi2_max), int(cell), int(capacity)


def initial_state(Tcw0):
    s = vr.initial_state(Tcw0)
    s.update(kf_keys=np.zeros((0, 2), F32), kf_Tcw=np.zeros((4, 4), F32), alive=np.zeros(0, bool))
    return s


def merge_cell(x, y, cell, cw, ch):
    """The occupancy cell ((int)x / cell, (int)y / cell) of a pixel as C computes it (truncation toward zero), -1 outside the
    cw x ch grid and for a coordinate no int holds."""
    x, y = F32(x), F32(y)
    if not (abs(x) < F32(1.0e9)) or not (abs(y) < F32(1.0e9)):
        return -1
    ix, iy = int(x), int(y)
    cx = abs(ix) // cell if ix >= 0 else -(abs(ix) // cell)
    cy = abs(iy) // cell if iy >= 0 else -(abs(iy) // cell)
    if cx < 0 or cx >= cw or cy < 0 or cy >= ch:
        return -1
    return cy * cw + cx


def merge(keys, mp, valid, orb_xy, width, height, M):
    """The mono keyframe's new key list -> (keys, mp, valid, survivors, added)"""
    cw, ch = -(-width // M.cell), -(-height // M.cell)
    surv = np.nonzero(valid)[0]
    occupied = set()
    for i in surv:
        c = merge_cell(keys[i, 0], keys[i, 1], M.cell, cw, ch)
        if c >= 0:
            occupied.add(c)
    take = []
    for j in range(len(orb_xy)):
        if len(surv) + len(take) >= M.capacity:
            break
        c = merge_cell(orb_xy[j, 0], orb_xy[j, 1], M.cell, cw, ch)
        if c >= 0 and c in occupied:
            continue
        take.append(j)
    take = np.array(take, np.int64)
    new_keys = np.concatenate([keys[surv], orb_xy[take]]).astype(F32).reshape(-1, 2)
    new_mp = np.concatenate([mp[surv], np.zeros((len(take), 3), F32)]).astype(F32)
    new_valid = np.concatenate([np.ones(len(surv), bool), np.zeros(len(take), bool)])
    return new_keys, new_mp, new_valid, len(surv), len(take)


def step(state, left, right, P, M, tri_Tcw=None, spawn_Tcw=None):
    """Frame state['t'] of one sequence. Returns (new state, info): vo_reference's info plus, on a mono keyframe, tri_points
    [n][3], tri_flags [n], tri_tally [6] (code 0 counted over M.capacity entries, as the device counts its pitch), survivors,
    added, and pre = the keys / mp / valid before the merge renumbered them."""
    t = state["t"]
    if t == 0:
        new, info = vr.step(state, left, right, P, spawn_Tcw)
        new.update(kf_keys=new["keys"].copy(), kf_Tcw=new["Tcw"].copy(), alive=np.ones(len(new["keys"]), bool))
        return new, info
    keyframe = t % P.keyframe_every == 0
    # the tracking half of vo_reference.step (test_vo.cpp:716-761), which keeps LK's status
    cur, idx = oracle.search_by_opflow(left, state["last_img"], P.cam, state["keys"], True, True)
    keys = np.asarray(cur, F32).reshape(-1, 2).copy()
    n = len(keys)
    status = np.zeros(n, bool)
    status[idx] = True
    valid = status & state["valid"][:n]
    mp = np.where(valid[:, None], state["mp"][:n], F32(0)).astype(F32)
    sel = np.nonzero(valid)[0]
    obs = np.zeros(len(sel), oracle.OBS)
    obs["u"] = keys[sel, 0]; obs["v"] = keys[sel, 1]
    obs["X"] = mp[sel, 0]; obs["Y"] = mp[sel, 1]; obs["Z"] = mp[sel, 2]
    obs["inv_sigma2"] = 1.0
    n_inl, Tcw, outl, _ = oracle.pose_opt(P.K, state["Tcw"], obs)
    Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
    info = dict(keyframe=keyframe, obs=obs, n_inliers=int(n_inl), outlier=outl)
    alive = state["alive"][:n] & status
    kf_keys, kf_Tcw = state["kf_keys"], state["kf_Tcw"]
    if keyframe:
        Tt = Tcw if tri_Tcw is None else np.asarray(tri_Tcw, F32).reshape(4, 4)
        skip = valid | ~alive
        pts, flags, tally = tri.triangulate_batch(kf_keys[None, :n], keys[None], None, kf_Tcw[None], Tt[None], P.K, skip=skip[None],
                                                  cos_parallax_max=M.cos_parallax_max, chi2_max=M.chi2_max)
        pts, flags, tally = pts[0], flags[0], tally[0].copy()
        tally[0] += M.capacity - n
        acc = flags == tri.ACCEPTED
        mp = np.where(acc[:, None], pts, mp).astype(F32)
        valid = valid | acc
        info.update(tri_points=pts, tri_flags=flags, tri_tally=tally, pre=dict(keys=keys.copy(), mp=mp.copy(), valid=valid.copy()))
        levels, sf = oracle.pyramid(left, P.nlevels, P.scale)
        kps, _, _ = oracle.orb_extract(levels, sf, P.target, P.init_th, P.min_th)
        orb_xy = np.stack([kps["x"], kps["y"]], -1).astype(F32).reshape(-1, 2)
        keys, mp, valid, nsurv, nadd = merge(keys, mp, valid, orb_xy, P.width, P.height, M)
        info.update(survivors=nsurv, added=nadd)
        kf_keys, kf_Tcw, alive = keys.copy(), Tt.copy(), np.ones(len(keys), bool)
    new = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, last_img=np.ascontiguousarray(left, np.uint8), kf_keys=kf_keys,
               kf_Tcw=kf_Tcw, alive=alive)
    return new, info


def run(left, right, Tcw0, P, M, T=None):
    """Free run of one sequence over frames 0..T-1; `right` is read at frame 0 only -> (states, infos)"""
    T = len(left) if T is None else T
    s = initial_state(Tcw0)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, left[t], right[t] if t == 0 else None, P, M)
        states.append(s); infos.append(info)
    return states, infos
