"""CPU composition of the VO loop with the searchByNN tracker (test/test_vo.cpp:213, the line test_vo_1 runs): the descriptor
frame of tests/vo_desc_reference.py -- its extract / carry / rows pieces and the oracle's pose optimisation -- with the matcher
line swapped for tests/lsh_reference.py. The yardstick of tb_vo_create_lsh (StereoVO(tracker="lsh"))."""
import numpy as np

import oracle
import lsh_reference as lr
import vo_desc_reference as vd
import vo_reference as vr

F32 = np.float32
Params = vr.Params
initial_state = vd.initial_state


class Tracker:
    """tb_vo_lsh: searchByNN(cur, kf, 0, 5, 10, 30) with LshIndexParams(20, 10, 2) by default; the bit table from seed or given."""

    def __init__(self, nlevels=5, ratio=10.0, min_th=30.0, min_level=0, max_level=None, tables=20, key_size=10, multi_probe_level=2,
                 seed=0, bits=None):
        self.kind = "lsh"
        self.ratio, self.min_th = float(F32(ratio)), float(F32(min_th))
        self.min_level, self.max_level = int(min_level), int(nlevels if max_level is None else max_level)
        self.multi_probe_level = int(multi_probe_level)
        self.bits = lr.draw_bits(tables, key_size, seed) if bits is None else np.asarray(bits, np.uint16)


def match(desc, kf, tr):
    """The tracker: the current frame (query) against the keyframe (train)."""
    return lr.search_by_nn(desc, kf["desc"], tr.bits, tr.multi_probe_level, tr.ratio, tr.min_th)


def step(state, left, right, P, tr, spawn_Tcw=None, keyframe=None):
    """Frame state['t'] of one sequence: vo_desc_reference.step with the matcher line swapped. keyframe: None = the cadence."""
    t = state["t"]
    keyframe = (t % P.keyframe_every == 0) if keyframe is None else bool(keyframe)
    inv_sigma2 = oracle.scale_factors(P.nlevels, P.scale)[3]
    kps, desc = vd.extract(left, P)
    m = len(kps)
    keys = np.stack([kps["x"], kps["y"]], -1).astype(F32).reshape(-1, 2)
    Tcw = np.asarray(state["Tcw"], F32).reshape(4, 4).copy()
    matches = np.zeros(0, oracle.MATCH)
    if t > 0:
        kf = state["kf"]
        matches = match(desc, kf, tr)
        mp, valid = vd.carry(matches, m, kf["mp"], kf["valid"])
    else:
        mp, valid = np.zeros((m, 3), F32), np.zeros(m, bool)
    obs = vd.rows(kps, mp, valid, inv_sigma2)
    info = dict(keyframe=keyframe, matches=matches, obs=obs if t > 0 else obs[:0], n_inliers=0, outlier=np.zeros(0, np.uint8))
    if t > 0:
        n_inl, Tcw, outl, _ = oracle.pose_opt(P.K, state["Tcw"], obs)
        Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
        info.update(n_inliers=int(n_inl), outlier=outl)
    kf = state["kf"]
    if keyframe:
        mp, valid = vr.resize_map_points(mp, valid, m)
        depth = oracle.add_map_points_by_stereo(right, left, P.cam, keys, P.bf)
        mp, valid = vr.spawn_points(keys, depth, Tcw if spawn_Tcw is None else spawn_Tcw, P.K, mp, valid)
        info["depth"] = depth
        kf = dict(orb=kps.copy(), desc=desc.copy(), mp=mp.copy(), valid=valid.copy(), frame=t)
    new = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, orb=kps, desc=desc, kf=kf, last_img=None)
    return new, info


def run(left, right, Tcw0, P, tr, T=None):
    """Free run of one sequence over frames 0..T-1 -> (list of states after every frame, list of infos)."""
    T = len(left) if T is None else T
    s = initial_state(Tcw0)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, left[t], right[t], P, tr)
        states.append(s); infos.append(info)
    return states, infos
