"""CPU composition of the VO loop with a projection tracker (test/test_projection.cpp test_projection, :449-646, with the
commented tracking lines enabled) over the oracle's entry points -- the yardstick of tb_vo_step_dev with a TB_VO_PROJECTION or
TB_VO_PROJECTION_MAP tracker (trackingbench_slam_amd/vo.py, StereoVO(tracker="projection" | "projection_map")).

    :512-513  setProjectionParam(30, 50, 30, true, 30); searchByProjection(cur_frame_ptr, key_frame)
    :516-517  setProjectionParam(30, 50, 30, true, 20); searchByProjection(map_ptr, cur_frame_ptr, 0.6)

One sequence per state; step() is one frame:
    ORB on the left image, the frame's lookup grid (inside the oracle's matchers) -> t > 0: the matcher at the last frame's pose,
    with no key taken (Frame::AddMapPoint never calls AddObservation); the matched map points and their descriptors go to the
    keys, a later match in list order winning a key; pose optimisation on one row per key with a map point, in key order ->
    keyframe: stereo depths, new map points (descriptor = the key's row); with the map tracker each is appended to the map.
The map holds the points of the last map_keyframes keyframes in insertion order (the one deviation: the reference's only
grows); a keyframe past that evicts the oldest keyframe's block. The glue reuses tests/vo_reference.py (twc, spawn_points) and
tests/vo_desc_reference.py (extract, rows). A state can be injected -- keyframe and map included -- so each GPU step can be
checked from the GPU's previous state.
"""
import numpy as np

import oracle
import vo_desc_reference as vd
import vo_reference as vr

F32 = np.float32
Params = vr.Params
MIN_DIST, MAX_DIST = F32(1.0), F32(1000.0)   # MapPoint::GetMin/MaxDistanceInvariance return constants (MapPoint.cpp:207-217)


class Tracker:
    """tb_vo_tracker of the projection trackers: the reference's arguments by default."""

    def __init__(self, kind, nratio=None, radio=0.6, th_high=50, histo_len=30, check_orientation=True, map_keyframes=4):
        assert kind in ("projection", "projection_map")
        self.kind = kind
        self.nratio = float(F32((30.0 if kind == "projection" else 20.0) if nratio is None else nratio))
        self.radio, self.th_high = float(F32(radio)), int(th_high)
        self.histo_len, self.check_orientation, self.map_keyframes = int(histo_len), bool(check_orientation), int(map_keyframes)


def empty_map():
    """No point, no block."""
    return dict(points=np.zeros(0, oracle.MAPPOINT), desc=np.zeros((0, 32), np.uint8), blocks=[])


def initial_state(Tcw0):
    """The state before frame 0: no keys, pose Tcw0, no keyframe, an empty map."""
    s = vd.initial_state(Tcw0)
    s.update(mp_desc=np.zeros((0, 32), np.uint8), map=empty_map())
    return s


def normal(pos, Ow):
    """MapPoint.cpp:22-24: (pos - Ow) / |pos - Ow| in float32, one operation per statement, left to right."""
    e = [F32(F32(pos[i]) - F32(Ow[i])) for i in range(3)]
    q = F32(e[0] * e[0])
    q = F32(q + F32(e[1] * e[1]))
    q = F32(q + F32(e[2] * e[2]))
    n = F32(np.sqrt(q))
    return np.array([F32(e[0] / n), F32(e[1] / n), F32(e[2] / n)], F32)


def map_records(pos, Ow):
    """The tb_mappoint records of new points at `pos`, made from camera centre Ow."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    rec = np.zeros(len(pos), oracle.MAPPOINT)
    rec["pos"] = pos
    for i in range(len(pos)):
        rec["normal"][i] = normal(pos[i], Ow)
    rec["min_dist"], rec["max_dist"], rec["bad"] = MIN_DIST, MAX_DIST, 0
    return rec


def map_append(mp, rec, desc, map_keyframes):
    """One keyframe's points (possibly none) join the map as a block; the (map_keyframes + 1)-th block evicts the oldest."""
    points, d, blocks = mp["points"], mp["desc"], list(mp["blocks"])
    if len(blocks) == map_keyframes:
        points, d, blocks = points[blocks[0]:], d[blocks[0]:], blocks[1:]
    return dict(points=np.concatenate([points, rec]), desc=np.concatenate([d, np.asarray(desc, np.uint8).reshape(-1, 32)]),
                blocks=blocks + [len(rec)])


def frame_records(mp, valid):
    """The keyframe's key-aligned map points as searchByProjection(F1, F2) reads them: pos, bad = no map point."""
    rec = np.zeros(len(valid), oracle.MAPPOINT)
    rec["pos"] = np.where(np.asarray(valid, bool)[:, None], mp, F32(0))
    rec["bad"] = ~np.asarray(valid, bool)
    return rec


def match(kps, desc, Tcw, state, P, tr):
    """The tracker at pose Tcw (the last frame's, :510); taken1 all zero (Observations() is 0 throughout the loop)."""
    sf = oracle.scale_factors(P.nlevels, P.scale)[0]
    taken = np.zeros(len(kps), np.uint8)
    if tr.kind == "projection":
        kf = state["kf"]
        return oracle.search_by_projection(Tcw, P.cam, P.width, P.height, kps, desc, taken, kf["orb"], frame_records(kf["mp"], kf["valid"]),
                                           kf["mp_desc"], sf, tr.nratio, tr.th_high, tr.histo_len, tr.check_orientation)
    m = state["map"]
    if len(m["points"]) == 0:
        return np.zeros(0, oracle.MATCH)
    return oracle.search_by_projection_map(Tcw, P.cam, P.width, P.height, kps, desc, taken, m["points"], m["desc"], sf, tr.nratio,
                                           tr.radio, tr.th_high)


def carry(matches, m, src_pos, src_valid, src_desc):
    """A fresh frame of m keys, then for every match whose source entry trainIdx has a map point, key queryIdx gets it with its
    descriptor (:520-530; Frame::AddMapPoint overwrites, so a later match in list order wins)."""
    mp = np.zeros((m, 3), F32)
    valid = np.zeros(m, bool)
    mpd = np.zeros((m, 32), np.uint8)
    for q, tr in zip(matches["queryIdx"], matches["trainIdx"]):
        if src_valid is None or src_valid[tr]:
            mp[q] = src_pos[tr]
            mpd[q] = src_desc[tr]
            valid[q] = True
    return mp, valid, mpd


def step(state, left, right, P, tr, spawn_Tcw=None):
    """Frame state['t'] of one sequence. Returns (new state, info) with info = matches, obs rows, n_inliers, outlier flags,
    keyframe (and depth on a keyframe)."""
    t = state["t"]
    keyframe = t % P.keyframe_every == 0
    inv_sigma2 = oracle.scale_factors(P.nlevels, P.scale)[3]
    kps, desc = vd.extract(left, P)
    m = len(kps)
    keys = np.stack([kps["x"], kps["y"]], -1).astype(F32).reshape(-1, 2)
    Tcw = np.asarray(state["Tcw"], F32).reshape(4, 4).copy()
    matches = np.zeros(0, oracle.MATCH)
    mp, valid, mpd = np.zeros((m, 3), F32), np.zeros(m, bool), np.zeros((m, 32), np.uint8)
    if t > 0:
        matches = match(kps, desc, Tcw, state, P, tr)
        if tr.kind == "projection":
            kf = state["kf"]
            mp, valid, mpd = carry(matches, m, kf["mp"], kf["valid"], kf["mp_desc"])
        else:
            mp, valid, mpd = carry(matches, m, state["map"]["points"]["pos"], None, state["map"]["desc"])
    obs = vd.rows(kps, mp, valid, inv_sigma2)
    info = dict(keyframe=keyframe, matches=matches, obs=obs if t > 0 else obs[:0], n_inliers=0, outlier=np.zeros(0, np.uint8))
    if t > 0:
        n_inl, Tcw, outl, _ = oracle.pose_opt(P.K, state["Tcw"], obs)
        Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
        info.update(n_inliers=int(n_inl), outlier=outl)
    kf, themap = state["kf"], state["map"]
    if keyframe:
        depth = oracle.add_map_points_by_stereo(right, left, P.cam, keys, P.bf)   # :602
        T = Tcw if spawn_Tcw is None else spawn_Tcw
        mp, valid = vr.spawn_points(keys, depth, T, P.K, mp, valid)
        new = np.nonzero((depth > 0) & np.isfinite(depth))[0]                     # spawn_points' own test
        mpd = mpd.copy()
        mpd[new] = desc[new]                                                      # :631 GetDescriptor(j)
        if tr.kind == "projection_map":
            themap = map_append(themap, map_records(mp[new], vr.twc(T)[1]), desc[new], tr.map_keyframes)   # :634
        info["depth"] = depth
        kf = dict(orb=kps.copy(), desc=desc.copy(), mp=mp.copy(), valid=valid.copy(), mp_desc=mpd.copy(), frame=t)
    new_state = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, mp_desc=mpd, orb=kps, desc=desc, kf=kf, map=themap, last_img=None)
    return new_state, info


def run(left, right, Tcw0, P, tr, T=None):
    """Free run of one sequence over frames 0..T-1 -> (list of states after every frame, list of infos)."""
    T = len(left) if T is None else T
    s = initial_state(Tcw0)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, left[t], right[t], P, tr)
        states.append(s); infos.append(info)
    return states, infos
