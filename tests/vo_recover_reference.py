"""CPU composition of recovery in the searchByBow VO loop -- the yardstick of a tb_vo_recover_enable loop (include/tb_capi.h;
trackingbench_slam_amd/vo.py, StereoVO(tracker="bow", keyframe_db=N, relocalize=M, recover=...)).

The reference has no such step; every operator is the reference's, pinned elsewhere, and the composition is ours:

    vo_bow_reference's frame (SetBow, searchByBow against the tracking keyframe, carry, rows, PoseOptimization)
      -> lost = n_inliers < lost_inliers
      -> lost: the database's topk candidates (reloc_reference.Keyframes.candidates) verified by reloc_reference.relocalize
      -> an answer (best_rank >= 0): the frame takes the winner's pose, match list, rows, outlier flags and inlier count; its
         carried map points are those of the winner's matches (vo_desc_reference.carry on the stored keyframe: the failed
         step's points are dropped, outlier rows keep theirs); the stored keyframe becomes the keyframe it tracks against
      -> a keyframe step then runs vo_bow_reference's keyframe block unchanged: stereo points at the (adopted) pose, the frame
         becomes the keyframe and goes into the store.

A frame that is not lost, or finds no answer, is vo_bow_reference.step's frame bit for bit. One sequence per state; a state and
a store can be injected, so each GPU step can be checked from the GPU's previous state.
"""
import numpy as np

import oracle
import reloc_reference as rr
import vo_bow_reference as vb
import vo_desc_reference as vd
import vo_reference as vr

F32 = np.float32
# StereoVO's RECOVER_DEFAULTS: ORB-SLAM-style figures, not the reference's
DEFAULTS = dict(lost_inliers=30, topk=4, exclude_newest=1, min_inliers=50)


def recover_stage(kps, desc, bow, n_inliers, store, tr, P, recover):
    """The stage between the tracking step's pose and the keyframe block -> dict(lost, track_inliers, recovered_kf, slot, out):
    out = reloc_reference.relocalize's result for a lost frame (None otherwise), slot = the winning ring slot or -1."""
    rec = dict(DEFAULTS, **recover)
    res = dict(lost=bool(n_inliers < rec["lost_inliers"]), track_inliers=int(n_inliers), recovered_kf=-1, slot=-1, out=None)
    if not res["lost"]:
        return res
    slots = store.candidates(bow["bv"], rec["topk"], rec["exclude_newest"])
    out = rr.relocalize(kps, desc, bow, store, slots, tr, P.K, P.nlevels, P.scale, rec["min_inliers"])
    res["out"] = out
    if out["best_rank"] >= 0:
        res.update(recovered_kf=int(out["best_kf"]), slot=int(slots[out["best_rank"]]))
    return res


def step(state, store, left, right, P, tr, voc, recover, spawn_Tcw=None, orb=None):
    """Frame state['t'] of one sequence; store: the reloc_reference.Keyframes of the keyframes so far (a keyframe step adds to
    it). Returns (new state, info) as vo_bow_reference.step does, with info['lost'], ['track_inliers'], ['recovered_kf'],
    ['reloc'] (the verification of a lost frame, else None) and state['kf_id'] = the frame index of the tracking keyframe."""
    t = state["t"]
    keyframe = t % P.keyframe_every == 0
    inv_sigma2 = oracle.scale_factors(P.nlevels, P.scale)[3]
    kps, desc = vd.extract(left, P) if orb is None else orb
    m = len(kps)
    keys = np.stack([kps["x"], kps["y"]], -1).astype(F32).reshape(-1, 2)
    bow = vb.set_bow(voc, desc, tr.levelsup)
    Tcw = np.asarray(state["Tcw"], F32).reshape(4, 4).copy()
    matches = np.zeros(0, oracle.MATCH)
    kf = state["kf"]
    if t > 0:
        matches = vb.match(kps, desc, bow, kf, tr)
        mp, valid = vd.carry(matches, m, kf["mp"], kf["valid"])
    else:
        mp, valid = np.zeros((m, 3), F32), np.zeros(m, bool)
    obs = vd.rows(kps, mp, valid, inv_sigma2)
    info = dict(keyframe=keyframe, matches=matches, obs=obs if t > 0 else obs[:0], n_inliers=0, outlier=np.zeros(0, np.uint8), lost=False,
                track_inliers=0, recovered_kf=-1, reloc=None, seed=Tcw.copy())
    if t > 0:
        n_inl, Tcw, outl, _ = oracle.pose_opt(P.K, state["Tcw"], obs)
        Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
        info.update(n_inliers=int(n_inl), outlier=outl)
        r = recover_stage(kps, desc, bow, int(n_inl), store, tr, P, recover)
        info.update(lost=r["lost"], track_inliers=r["track_inliers"], recovered_kf=r["recovered_kf"], reloc=r["out"])
        if r["recovered_kf"] >= 0:
            c, won = r["out"]["cands"][r["out"]["best_rank"]], store.kfs[r["slot"]]
            Tcw = c["Tcw"].copy()
            mp, valid = vd.carry(c["matches"], m, won["mp"], won["valid"])
            info.update(matches=c["matches"], obs=c["obs"], n_inliers=c["n_inliers"], outlier=c["outlier"], seed=won["Tcw"].copy())
            kf = dict(orb=won["orb"], desc=won["desc"], mp=won["mp"], valid=won["valid"], frame=won["kf_id"], bow=won["bow"])
    if keyframe:
        mp, valid = vr.resize_map_points(mp, valid, m)
        depth = oracle.add_map_points_by_stereo(right, left, P.cam, keys, P.bf)
        mp, valid = vr.spawn_points(keys, depth, Tcw if spawn_Tcw is None else spawn_Tcw, P.K, mp, valid)
        info["depth"] = depth
        kf = dict(orb=kps.copy(), desc=desc.copy(), mp=mp.copy(), valid=valid.copy(), frame=t, bow=bow)
        store.add(kf, Tcw if spawn_Tcw is None else spawn_Tcw, t)
    new = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, orb=kps, desc=desc, kf=kf, last_img=None, bow=bow, kf_id=kf["frame"])
    return new, info


def run(left, right, Tcw0, P, tr, voc, capacity, recover, T=None):
    """A free run of S = 1 sequence over frames 0..T-1 -> (states, infos, store): per frame the state (with 'kf_id') and the
    info (with 'lost', 'track_inliers', 'recovered_kf')."""
    T = len(left) if T is None else T
    s = vd.initial_state(Tcw0)
    store = rr.Keyframes(capacity, voc.c.scoring)
    states, infos = [], []
    for t in range(T):
        s, info = step(s, store, left[t], right[t], P, tr, voc, recover)
        states.append(s); infos.append(info)
    return states, infos, store
