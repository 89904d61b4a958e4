"""CPU composition of loop correction in the searchByBow VO loop: what a keyframe step would do with a verified revisit, built
from vo_bow_reference's frame, reloc_reference's verification and pose_graph_reference's solver -- the yardstick of a
tb_vo_loop_enable loop (include/tb_capi.h; trackingbench_slam_amd/vo.py, StereoVO(tracker="bow", keyframe_db=N, relocalize=M,
loop_close=...)). The reference has no such step; every operator is pinned elsewhere and the composition is ours.

A keyframe step t > 0, after the tracking step's pose optimisation and before the keyframe block:

    query    the database's topk candidates for the current BowVector (exclude_newest), verified by reloc_reference.relocalize with
             min_inliers
    graph    nodes = the stored keyframes in ascending kf_id, then the current frame; node 0, the oldest, is fixed; odometry edges
             join consecutive nodes, Z = T_next T_prev^-1 from the stored poses and the current pose; one loop edge joins the
             winning keyframe's node to the current node, Z = best_Tcw T_j^-1. No answer, or fewer than 2 keyframes held: no edge.
    solve    pose_graph_reference.solve(nfixed = 1, iters, w_rot, w_trans)
    adopt    where a loop closed and the solver did not flag the graph: every stored keyframe takes its node's pose and its valid
             map points move rigidly with it, X' = T_new^-1 T_old X in float64, stored as float32; the keyframe snapshot and the
             frame's carried map points (copies of the newest keyframe's points) move by the newest keyframe's correction; the
             current pose becomes the last node's. obs, outlier, n_inliers and the match list stay: they describe the tracking step.

The keyframe block then runs unchanged: the frame spawns its stereo points at the corrected pose and goes into the store with it.
A step that closes nothing is vo_bow_reference.step's frame bit for bit.
"""
import numpy as np

import oracle
import pose_graph_reference as pg
import reloc_reference as rr
import vo_bow_reference as vb
import vo_desc_reference as vd
import vo_reference as vr

F32 = np.float32
DEFAULTS = dict(topk=4, exclude_newest=1, min_inliers=50, iters=10, w_rot=1.0, w_trans=1.0)


def build_graph(store, Tcw, best_kf, best_Tcw, w_rot=1.0, w_trans=1.0):
    """-> (slots of the live keyframes in ascending kf_id, poses float32 [n + 1, 4, 4], edges); no loop -> best_kf < 0"""
    slots = sorted((s for s in range(store.capacity) if store.kfs[s] is not None), key=lambda s: store.kfs[s]["kf_id"])
    poses = np.stack([store.kfs[s]["Tcw"] for s in slots] + [np.asarray(Tcw, F32).reshape(4, 4)]).astype(F32)
    n = len(poses)
    if best_kf < 0 or len(slots) < 2:
        return slots, poses, np.zeros(0, pg.EDGE)
    edges = [pg.edge_between(i, i + 1, poses[i], poses[i + 1], w_rot, w_trans) for i in range(n - 1)]
    j = [store.kfs[s]["kf_id"] for s in slots].index(best_kf)
    edges.append(pg.make_edge(j, n - 1, pg.pose_in(best_Tcw) @ pg.inv(pg.pose_in(poses[j])), w_rot, w_trans))
    return slots, poses, np.array(edges)


def move_points(mp, valid, T_old, T_new):
    """X' = T_new^-1 (T_old X) for the valid points, float64 in the kernel's order of operations (Y = (R_old X + t_old) - t_new,
    X' = R_new' Y, sums left to right), stored as float32; the others keep their bytes"""
    Ro, Rn = np.asarray(T_old, np.float64)[:3, :3], np.asarray(T_new, np.float64)[:3, :3]
    to, tn = np.asarray(T_old, np.float64)[:3, 3], np.asarray(T_new, np.float64)[:3, 3]
    out = np.asarray(mp, F32).copy()
    v = np.asarray(valid, bool)
    X = np.asarray(mp, np.float64)[v]
    Y = [(Ro[i, 0] * X[:, 0] + Ro[i, 1] * X[:, 1] + Ro[i, 2] * X[:, 2]) + to[i] - tn[i] for i in range(3)]
    out[v] = np.stack([Rn[0, i] * Y[0] + Rn[1, i] * Y[1] + Rn[2, i] * Y[2] for i in range(3)], 1).astype(F32)
    return out


def loop_stage(kps, desc, bow, Tcw, store, tr, P, loop):
    """-> dict(closed, loop_kf, loop_inliers, reloc, slots, before, after, edges, stats); the store is not changed"""
    lp = dict(DEFAULTS, **loop)
    cand = store.candidates(bow["bv"], lp["topk"], lp["exclude_newest"])
    out = rr.relocalize(kps, desc, bow, store, cand, tr, P.K, P.nlevels, P.scale, lp["min_inliers"])
    slots, poses, edges = build_graph(store, Tcw, int(out["best_kf"]) if out["best_rank"] >= 0 else -1, out["best_Tcw"], lp["w_rot"],
                                      lp["w_trans"])
    res = dict(closed=False, loop_kf=-1, loop_inliers=0, reloc=out, slots=slots, before=poses, after=poses, edges=edges, stats=np.zeros(8))
    if len(edges) == 0:
        return res
    after, stats = pg.solve(poses, 1, edges, lp["iters"])
    res.update(after=after, stats=stats)
    if stats[7] == 0:
        res.update(closed=True, loop_kf=int(out["best_kf"]), loop_inliers=int(out["cands"][out["best_rank"]]["n_inliers"]))
    return res


def adopt_store(store, res):
    """every stored keyframe takes its node's pose and its valid points move with it"""
    before, after = res["before"], res["after"]
    for i, s in enumerate(res["slots"]):
        k = store.kfs[s]
        store.kfs[s] = dict(k, mp=move_points(k["mp"], k["valid"], before[i], after[i]), Tcw=after[i].copy())


def adopt(store, res, kf, mp, valid):
    """the stored keyframes, the snapshot kf and the carried points (mp, valid) after the correction -> (kf, mp, Tcw)"""
    adopt_store(store, res)
    before, after = res["before"], res["after"]
    i = len(res["slots"]) - 1     # the newest keyframe: the snapshot and the carried points are copies of its points
    kf = dict(kf, mp=move_points(kf["mp"], kf["valid"], before[i], after[i]))
    return kf, move_points(mp, valid, before[i], after[i]), after[-1].copy()


def step(state, store, left, right, P, tr, voc, loop, orb=None, after=None, spawn_Tcw=None):
    """Frame state['t'] of one sequence (vo_bow_reference.step with the stage in it); a keyframe step adds to the store.
    info['loop'] = loop_stage's result on a keyframe step t > 0, else None. after: node poses to adopt instead of the solver's own,
    which stay in info['loop']['solved'] (a GPU step is checked from the GPU's solution); spawn_Tcw: the pose the keyframe block
    spawns at and stores, as in vo_bow_reference.step."""
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
    info = dict(keyframe=keyframe, matches=matches, obs=obs if t > 0 else obs[:0], n_inliers=0, outlier=np.zeros(0, np.uint8), loop=None)
    if t > 0:
        n_inl, Tcw, outl, _ = oracle.pose_opt(P.K, state["Tcw"], obs)
        Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
        info.update(n_inliers=int(n_inl), outlier=outl)
        if keyframe:
            res = loop_stage(kps, desc, bow, Tcw, store, tr, P, loop)
            info["loop"] = res
            info["drifted_Tcw"] = Tcw.copy()
            res["solved"] = res["after"]
            if after is not None and res["closed"]:
                res["after"] = np.asarray(after, F32).reshape(-1, 4, 4)[:len(res["before"])].copy()
            if res["closed"]:
                kf, mp, Tcw = adopt(store, res, kf, mp, valid)
    if keyframe:
        mp, valid = vr.resize_map_points(mp, valid, m)
        depth = oracle.add_map_points_by_stereo(right, left, P.cam, keys, P.bf)
        mp, valid = vr.spawn_points(keys, depth, Tcw if spawn_Tcw is None else spawn_Tcw, P.K, mp, valid)
        info["depth"] = depth
        kf = dict(orb=kps.copy(), desc=desc.copy(), mp=mp.copy(), valid=valid.copy(), frame=t, bow=bow)
        store.add(kf, Tcw if spawn_Tcw is None else spawn_Tcw, t)
    new = dict(t=t + 1, Tcw=Tcw, keys=keys, mp=mp, valid=valid, orb=kps, desc=desc, kf=kf, last_img=None, bow=bow)
    return new, info


def run(left, right, Tcw0, P, tr, voc, capacity, loop, orbs=None):
    """A free run of one sequence -> (states, infos, store); orbs: per frame (kps, desc) to use instead of extracting"""
    s = vd.initial_state(Tcw0)
    store = rr.Keyframes(capacity, voc.c.scoring)
    states, infos = [], []
    for t in range(len(left)):
        s, info = step(s, store, left[t], right[t], P, tr, voc, loop, orb=None if orbs is None else orbs[t])
        states.append(s); infos.append(info)
    return states, infos, store
