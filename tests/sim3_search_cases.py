"""The fixture of the SearchBySim3 tests: test_gpu_kf_store_sim3's store (S = 2 sequences, capacity 2, 200 keys, pitch 256; slot 0 a
keyframe 70 % of whose stored points are displaced by metres, slot 1 one with five points) with a query whose map drifted TOGETHER
WITH ITS POSE. With D: X -> s_d R_d X + t_d the query's world points are D X and its pose is Rq' = Rq R_d', tq' = s_d tq - Rq' t_d, so
its camera points are s_d (Tq X) and project exactly onto its keys (points moved under an unmoved pose would not: DESIGN.md 9p).
The truth is s12 = s_d, R12 = Rq Rst', t12 = s_d tq - s_d R12 tst.

A third of the query's keys carry 64 flipped bits: searchByBow refuses them (TH_LOW = 50, and their word changes) while their
distance to the stored descriptor stays near 68, under th_high = 100. Crafted entries of sequence 0 (its query and its slot 0):
    BEHIND   a query key whose point lies 5 m behind the stored camera
    OUTSIDE  a query key whose point lies 30 m to the side of the stored camera's axis
    TIE      stored key TIE_LOW is a copy of stored key TIE_HIGH (one pixel away, no point of its own): two equal descriptors in one
             window, the lower index has to win
Point ids are kept: q_ids[s][i] and kf_ids[a][s][j] name the scene point a key views."""
import numpy as np

import pnp_cases as pc
import sim3_cases as sc
import vo_bow_reference as vb
from test_gpu_kf_store import K, NLEVELS, SCALE, TR, _view
from trackingbench_slam_amd import synth

S, CAP, PITCH, N = 2, 2, 256, 200
WIDTH, HEIGHT = 640, 240
CANDS = np.array([[0, -1], [1, 0]], np.int32)
HEAVY_FLIPS = 64
SEED = 91


def drift():
    """D: X -> s R X + t in world coordinates"""
    return 1.1, sc.rodrigues((0.3, 1.0, -0.2), 0.1), np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74])


def _flip(rng, desc, rows, nbits):
    bits = np.unpackbits(desc, axis=1)
    for r in rows:
        bits[r, rng.permutation(256)[:nbits]] ^= 1
    return np.packbits(bits, axis=1)


def build_case(voc):
    """adds[a][s] = (keyframe, Tcw, kf_id), queries[s] = (kps, desc, bow), q_mp[s] float32 [N][3] = D applied to the true points, q_valid[s],
    q_Tcw[s] (the drifted pose), truth[s] = (s, R, t) of S12, q_ids[s], kf_ids[a][s], heavy[s], scenes[s] (the true points), crafted = dict(behind, outside, tie_low,
    tie_high, tie_query)"""
    rng = np.random.default_rng(SEED)
    sD, RD, tD = drift()
    adds = [[None] * S for _ in range(CAP)]
    out = dict(adds=adds, queries=[], q_mp=[], q_valid=[], q_Tcw=[], truth=[], q_ids=[], kf_ids=[[None] * S for _ in range(CAP)], heavy=[],
               crafted={}, scenes=[])
    vrng = np.random.default_rng(SEED + 1)
    for s in range(S):
        scene = (np.stack([rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(8, 30, N)], -1).astype(np.float32),
                 synth.descriptors_near_words(700 + s, voc, N, flips=12), rng.uniform(0, 360, N), rng.integers(0, NLEVELS, N))
        Tst = pc.pose(0.1 * (s + 1), -0.05, (0.4, -0.2, 0.5)).astype(np.float32)
        Tq = pc.moved(Tst.astype(np.float64), 0.2, 3.0).astype(np.float64)
        kps, desc, _, ids = _view(rng, voc, scene, Tq, N, 2, 0.5)
        heavy = np.sort(rng.permutation(N)[:N // 3])
        desc = _flip(rng, desc, heavy, HEAVY_FLIPS)
        q_valid = vrng.uniform(0, 1, N) < 0.9
        X = scene[0][ids].astype(np.float64)
        Rs, ts = Tst[:3, :3].astype(np.float64), Tst[:3, 3].astype(np.float64)
        kfs = []
        for a in range(CAP):
            kkps, kdesc, _, kids = _view(rng, voc, scene, Tst, N, 2, 0.5)
            mp = scene[0][kids].copy()
            valid = np.ones(N, bool)
            if a == 0:
                bad = rng.permutation(N)[:int(0.7 * N)]
                mp[bad] += (rng.uniform(2, 5, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))).astype(np.float32)
            else:
                valid[:] = False
                valid[rng.permutation(N)[:5]] = True
            kfs.append([kkps, kdesc, mp.astype(np.float32), valid, kids.copy()])
        if s == 0:
            free = [int(i) for i in np.nonzero(q_valid)[0] if i not in set(heavy.tolist())]
            b, o = free[0], free[1]
            X[b] = Rs.T @ (np.array([0.3, 0.1, -5.0]) - ts)        # 5 m behind the stored camera
            X[o] = Rs.T @ (np.array([30.0, 0.0, 10.0]) - ts)       # u = 360 * 3 + 320
            ids = ids.copy()
            ids[[b, o]] = -1
            # the tie: a heavy query key with a point, its true partner at index hi > 0 of slot 0; the copy goes to a lower index
            kkps, kdesc, mp, valid, kids = kfs[0]
            where = {int(p): j for j, p in enumerate(kids)}
            tq_key = next(int(i) for i in heavy if q_valid[i] and where[int(ids[i])] >= 20)
            hi = where[int(ids[tq_key])]
            lo = next(j for j in range(hi) if kids[j] not in set(ids[heavy].tolist()))
            kkps[lo] = kkps[hi]
            kkps["x"][lo] += 1.0
            kdesc[lo] = kdesc[hi]
            valid[lo] = False
            kids[lo] = kids[hi]
            out["crafted"] = dict(behind=b, outside=o, tie_low=lo, tie_high=hi, tie_query=tq_key)
        out["queries"].append((kps, desc, vb.set_bow(voc, desc, TR.levelsup)))
        out["q_ids"].append(ids)
        out["scenes"].append(scene[0])
        out["heavy"].append(heavy)
        out["q_valid"].append(q_valid)
        out["q_mp"].append((sD * X @ RD.T + tD).astype(np.float32))
        Rq, tq = Tq[:3, :3], Tq[:3, 3]
        Tqd = np.eye(4)
        Tqd[:3, :3] = Rq @ RD.T
        Tqd[:3, 3] = sD * tq - Tqd[:3, :3] @ tD
        out["q_Tcw"].append(Tqd.astype(np.float32))
        R12 = Rq @ Rs.T
        out["truth"].append((sD, R12, sD * tq - sD * R12 @ ts))
        for a, (kkps, kdesc, mp, valid, kids) in enumerate(kfs):
            adds[a][s] = (dict(orb=kkps, desc=kdesc, mp=mp, valid=valid, frame=10 * a, bow=vb.set_bow(voc, kdesc, TR.levelsup)), Tst, 10 * a)
            out["kf_ids"][a][s] = kids
    return out


def truth_srt(truth):
    """(s, R, t) -> srt [8] float64 (the quaternion w x y z with w >= 0, t, s)"""
    s, R, t = truth
    tr = np.trace(R)
    w = np.sqrt(max(0.0, 1.0 + tr)) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    q /= np.linalg.norm(q)
    return np.concatenate([q, np.asarray(t, np.float64), [s]])
