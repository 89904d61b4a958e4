"""CPU composition of the keyframe store's Sim(3) query -- the yardstick of tb_kf_store_sim3_dev (include/tb_capi.h): the 3D-3D
rows through the verification's match list, sim3_reference.ransac on them, and the selection.

    vo_bow_reference.match (what tb_relocalize_batch_dev left in the work buffer)
      -> rows: a match counts where the stored entry trainIdx AND the query key queryIdx both have a valid map point, the last
         match in list order wins a key, rows in key order; X1 = the query's Tcw applied to the query key's world point, X2 = the
         stored keyframe's Tcw applied to its stored world point, both ((T0 X + T1 Y) + T2 Z) + T3 in float64, stored as float32;
         the weights are invLevelSigma2[octave] of the two keys
      -> sim3_reference.ransac
      -> select: the largest consensus, ties to the lower rank, absent candidates left out; -1 below min_consensus"""
import numpy as np

import oracle
import sim3_reference as sr
import vo_bow_reference as vb

F32 = np.float32
F64 = np.float64
SRT_EYE = np.array([1, 0, 0, 0, 0, 0, 0, 1], F64)


def apply(T, X):
    """T float32 4 x 4, X [n][3] float32 -> float32 [n][3], each coordinate ((T0 X + T1 Y) + T2 Z) + T3 in float64"""
    T = np.asarray(T, F32).reshape(4, 4).astype(F64)
    X = np.asarray(X, F32).reshape(-1, 3).astype(F64)
    out = np.zeros((len(X), 3), F32)
    for r in range(3):
        a = T[r, 0] * X[:, 0]
        a = a + T[r, 1] * X[:, 1]
        a = a + T[r, 2] * X[:, 2]
        a = a + T[r, 3]
        out[:, r] = a.astype(F32)
    return out


def rows(matches, q_kps, q_mp, q_valid, q_Tcw, kf, inv_sigma2):
    """the 3D-3D rows of one pair (sim3_reference.ROW, in key order)"""
    m, nk = len(q_kps), len(kf["orb"])
    win = np.full(m, -1, np.int64)
    for k, (q, tr) in enumerate(zip(matches["queryIdx"], matches["trainIdx"])):
        if 0 <= q < m and 0 <= tr < nk and kf["valid"][tr] and q_valid[q]:
            win[q] = k
    sel = np.nonzero(win >= 0)[0]
    j = matches["trainIdx"][win[sel]]
    sig = np.asarray(inv_sigma2, F32)
    w1 = sig[np.clip(q_kps["octave"][sel], 0, len(sig) - 1)]
    w2 = sig[np.clip(kf["orb"]["octave"][j], 0, len(sig) - 1)]
    return sr.make_rows(apply(q_Tcw, np.asarray(q_mp, F32)[sel]), apply(kf["Tcw"], np.asarray(kf["mp"], F32)[j]), w1, w2)


def absent():
    return dict(kf=-1, rows=np.zeros(0, sr.ROW), consensus=0, flags=sr.FLAG_VOID, winner=(-2, 0), S12=np.eye(4, dtype=F32), srt=SRT_EYE.copy(),
                inlier=np.zeros(0, np.uint8), margin=np.inf)


def solve_one(kps, desc, bow, q_mp, q_valid, q_Tcw, kf, tr, K, inv_sigma2, prm, matches=None):
    if matches is None:
        matches = vb.match(kps, desc, bow, kf, tr) if len(kps) and len(kf["orb"]) else np.zeros(0, oracle.MATCH)
    r0 = rows(matches, kps, q_mp, q_valid, q_Tcw, kf, inv_sigma2)
    r = sr.ransac(K, r0, len(r0), **prm)
    return dict(kf=kf["kf_id"], rows=r0, consensus=r["consensus"], flags=r["flags"], winner=r["winner"], S12=r["S1232"], srt=r["srt"],
                inlier=r["inlier"], margin=sr.margin(r, prm.get("chi2_max", sr.CHI2_MAX)))


def select(cands, min_consensus):
    """-> (best_rank, best_kf, best_S12, best_srt)"""
    best, most = -1, -1
    for r, c in enumerate(cands):
        if c["kf"] >= 0 and c["consensus"] > most:
            best, most = r, c["consensus"]
    if best >= 0 and most < min_consensus:
        best = -1
    if best < 0:
        return -1, -1, np.eye(4, dtype=F32), SRT_EYE.copy()
    return best, cands[best]["kf"], cands[best]["S12"], cands[best]["srt"]


def sim3(kps, desc, bow, q_mp, q_valid, q_Tcw, store, cand_slots, tr, K, nlevels, scale, min_consensus=20, **prm):
    """The query frame of one sequence, with its own map points and pose, against the ring slots cand_slots of a
    reloc_reference.Keyframes -> dict(cands = per rank dict(kf, rows, consensus, flags, winner, S12, srt, inlier, margin);
    best_rank, best_kf, best_S12, best_srt). prm: sim3_reference.ransac's hypotheses, fixed_scale, chi2_max, seed."""
    inv_sigma2 = oracle.scale_factors(nlevels, scale)[3]
    cands = []
    for slot in cand_slots:
        slot = int(slot)
        kf = store.kfs[slot] if 0 <= slot < store.capacity else None
        cands.append(absent() if kf is None else solve_one(kps, desc, bow, q_mp, q_valid, q_Tcw, kf, tr, K, inv_sigma2, prm))
    rank, kf_id, S12, srt = select(cands, min_consensus)
    return dict(cands=cands, best_rank=rank, best_kf=kf_id, best_S12=S12, best_srt=srt)
