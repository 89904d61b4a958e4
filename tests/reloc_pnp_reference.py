"""CPU composition of candidate verification with PnP in front of the pose stage -- the yardstick of tb_relocalize_batch_dev on a
store that called tb_kf_store_pnp_enable (include/tb_capi.h): reloc_reference.py's stages with pnp_reference.py between rows and
pose.

    vo_bow_reference.match -> vo_desc_reference.carry / rows                      (as reloc_reference.verify_one)
      -> pnp_reference.ransac on the rows, the stored pose as the prior
      -> consensus >= min_consensus: the consensus rows in key order, oracle.pose_opt seeded with the PnP pose (float32)
         otherwise:                  every row, oracle.pose_opt seeded with the stored pose -- reloc_reference's candidate
      -> expand, on the PnP path:    every original row that is an inlier of the optimised pose (pnp_reference.inliers on the
                                     float32 pose), oracle.pose_opt once more, seeded with the optimised pose

then reloc_reference.select, unchanged."""
import numpy as np

import oracle
import pnp_reference as pr
import reloc_reference as rr
import vo_bow_reference as vb
import vo_desc_reference as vd

F32 = np.float32
F64 = np.float64
PNP_DEFAULTS = dict(hypotheses=256, chi2_max=5.991, seed=0, min_consensus=10, expand=1)


def absent():
    c = rr.absent()
    c.update(rows0=np.zeros(0, oracle.OBS), consensus=0, winner=(-2, 0), pnp_flags=1, pnp_Tcw=rr.EYE.copy(), took=0, seed=rr.EYE.copy(), margin=np.inf, expand_margin=np.inf)
    return c


def recount(Tcw, obs, K, chi2_max):
    """(mask, margin): the rows of obs that are inliers of the float32 pose Tcw, by the RANSAC's rule, and the smallest relative
    distance of a row's chi2 from chi2_max -- the pose comes out of PoseOptimization, which two solvers agree on to 1e-6 only"""
    T = np.asarray(Tcw, F32).reshape(4, 4).astype(F64)
    R = [[T[i, j] for j in range(3)] for i in range(3)]
    t = [T[i, 3] for i in range(3)]
    with np.errstate(all="ignore"):
        z, c = pr.row_chi2(R, t, pr._rows64(obs, len(obs)), K)
        mask = (z > 0) & (c <= F64(chi2_max))
    c = c[np.isfinite(c)]
    return mask, (float(np.min(np.abs(c - chi2_max)) / chi2_max) if len(c) else np.inf)


def verify_one(kps, desc, bow, kf, tr, K, inv_sigma2, pnp, matches=None):
    """One candidate with PnP: reloc_reference.verify_one's dict plus rows0 (the rows before the gather), consensus, winner,
    pnp_flags, pnp_Tcw, took, seed (what the first pose stage started from), first (the first pose stage's rows, pose and inliers), margin
    (pnp_reference.margin of the RANSAC) and expand_margin (recount's)."""
    p = dict(PNP_DEFAULTS, **pnp)
    m = len(kps)
    if matches is None:
        matches = vb.match(kps, desc, bow, kf, tr) if m and len(kf["orb"]) else np.zeros(0, oracle.MATCH)
    mp, valid = vd.carry(matches, m, kf["mp"], kf["valid"])
    rows0 = vd.rows(kps, mp, valid, inv_sigma2)
    r = pr.ransac(K, rows0, len(rows0), p["hypotheses"], p["chi2_max"], p["seed"], kf["Tcw"])
    took = int(r["consensus"] >= p["min_consensus"])
    obs = rows0[r["inlier"] != 0] if took else rows0
    seed = r["Tcw32"] if took else kf["Tcw"]
    n_inl, Tcw, outl, _ = oracle.pose_opt(K, seed, obs)
    Tcw = np.asarray(Tcw, F32).reshape(4, 4).copy()
    first = dict(obs=obs, Tcw=Tcw, n_inliers=int(n_inl))
    expand_margin = np.inf
    if took and p["expand"]:
        mask, expand_margin = recount(Tcw, rows0, K, p["chi2_max"])
        obs = rows0[mask]
        n_inl, T2, outl, _ = oracle.pose_opt(K, Tcw, obs)
        Tcw = np.asarray(T2, F32).reshape(4, 4).copy()
    return dict(kf=kf["kf_id"], matches=matches, obs=obs, n_inliers=int(n_inl), outlier=outl, Tcw=Tcw, rows0=rows0,
                consensus=r["consensus"], winner=r["winner"], pnp_flags=r["flags"], pnp_Tcw=r["Tcw32"], took=took,
                seed=np.asarray(seed, F32).reshape(4, 4).copy(), margin=pr.margin(r, p["chi2_max"]), first=first, expand_margin=expand_margin)


def relocalize(kps, desc, bow, store, cand_slots, tr, K, nlevels, scale, min_inliers=50, pnp=None):
    """reloc_reference.relocalize with PnP verification: the query frame of one sequence against the ring slots cand_slots"""
    inv_sigma2 = oracle.scale_factors(nlevels, scale)[3]
    cands = []
    for slot in cand_slots:
        slot = int(slot)
        kf = store.kfs[slot] if 0 <= slot < store.capacity else None
        cands.append(absent() if kf is None else verify_one(kps, desc, bow, kf, tr, K, inv_sigma2, pnp or {}))
    rank, kf_id, Tcw = rr.select(cands, min_inliers)
    return dict(cands=cands, best_rank=rank, best_kf=kf_id, best_Tcw=Tcw)
