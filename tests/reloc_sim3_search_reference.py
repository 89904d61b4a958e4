"""CPU composition of the keyframe store's SearchBySim3 query -- the yardstick of tb_kf_store_sim3_search_dev (include/tb_capi.h),
built on reloc_sim3_reference (the Sim(3) query's composition), sim3_search_reference (the operator's definition) and
reloc_sim3_opt_reference / sim3_opt_reference (what the refinement then runs on):

    reloc_sim3_reference.solve_one per candidate (rows, RANSAC: cand_srt, consensus, mask)
      -> prep: the camera points of both sides as the row kernel forms X1 and X2 (reloc_sim3_reference.apply) for EVERY key; a key
         is `already matched` if it belongs to a row whose RANSAC mask is 1; a pair with no candidate or with a consensus below 3
         (a flagged Sim(3) output has consensus 0) is skipped: stats flag 2, no pairs
      -> sim3_search_reference.search under cand_srt (or the srt the caller passes)
      -> merge: the RANSAC-inlier rows' matches united with the new pairs, in ascending query key, one entry a key
      -> (use_for_refine) the pixel rows of the widened list by the row rule, every row active, sim3_opt_reference.optimize"""
import numpy as np

import oracle
import reloc_sim3_opt_reference as ro
import reloc_sim3_reference as rs
import sim3_opt_reference as so
import sim3_search_reference as ss

F32 = np.float32


def row_keys(matches, q_kps, q_valid, kf):
    """the row rule's selection: (query keys sel in ascending order, the index k into matches of each)"""
    m, nk = len(q_kps), len(kf["orb"])
    win = np.full(m, -1, np.int64)
    for k, (q, tr) in enumerate(zip(matches["queryIdx"], matches["trainIdx"])):
        if 0 <= q < m and 0 <= tr < nk and kf["valid"][tr] and q_valid[q]:
            win[q] = k
    sel = np.nonzero(win >= 0)[0]
    return sel, win[sel]


def skipped(n1, n2):
    st = np.zeros(8, np.int32)
    st[7] = ss.FLAG_SKIPPED
    return dict(match1=np.full(n1, -1, np.int32), match2=np.full(n2, -1, np.int32), pairs=np.zeros(0, oracle.MATCH), stats=st,
                widened=np.zeros(0, oracle.MATCH), ran=False)


def sides(q_kps, q_desc, q_mp, q_valid, q_Tcw, kf, matches, inlier):
    """prep -> (side1, side2, the inlier rows' match records)"""
    sel, k = row_keys(matches, q_kps, q_valid, kf)
    inl = np.asarray(inlier).astype(bool)[:len(sel)]
    m1, m2 = np.zeros(len(q_kps), bool), np.zeros(len(kf["orb"]), bool)
    kept = matches[k[inl]]
    m1[sel[inl]] = True
    m2[kept["trainIdx"]] = True
    s1 = ss.side(q_kps, q_desc, rs.apply(q_Tcw, q_mp), q_valid, m1)
    s2 = ss.side(kf["orb"], kf["desc"], rs.apply(kf["Tcw"], kf["mp"]), kf["valid"], m2)
    return s1, s2, kept


def search_one(q_kps, q_desc, q_mp, q_valid, q_Tcw, kf, matches, cand, srt, K, width, height, nlevels, scale, th=ss.TH, th_high=ss.TH_HIGH):
    """one pair: cand = reloc_sim3_reference.solve_one's dict (None kf: absent). -> the operator's outputs, widened (MATCH records in
    ascending query key), the two sides and ran"""
    n1 = len(q_kps)
    if kf is None or cand["kf"] < 0 or cand["consensus"] < 3:
        return skipped(n1, 0 if kf is None else len(kf["orb"]))
    s1, s2, kept = sides(q_kps, q_desc, q_mp, q_valid, q_Tcw, kf, matches, cand["inlier"])
    r = ss.search(s1, s2, srt, K, width, height, nlevels, scale, th, th_high)
    wide = np.concatenate([kept, r["pairs"]])
    wide = wide[np.argsort(wide["queryIdx"], kind="stable")]
    assert len(np.unique(wide["queryIdx"])) == len(wide)
    return dict(r, widened=wide, side1=s1, side2=s2, ran=True)


def refine_widened(q_kps, q_mp, q_valid, q_Tcw, kf, widened, srt, K, inv_sigma2, **opt):
    """what tb_kf_store_sim3_refine_dev runs on after a search with use_for_refine: the pixel rows of the widened list, all active"""
    rows3 = rs.rows(widened, q_kps, q_mp, q_valid, q_Tcw, kf, inv_sigma2)
    rows = ro.pixel_rows(widened, q_kps, q_valid, kf, rows3)
    trace, gates = [], []
    o = so.optimize(K, rows, len(rows), srt, active=np.ones(len(rows), np.uint8), trace=trace, gates=gates, **opt)
    return dict(rows=rows, srt=o["srt"], S12=o["S12"], inliers=o["inliers"], stats=o["stats"], mask=o["mask"],
                margins=so.margins(trace, gates, opt.get("th2", so.TH2)))
