"""CPU composition of the keyframe store's Sim(3) refinement -- the yardstick of tb_kf_store_sim3_refine_dev (include/tb_capi.h),
built on reloc_sim3_reference (the Sim(3) query's composition) and sim3_opt_reference (the optimiser's definition):

    reloc_sim3_reference.solve_one per candidate (rows, RANSAC: cand_srt, consensus, mask)
      -> pixel rows: the same matches in the same order, with the two keys' x, y as (u1, v1), (u2, v2)
      -> a pair with no candidate or a consensus below 3 is skipped: the identity, no inliers, stats[7] = 2
      -> sim3_opt_reference.optimize from cand_srt on the RANSAC's mask
      -> the candidate reloc_sim3_reference.select chose: its four outputs (the identity and stats[7] = 2 when none); the srt the
         graph query would read: the refined one where use_for_graph, the candidate ran and its inliers reach min_inliers"""
import numpy as np

import oracle
import reloc_sim3_reference as rs
import sim3_opt_reference as so
import vo_bow_reference as vb

FLAG_SKIPPED = 2.0


def pixel_rows(matches, q_kps, q_valid, kf, rows3):
    """the pixel rows of one pair: rows3 (reloc_sim3_reference.rows) with the pixels of the keys its rule selects"""
    m, nk = len(q_kps), len(kf["orb"])
    win = np.full(m, -1, np.int64)
    for k, (q, tr) in enumerate(zip(matches["queryIdx"], matches["trainIdx"])):
        if 0 <= q < m and 0 <= tr < nk and kf["valid"][tr] and q_valid[q]:
            win[q] = k
    sel = np.nonzero(win >= 0)[0]
    j = matches["trainIdx"][win[sel]]
    assert len(sel) == len(rows3)
    out = np.zeros(len(sel), so.OBS_ROW)
    for f in rows3.dtype.names:
        out[f] = rows3[f]
    out["u1"], out["v1"] = q_kps["x"][sel], q_kps["y"][sel]
    out["u2"], out["v2"] = kf["orb"]["x"][j], kf["orb"]["y"][j]
    return out


def skipped():
    st = np.zeros(8)
    st[7] = FLAG_SKIPPED
    return dict(srt=rs.SRT_EYE.copy(), S12=np.eye(4, dtype=np.float32), inliers=0, stats=st, mask=np.zeros(0, np.uint8),
                rows=np.zeros(0, so.OBS_ROW), margins=(np.inf, np.inf), ran=False)


def refine(kps, desc, bow, q_mp, q_valid, q_Tcw, store, cand_slots, tr, K, nlevels, scale, min_consensus, sim3_prm, min_inliers=20,
           use_for_graph=False, **opt):
    """One sequence -> dict(sim3 = reloc_sim3_reference's result, cands = per rank dict(rows, srt, S12, inliers, stats, mask, margins,
    ran), best_srt, best_S12, best_inliers, best_stats, keep_srt). opt: sim3_opt_reference.optimize's parameters."""
    inv_sigma2 = oracle.scale_factors(nlevels, scale)[3]
    first, cands = [], []
    for slot in cand_slots:
        slot = int(slot)
        kf = store.kfs[slot] if 0 <= slot < store.capacity else None
        if kf is None:
            first.append(rs.absent())
            cands.append(skipped())
            continue
        matches = vb.match(kps, desc, bow, kf, tr) if len(kps) and len(kf["orb"]) else np.zeros(0, oracle.MATCH)
        c = rs.solve_one(kps, desc, bow, q_mp, q_valid, q_Tcw, kf, tr, K, inv_sigma2, sim3_prm, matches=matches)
        first.append(c)
        rows = pixel_rows(matches, kps, q_valid, kf, c["rows"])
        if c["consensus"] < 3:
            cands.append(dict(skipped(), rows=rows))
            continue
        trace, gates = [], []
        o = so.optimize(K, rows, len(rows), c["srt"], active=c["inlier"], trace=trace, gates=gates, **opt)
        cands.append(dict(rows=rows, srt=o["srt"], S12=o["S12"], inliers=o["inliers"], stats=o["stats"], mask=o["mask"],
                          margins=so.margins(trace, gates, opt.get("th2", so.TH2)), ran=True))
    rank, kf_id, S12, srt = rs.select(first, min_consensus)
    b = cands[rank] if rank >= 0 else skipped()
    keep = b["srt"] if (use_for_graph and rank >= 0 and b["stats"][7] == 0 and b["inliers"] >= min_inliers) else srt
    return dict(sim3=dict(cands=first, best_rank=rank, best_kf=kf_id, best_S12=S12, best_srt=srt), cands=cands, best_srt=b["srt"],
                best_S12=b["S12"], best_inliers=b["inliers"], best_stats=b["stats"], keep_srt=np.asarray(keep, np.float64))
