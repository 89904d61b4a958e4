"""CPU tests of the SearchBySim3 definition (tests/sim3_search_reference.py) and of the store composition around it
(tests/reloc_sim3_search_reference.py) on the fixture of tests/sim3_search_cases.py: a query whose map drifted together with its
pose, a third of its keys with 64 flipped bits (searchByBow refuses them), against the store of test_gpu_kf_store_sim3.

Measured on the fixture under the true similarity (and the same under the RANSAC's): the far keyframe of sequence 0 gives 15 new
pairs, that of sequence 1 gives 16, the keyframe with five points gives 1; every one joins two views of one scene point. The floors
below are half of the two large counts.

The level prediction: ORB-SLAM's ceil(log(maxD / d) / log(1.25)) is never below 0 once the range test d <= 1.2 maxD has passed
(log(1 / 1.2) / log(1.25) = -0.82), so "the clamp at 0" is the case d > maxD, where the quotient is negative and the level is 0; the
clamp at nlevels - 1 is the case g[nlevels - 1] d < maxD, where no level of the table qualifies."""
import numpy as np
import pytest

import oracle
import reloc_sim3_reference as rs
import reloc_sim3_search_reference as rss
import sim3_reference as sr
import sim3_search_cases as cs
import sim3_search_reference as ss
import vo_bow_reference as vb
from test_gpu_kf_store import K, NLEVELS, SCALE, TR
from trackingbench_slam_amd import synth

PRM = dict(hypotheses=256, fixed_scale=False, chi2_max=sr.CHI2_MAX, seed=3)
FLOOR = {(0, 0): 8, (1, 1): 8}      # (sequence, rank) -> half of the measured 15 and 16


@pytest.fixture(scope="module")
def case():
    return cs.build_case(synth.vocabulary(1, 10, 5))


@pytest.fixture(scope="module")
def ran(case):
    """(sequence, rank) -> the composition of one pair under the TRUE similarity, with the RANSAC's dict and the match list"""
    inv = oracle.scale_factors(NLEVELS, SCALE)[3]
    out = {}
    for s in range(cs.S):
        kps, desc, bow = case["queries"][s]
        for r, slot in enumerate(cs.CANDS[s]):
            if slot < 0:
                continue
            kf, T, kid = case["adds"][slot][s]
            kf = dict(kf, Tcw=np.asarray(T, np.float32).reshape(4, 4), kf_id=kid)
            m = vb.match(kps, desc, bow, kf, TR)
            c = rs.solve_one(kps, desc, bow, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, TR, K, inv, PRM, matches=m)
            o = rss.search_one(kps, desc, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, m, c, cs.truth_srt(case["truth"][s]), K,
                               cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)
            out[(s, r)] = dict(o, sim3=c, matches=m, slot=int(slot), kf=kf)
    return out


def test_the_drifted_camera_points_project_onto_the_keys(case):
    for s in range(cs.S):
        Xc = rs.apply(case["q_Tcw"][s], case["q_mp"][s]).astype(np.float64)
        kps = case["queries"][s][0]
        ok = case["q_ids"][s] >= 0
        u = K[0] * Xc[:, 0] / Xc[:, 2] + K[2]
        v = K[1] * Xc[:, 1] / Xc[:, 2] + K[3]
        assert np.abs(u - kps["x"])[ok].max() < 2.5 and np.abs(v - kps["y"])[ok].max() < 2.5     # the view's 0.5 px noise, 5 sigma


def test_searchbybow_refuses_the_heavy_keys_and_they_stay_under_th_high(case, ran):
    for (s, r), o in ran.items():
        heavy = set(case["heavy"][s].tolist())
        assert not heavy & set(o["matches"]["queryIdx"].tolist())
        where = {int(p): j for j, p in enumerate(case["kf_ids"][o["slot"]][s])}
        d = [ss.hamming(case["queries"][s][1][i], o["kf"]["desc"][where[int(case["q_ids"][s][i])]][None])[0] for i in heavy
             if case["q_ids"][s][i] >= 0]
        assert 50 < min(d) and max(d) < ss.TH_HIGH
        assert abs(len(heavy) - cs.N / 3) < 2


def test_every_new_pair_is_a_true_correspondence_and_the_floor(case, ran):
    for (s, r), o in ran.items():
        assert o["ran"] and o["stats"][7] == 0
        qi, ki = case["q_ids"][s], case["kf_ids"][o["slot"]][s]
        p = o["pairs"]
        print("sequence %d rank %d: %d new pairs, %d inlier rows, widened %d" % (s, r, len(p), int(o["sim3"]["inlier"].sum()), len(o["widened"])))
        assert all(qi[a] >= 0 and qi[a] == ki[b] for a, b in zip(p["queryIdx"], p["trainIdx"]))
        assert (np.diff(p["queryIdx"]) > 0).all() and o["stats"][6] == len(p)
        assert len(p) >= FLOOR.get((s, r), 0)
        assert ((p["distance"] >= 0) & (p["distance"] <= ss.TH_HIGH)).all()
        # the heavy keys are what the search is there for
        assert len(set(p["queryIdx"].tolist()) & set(case["heavy"][s].tolist())) >= FLOOR.get((s, r), 0) // 2


def test_no_already_matched_key_reappears_and_the_merge(ran):
    for o in ran.values():
        m1, m2 = o["side1"]["matched"], o["side2"]["matched"]
        assert m1.sum() == m2.sum() == o["sim3"]["inlier"].sum() > 0
        assert not m1[o["pairs"]["queryIdx"]].any() and not m2[o["pairs"]["trainIdx"]].any()
        assert (o["match1"][m1] == -1).all() and (o["match2"][m2] == -1).all()
        w = o["widened"]
        assert len(w) == m1.sum() + len(o["pairs"]) and (np.diff(w["queryIdx"]) > 0).all()
        assert len(np.unique(w["trainIdx"])) == len(w)


def test_every_skip_reason_occurs(case, ran):
    o = ran[(0, 0)]
    w1, w2 = o["why"]
    cr = case["crafted"]
    assert w1[cr["behind"]] == ss.BEHIND and w1[cr["outside"]] == ss.OUTSIDE
    both = np.concatenate([w1, w2])
    for reason in (ss.BEHIND, ss.OUTSIDE, ss.RANGE, ss.NO_CANDIDATE, ss.TOO_FAR, ss.OK, ss.NOT_TRIED):
        assert (both == reason).any(), reason
    # not mutual, and among them a stored point displaced by metres: the query key finds the stored key, whose own point leads elsewhere
    m1, m2 = o["match1"], o["match2"]
    lost = [i for i in range(len(m1)) if m1[i] >= 0 and m2[m1[i]] != i]
    assert lost
    kf, ids, scene = o["kf"], case["kf_ids"][0][0], case["scenes"][0]
    moved = [i for i in lost if kf["valid"][m1[i]] and np.linalg.norm(kf["mp"][m1[i]] - scene[ids[m1[i]]]) > 1.0]
    assert moved
    # the stats count what why says
    st = o["stats"]
    assert st[0] == (w1 != ss.NOT_TRIED).sum() and st[1] == np.isin(w1, (ss.OK, ss.NO_CANDIDATE, ss.TOO_FAR)).sum()
    assert st[4] == (m1 >= 0).sum() and st[5] == (m2 >= 0).sum()


def test_the_level_clamps_occur(ran):
    g = ss.level_px(NLEVELS, SCALE).astype(np.float64)
    low = high = 0
    for o in ran.values():
        for lev, geom in zip(o["level"], o["geom"]):
            reached = lev >= 0
            low += int(((lev == 0) & (geom[:, 1] > geom[:, 0]))[reached].sum())
            high += int(((lev == NLEVELS - 1) & (g[-1] * geom[:, 1] < geom[:, 0]))[reached].sum())
            # the comparisons against the table are ORB-SLAM's ceil(log(maxD / d) / log(1.25)) clamped, away from the table's own rounding
            ratio = geom[reached, 0] / geom[reached, 1]
            orb = np.clip(np.ceil(np.log(ratio) / np.log(1.25)), 0, NLEVELS - 1)
            away = np.abs(np.log(ratio) / np.log(1.25) - np.round(np.log(ratio) / np.log(1.25))) > 1e-6
            assert (orb[away] == lev[reached][away]).all()
    assert low > 0 and high > 0


def test_a_tie_goes_to_the_lower_index(case, ran):
    o, cr = ran[(0, 0)], case["crafted"]
    kf = o["kf"]
    assert cr["tie_low"] < cr["tie_high"] and np.array_equal(kf["desc"][cr["tie_low"]], kf["desc"][cr["tie_high"]])
    assert o["why"][0][cr["tie_query"]] == ss.OK and o["match1"][cr["tie_query"]] == cr["tie_low"]
    # with the two stored keys exchanged the other index wins: the index decides, not the order of a scan
    s2 = dict(o["side2"])
    perm = np.arange(len(s2["keys"]))
    perm[[cr["tie_low"], cr["tie_high"]]] = perm[[cr["tie_high"], cr["tie_low"]]]
    s2 = {k: v[perm] for k, v in s2.items()}
    again = ss.search(o["side1"], s2, cs.truth_srt(case["truth"][0]), K, cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)
    assert again["match1"][cr["tie_query"]] == cr["tie_low"]


def test_malformed_problems_and_skips(case, ran):
    o = ran[(0, 0)]
    srt = cs.truth_srt(case["truth"][0])
    for bad in (0.0, -1.0, np.nan, np.inf):
        r = ss.search(o["side1"], o["side2"], np.concatenate([srt[:7], [bad]]), K, cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)
        assert r["stats"].tolist() == [0] * 7 + [ss.FLAG_MALFORMED] and (r["match1"] == -1).all() and len(r["pairs"]) == 0
    s1 = dict(o["side1"], keys=o["side1"]["keys"].copy())
    s1["keys"]["octave"][7] = NLEVELS
    assert ss.search(s1, o["side2"], srt, K, cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)["stats"][7] == ss.FLAG_MALFORMED
    # the store's skips: no candidate, a consensus below 3
    kps, desc, _ = case["queries"][0]
    a = rss.search_one(kps, desc, case["q_mp"][0], case["q_valid"][0], case["q_Tcw"][0], None, None, rs.absent(), srt, K, cs.WIDTH, cs.HEIGHT,
                       NLEVELS, SCALE)
    b = rss.search_one(kps, desc, case["q_mp"][0], case["q_valid"][0], case["q_Tcw"][0], o["kf"], o["matches"], dict(o["sim3"], consensus=2), srt,
                       K, cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)
    for r in (a, b):
        assert not r["ran"] and r["stats"].tolist() == [0] * 7 + [ss.FLAG_SKIPPED] and len(r["pairs"]) == 0 and len(r["widened"]) == 0


def test_the_widened_rows_refine_no_worse(case, ran):
    """what the search is for: OptimizeSim3 from the RANSAC's srt on the widened rows, all active, keeps at least the RANSAC's inliers"""
    inv = oracle.scale_factors(NLEVELS, SCALE)[3]
    for (s, r) in FLOOR:
        o = ran[(s, r)]
        f = rss.refine_widened(case["queries"][s][0], case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], o["kf"], o["widened"],
                               o["sim3"]["srt"], K, inv)
        print("sequence %d rank %d: consensus %d, widened rows %d, refined inliers %d" % (s, r, o["sim3"]["consensus"], len(f["rows"]), f["inliers"]))
        assert len(f["rows"]) == len(o["widened"]) and f["stats"][7] == 0
        assert f["inliers"] >= o["sim3"]["consensus"]
