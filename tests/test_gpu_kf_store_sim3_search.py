"""GPU tests (pytest -m gpu) of the keyframe store's SearchBySim3 query (tb_kf_store_sim3_search_dev, include/tb_capi.h) against
tests/reloc_sim3_search_reference.py, on the fixture of tests/sim3_search_cases.py (a query whose map drifted with its pose, a third
of its keys refused by searchByBow) in a store with S = 2, capacity 2 and pitch 256, filled as test_gpu_kf_store_pnp fills its own:
relocalize, then sim3, then the search under the RANSAC's own cand_srt.

Everything the search writes is EQUAL to the composition (integers and the verification's match records). The refinement on the
widened lists: rows exact, the optimiser's outputs to tests/test_gpu_sim3_opt.py's bounds through test_gpu_kf_store_sim3_refine.check
(1e-6 relative; counts, flags, inlier count and mask exact), with the reference's margins asserted first and that file's 2 + 2
iterations, for its reason: at the defaults these problems reach the rounding floor of chi2."""
import numpy as np
import pytest
import torch

import oracle
import reloc_sim3_reference as rs
import reloc_sim3_search_reference as rss
import sim3_search_cases as cs
import sim3_search_reference as ss
import test_gpu_kf_store_pnp as kp
import test_gpu_kf_store_sim3 as ks
import vo_bow_reference as vb
from test_gpu_kf_store import K, NLEVELS, SCALE, TR, _pack_frames
from test_gpu_kf_store_sim3_graph import _np, _relocalize, _snapshot
from test_gpu_kf_store_sim3_refine import MIN_INL, OPT, check
from test_gpu_vo_desc import _same_bits
from trackingbench_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

S, CAP, PITCH = cs.S, cs.CAP, cs.PITCH
assert (S, CAP, PITCH, cs.N) == (kp.S, kp.CAP, kp.PITCH, kp.N) and np.array_equal(cs.CANDS, kp.CANDS)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _views(d):
    """the lent views, copied while they hold this call's bytes"""
    return {k: v.clone().cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def ran(ctx):
    case = cs.build_case(synth.vocabulary(1, 10, 5))
    q = _pack_frames(case["queries"], PITCH, 55)
    cands = torch.from_numpy(cs.CANDS).cuda()
    mp, valid, Tq = ks._query_map(case)
    args = (K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands)
    sargs = (K, cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE, q[0], q[1], q[2], mp, valid, Tq, cands)
    out = {}

    def sim3(st):
        o = st.sim3(*args, min_consensus=ks.MIN_CONS, **ks.PRM)
        ctx.synchronize()
        return o

    def refine(st, win):
        o = st.sim3_refine(*args, win, min_inliers=MIN_INL, **OPT)
        ctx.synchronize()
        return _np(o), _views(st.sim3_refine_state("cuda", 2))

    def search(st, win, **kw):
        o = st.sim3_search(*sargs, win, **kw)
        ctx.synchronize()
        return _np(o), _views(st.sim3_search_state("cuda", 2))

    st, rings = kp._fill(ctx, case)
    try:
        reloc = _relocalize(st, q, cands)
        out["rc_before_sim3"] = st.sim3_search_rc(*sargs, None)[0]
        with pytest.raises(capi.TBError) as early:
            st.sim3_search_state("cuda", 2)
        out["early_state"] = early.value.code
        win = sim3(st)
        out["rc_not_own"] = st.sim3_search_rc(*sargs, None)[0]          # that query wrote cand_srt into the caller's tensors
        out["base"] = refine(st, win)                                   # the refinement without any search
        before = _snapshot(ctx, st, dict(reloc=reloc, win=win))
        out["s0"] = search(st, win, use_for_refine=False)
        after0 = _snapshot(ctx, st, dict(reloc=reloc, win=win))
        out["r0"] = refine(st, win)
        out["s1"] = search(st, win, use_for_refine=True)
        after1 = _snapshot(ctx, st, dict(reloc=reloc, win=win))
        out["r1"] = refine(st, win)
        out["r1_again"] = refine(st, win)
        after2 = _snapshot(ctx, st, dict(reloc=reloc, win=win))
        out["snap"] = (before, after0, after1, after2)
        out["s_refined"] = search(st, dict(win, cand_srt=torch.from_numpy(out["r1"][0]["cand_srt"]).cuda()), use_for_refine=False)
        out["r_after_plain_search"] = refine(st, win)                   # use_for_refine = 0 dropped the widened lists again
        out["s_low"] = search(st, dict(win, cand_consensus=torch.full_like(win["cand_consensus"], 2)), use_for_refine=True)
        out["r_low"] = refine(st, dict(win, cand_consensus=torch.full_like(win["cand_consensus"], 2)))
        search(st, win, use_for_refine=True)
        win2 = sim3(st)                                                 # a new Sim(3) query drops the widened lists
        out["r_after_sim3"] = refine(st, win2)
        search(st, win2, use_for_refine=True)
        _relocalize(st, q, cands)                                       # and after a verification neither may run
        out["rc_refine_after_relocalize"] = st.sim3_refine_rc(*args, win2, **OPT)[0]
        out["rc_search_after_relocalize"] = st.sim3_search_rc(*sargs, win2)[0]
        win3 = sim3(st)
        bad = [dict(th=0.0), dict(th=float("nan")), dict(th_high=-1), dict(th_high=257), dict(use_for_refine=2), dict(ncand=1), dict(ncand=3),
               dict(q_pitch=PITCH + 1), dict(q_pitch=0)]
        out["errs"] = [st.sim3_search_rc(*sargs, win3, **b)[0] for b in bad]
        out["errs"] += [st.sim3_search_rc(K, 0, cs.HEIGHT, *sargs[3:], win3)[0], st.sim3_search_rc(K, cs.WIDTH, -1, *sargs[3:], win3)[0],
                        st.sim3_search_rc((0.0, 360.0, 320.0, 120.0), *sargs[1:], win3)[0], st.sim3_search_rc(*sargs[:3], 17, *sargs[4:], win3)[0]]
        out["after_all"] = search(st, win3, use_for_refine=False)
        st.clear()
        out["rc_cleared"] = st.sim3_search_rc(*sargs, win)[0]
        out["win"] = _np(win)
        ctx.synchronize()
    finally:
        st.close()
    # the composition
    inv = oracle.scale_factors(NLEVELS, SCALE)[3]
    exp = {}
    for s in range(S):
        kps, desc, bow = case["queries"][s]
        for r, slot in enumerate(cs.CANDS[s]):
            kf = rings[s].kfs[slot] if slot >= 0 else None
            if kf is None:
                exp[(s, r)] = dict(rss.skipped(len(kps), 0), kf=None)
                continue
            m = vb.match(kps, desc, bow, kf, TR)
            c = rs.solve_one(kps, desc, bow, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, TR, K, inv, ks.PRM, matches=m)
            o = rss.search_one(kps, desc, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, m, c, c["srt"], K, cs.WIDTH, cs.HEIGHT,
                               NLEVELS, SCALE)
            f = rss.refine_widened(kps, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, o["widened"], c["srt"], K, inv, **OPT)
            again = rss.search_one(kps, desc, case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], kf, m, c, out["r1"][0]["cand_srt"][s, r], K,
                                   cs.WIDTH, cs.HEIGHT, NLEVELS, SCALE)      # under the bits the GPU's refinement returned
            exp[(s, r)] = dict(o, kf=kf, sim3=c, refined=f, again=again)
    out["exp"], out["case"] = exp, case
    return out


def test_everything_the_search_writes_equals_the_composition(ran):
    for key in ("s0", "s1"):
        g, st = ran[key]
        for (s, r), e in ran["exp"].items():
            p, w = 2 * s + r, (key, s, r)
            n1, n2, npair, nw = len(e["match1"]), len(e["match2"]), len(e["pairs"]), len(e["widened"])
            assert np.array_equal(g["cand_stats"][s, r], e["stats"]), (w, g["cand_stats"][s, r], e["stats"])
            assert g["cand_new"][s, r] == npair == st["pair_counts"][p] and g["cand_total"][s, r] == nw == st["widened_counts"][p], w
            assert np.array_equal(st["match1"][p, :n1], e["match1"]) and (st["match1"][p, n1:] == -1).all(), w
            assert np.array_equal(st["match2"][p, :n2], e["match2"]) and (st["match2"][p, n2:] == -1).all(), w
            assert np.ascontiguousarray(st["pairs"][p, :npair]).tobytes() == e["pairs"].tobytes(), w
            assert np.ascontiguousarray(st["widened"][p, :nw]).tobytes() == e["widened"].tobytes(), w
        for s in range(S):
            rank = ran["win"]["best_rank"][s]
            assert rank >= 0 and g["best_new"][s] == g["cand_new"][s, rank] and g["best_total"][s] == g["cand_total"][s, rank]
    for k in ran["s0"][0]:
        assert ran["s0"][0][k].tobytes() == ran["s1"][0][k].tobytes(), k
    for k in ran["s0"][1]:
        assert ran["s0"][1][k].tobytes() == ran["s1"][1][k].tobytes() == ran["after_all"][1][k].tobytes(), k
    # what the case is there for: the far keyframes gain the pairs the CPU test measured, all of them true correspondences
    case = ran["case"]
    for (s, r), floor in (((0, 0), 8), ((1, 1), 8)):
        p = ran["exp"][(s, r)]["pairs"]
        qi, ki = case["q_ids"][s], case["kf_ids"][0][s]
        assert len(p) >= floor and all(qi[a] >= 0 and qi[a] == ki[b] for a, b in zip(p["queryIdx"], p["trainIdx"]))


def test_the_skips(ran):
    g, st = ran["s1"]
    assert g["cand_stats"][0, 1].tolist() == [0] * 7 + [ss.FLAG_SKIPPED] and g["cand_new"][0, 1] == 0 and g["cand_total"][0, 1] == 0   # no candidate
    assert (st["match1"][1] == -1).all() and (st["match2"][1] == -1).all()
    g, st = ran["s_low"]                                                # every consensus below 3
    assert (g["cand_stats"][..., 7] == ss.FLAG_SKIPPED).all() and not g["cand_stats"][..., :7].any()
    assert not g["cand_new"].any() and not g["cand_total"].any() and not g["best_new"].any() and not g["best_total"].any()
    assert (st["match1"] == -1).all() and (st["match2"] == -1).all() and not st["widened_counts"].any()
    r, rst = ran["r_low"]                                               # and the refinement on those lists skips as it always did
    assert (r["cand_stats"][..., 7] == 2).all() and not rst["row_counts"].any()


def test_the_search_changes_nothing_else(ran):
    before = ran["snap"][0]
    for snap in ran["snap"][1:]:
        assert before.keys() == snap.keys()
        for k in before:
            assert before[k] == snap[k], k


def test_without_use_for_refine_the_refinement_is_what_it_was(ran):
    base, bst = ran["base"]
    for key in ("r0", "r_after_plain_search", "r_after_sim3"):
        g, st = ran[key]
        for k, v in base.items():
            assert g[k].tobytes() == v.tobytes(), (key, k)
        assert np.array_equal(st["row_counts"], bst["row_counts"]), key
        for p, n in enumerate(bst["row_counts"]):      # what lies beyond a pair's count is whatever an earlier call left there
            for k in ("rows", "active", "inlier"):
                assert st[k][p, :n].tobytes() == bst[k][p, :n].tobytes(), (key, k, p)


def test_with_use_for_refine_the_refinement_runs_on_the_widened_rows(ran):
    g, st = ran["r1"]
    for k in g:
        assert g[k].tobytes() == ran["r1_again"][0][k].tobytes(), k
    for (s, r), e in ran["exp"].items():
        p, tag = 2 * s + r, (s, r)
        if not e["ran"]:
            assert st["row_counts"][p] == 0 and g["cand_stats"][s, r, 7] == 2, tag
            continue
        f = e["refined"]
        n = len(f["rows"])
        assert f["margins"][0] > 1e-9 and f["margins"][1] > 1e-4, (tag, f["margins"])
        assert st["row_counts"][p] == n == len(e["widened"]), tag
        assert _same_bits(st["rows"][p, :n], f["rows"].view(np.float32).reshape(-1, 12)), tag
        assert (st["active"][p] == 1).all(), tag
        check(dict(srt=g["cand_srt"][s, r], S12=g["cand_S12"][s, r], inliers=g["cand_inliers"][s, r], stats=g["cand_stats"][s, r]), f, tag)
        if f["stats"][7] == 0:
            assert np.array_equal(st["inlier"][p, :n], f["mask"]) and not st["inlier"][p, n:].any(), tag
    for s in range(S):
        rank = ran["win"]["best_rank"][s]
        for k in ("srt", "S12", "inliers", "stats"):
            assert g["best_" + k][s].tobytes() == g["cand_" + k][s, rank].tobytes(), (s, k)
    # more rows and more inliers than the refinement on the RANSAC's inliers alone
    b, bst = ran["base"]
    for (s, r) in ((0, 0), (1, 1)):
        p = 2 * s + r
        print("pair %s: RANSAC inliers %d, refined inliers %d, widened rows %d, refined inliers on them %d" %
              ((s, r), ran["win"]["cand_consensus"][s, r], b["cand_inliers"][s, r], st["row_counts"][p], g["cand_inliers"][s, r]))
        assert g["cand_inliers"][s, r] > b["cand_inliers"][s, r]
    # searching again under the refined transform: the composition under the same srt bits
    g2, st2 = ran["s_refined"]
    for (s, r), e in ran["exp"].items():
        if e["ran"]:
            p, a = 2 * s + r, e["again"]
            assert np.array_equal(g2["cand_stats"][s, r], a["stats"]) and np.array_equal(st2["match1"][p, :len(a["match1"])], a["match1"]), (s, r)
            assert np.ascontiguousarray(st2["widened"][p, :len(a["widened"])]).tobytes() == a["widened"].tobytes(), (s, r)


def test_state_and_argument_errors(ran):
    assert ran["rc_before_sim3"] == ran["early_state"] == ran["rc_not_own"] == ran["rc_cleared"] == capi.TB_ESTATE
    assert ran["rc_refine_after_relocalize"] == ran["rc_search_after_relocalize"] == capi.TB_ESTATE
    assert ran["errs"] == [capi.TB_EINVAL] * len(ran["errs"])
