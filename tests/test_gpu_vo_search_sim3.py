"""GPU tests (pytest -m gpu) of SearchBySim3 in the VO loop: StereoVO.search_sim3, tb_vo_search_sim3_dev, on the fixture of
tests/test_gpu_vo_refine_sim3.py (the out-and-back run at 640 x 240, S = 2, keyframes every 2, capacity 4, at the revisit, frame 6).

vo.relocalize(), vo.relocalize_sim3(), then vo.search_sim3() equals, bit for bit, the store-level call (KeyframeStore.sim3_search)
fed with the loop's own read-back ORB keys, descriptors, carried map points, pose and the verification's top_slot; no state tensor
of the loop, the store or the database changes; every step invalidates the query, and so does a verification after the Sim(3) query;
a loop stepped on after it ends in the same bytes as one that never asked. What the search finds on these rendered frames -- new
pairs, widened rows, refined inliers before and after -- is printed, not asserted (tests/test_gpu_kf_store_sim3_search.py holds the
query to the composition)."""
import numpy as np
import pytest

from test_gpu_vo_desc import _dev
from test_gpu_vo_loop import K, NF, S, _full, _vo, frames, voc  # noqa: F401 (fixtures)
from test_gpu_vo_recover import _same_seq
from test_gpu_vo_refine_sim3 import OPT
from test_gpu_vo_reloc_sim3 import CAP, RELOC, REVISIT, TOPK, _np, _same, _steps
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asked(frames, voc):
    """the loop run to the revisit, queried, and stepped on to the end"""
    vo = _vo(voc, CAP, None)
    out = {}
    try:
        vo.reset(frames["G0"])
        out["rc_before_a_step"] = vo.vo.search_sim3_dev(vo.dev, None)[0]
        _steps(vo, frames, 0, REVISIT + 1)
        reloc = _np(vo.relocalize(**RELOC))
        out["rc_without_sim3"] = vo.vo.search_sim3_dev(vo.dev, None)[0]
        with pytest.raises(capi.TBError) as e:
            vo.search_sim3()
        out["rc_wrapper_without_sim3"] = e.value.code
        win = vo.relocalize_sim3(fixed_scale=True, min_consensus=20, seed=7)
        out["refined_before"] = _np(vo.refine_sim3(fixed_scale=True, **OPT))
        vo.synchronize()
        before = _full(vo)
        out["plain"] = _np(vo.search_sim3(use_for_refine=False))
        vo.synchronize()
        after = _full(vo)
        out["state"] = {k: v.clone().cpu().numpy() for k, v in vo.store.sim3_search_state(vo.dev, TOPK).items()}
        # the store-level call fed from the loop's read-back state
        orb, desc, ocnt = vo.orb()
        mp, valid = vo.map_points()
        Tcw = vo.Tcw()
        top = _dev(reloc["top_slot"])
        vo.synchronize()
        p = vo.params
        o = vo.store.sim3_search(K, p.width, p.height, p.nlevels, p.scale, orb.contiguous(), desc.contiguous(), ocnt.contiguous(), mp.contiguous(),
                                 valid.contiguous(), Tcw.contiguous(), top.contiguous(), win, use_for_refine=False)
        vo.synchronize()                    # the store's call runs on the loop's stream
        out["store"] = _np(o)
        out["store_state"] = {k: v.clone().cpu().numpy() for k, v in vo.store.sim3_search_state(vo.dev, TOPK).items()}
        out["rc_bad"] = [vo.vo.search_sim3_dev(vo.dev, win, **b)[0] for b in (dict(th=0.0), dict(th_high=257), dict(th_high=-1), dict(use_for_refine=2))]
        out["rc_other_topk"] = [vo.vo.search_sim3_dev(vo.dev, win, topk=k)[0] for k in (2, 1, 0, TOPK + 1)]
        out["used"] = _np(vo.search_sim3(use_for_refine=True))
        out["refined_after"] = _np(vo.refine_sim3(fixed_scale=True, **OPT))
        out["refine_state"] = {k: v.clone().cpu().numpy() for k, v in vo.store.sim3_refine_state(vo.dev, TOPK).items()}
        out["again"] = _np(vo.search_sim3(use_for_refine=True, srt=_dev(out["refined_after"]["cand_srt"])))
        vo.synchronize()
        out.update(before=before, after=after, used_state=_full(vo), win=_np(win))
        # a verification after the Sim(3) query: the query has to be made again
        vo.relocalize(**RELOC)
        out["rc_after_relocalize"] = vo.vo.search_sim3_dev(vo.dev, win)[0]
        with pytest.raises(capi.TBError) as e:
            vo.search_sim3()
        out["rc_after_relocalize_wrapper"] = e.value.code
        win = vo.relocalize_sim3(fixed_scale=True, min_consensus=20, seed=7)
        out["rc_after_relocalize_again"], kept = vo.vo.search_sim3_dev(vo.dev, win)
        vo.synchronize()                    # the outputs live until the query has written them
        _steps(vo, frames, REVISIT + 1, REVISIT + 2)
        out["rc_after_the_next_step"] = vo.vo.search_sim3_dev(vo.dev, win)[0]
        _steps(vo, frames, REVISIT + 2, NF)
        out["end"] = _full(vo)
    finally:
        vo.close()
    return out


def test_the_query_equals_the_store_level_call(asked):
    a, b = asked["plain"], asked["store"]
    for k, v in b.items():
        assert a[k].tobytes() == v.tobytes(), k
    for k, v in asked["store_state"].items():
        assert asked["state"][k].tobytes() == v.tobytes(), k
    for k in ("new", "total", "cand_new", "cand_total", "cand_stats"):
        assert k in a, k
    for k, v in asked["used"].items():          # use_for_refine changes what the refinement reads, not what the search writes
        assert a[k].tobytes() == v.tobytes(), k
    win, st = asked["win"], asked["state"]
    assert a["cand_new"].shape == (S, TOPK) and a["cand_stats"].shape == (S, TOPK, 8)
    skipped = win["cand_consensus"] < 3
    assert (a["cand_stats"][..., 7][skipped] == 2).all() and (a["cand_stats"][..., 7][~skipped] == 0).all()
    assert np.array_equal(a["cand_new"].reshape(-1), st["pair_counts"]) and np.array_equal(a["cand_total"].reshape(-1), st["widened_counts"])
    assert np.array_equal(a["cand_total"][~skipped], (a["cand_new"] + win["cand_consensus"])[~skipped])
    for s in range(S):
        r = int(win["best_rank"][s])
        assert (a["new"][s], a["total"][s]) == ((a["cand_new"][s, r], a["cand_total"][s, r]) if r >= 0 else (0, 0))
    # the lists: mutual, and ascending in the query key
    for p, n in enumerate(st["widened_counts"]):
        w = st["widened"][p, :n]
        assert (np.diff(w[:, 0]) > 0).all()
        m = st["pairs"][p, :st["pair_counts"][p]]
        assert all(st["match1"][p, i] == j and st["match2"][p, j] == i for i, j in m[:, :2])
    # the refinement that followed ran on the widened rows, all of them active
    rs_ = asked["refine_state"]
    assert np.array_equal(rs_["row_counts"], st["widened_counts"]) and (rs_["active"] == 1).all()
    rb, ra = asked["refined_before"], asked["refined_after"]
    for s in range(S):
        print("sequence %d at the revisit: consensus %d, new pairs %d, widened rows %d, refined inliers %d before and %d after the search; "
              "again under the refined transform: %d new pairs" %
              (s, win["consensus"][s], a["new"][s], a["total"][s], rb["inliers"][s], ra["inliers"][s], asked["again"]["new"][s]))


def test_no_state_tensor_changes(asked):
    _same(asked["before"], asked["after"], "search_sim3 is a query")
    _same(asked["before"], asked["used_state"], "use_for_refine changes no state tensor either")


def test_a_loop_that_never_asked_ends_in_the_same_bytes(asked, frames, voc):
    vo = _vo(voc, CAP, None)
    try:
        vo.reset(frames["G0"])
        _steps(vo, frames, 0, NF)
        end = _full(vo)
        for s in range(S):
            _same_seq(end, asked["end"], s, "stepped on without the query")
    finally:
        vo.close()


def test_state_and_argument_errors(asked):
    for k in ("rc_before_a_step", "rc_without_sim3", "rc_wrapper_without_sim3", "rc_after_the_next_step", "rc_after_relocalize",
              "rc_after_relocalize_wrapper"):
        assert asked[k] == capi.TB_ESTATE, k
    assert asked["rc_after_relocalize_again"] == capi.TB_OK
    assert asked["rc_other_topk"] == [capi.TB_EINVAL] * 4
    assert asked["rc_bad"] == [capi.TB_EINVAL] * len(asked["rc_bad"])
    from trackingbench_slam_amd.vo import StereoVO
    vo = StereoVO(1, width=320, height=240, target=300)                     # optical flow: no store
    try:
        assert vo.vo.search_sim3_dev(vo.dev, None)[0] == capi.TB_ESTATE
        with pytest.raises(capi.TBError) as e:
            vo.search_sim3()
        assert e.value.code == capi.TB_ESTATE
    finally:
        vo.close()
