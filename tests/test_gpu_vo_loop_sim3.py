"""GPU tests (pytest -m gpu) of the Sim(3) graph query in the VO loop: StereoVO.loop_sim3, tb_vo_loop_sim3_dev, on the fixture of
tests/test_gpu_vo_reloc_sim3.py (the out-and-back run at 640 x 240, S = 2, keyframes every 2, capacity 4, at the revisit, frame 6).

vo.relocalize(), vo.relocalize_sim3(), then vo.loop_sim3() equals, bit for bit, the store-level call (KeyframeStore.sim3_graph) fed
with the loop's pose -- but for the frame node's id, the frame index here and -2 there -- and equals
tests/sim3_graph_reference.py on the store's rings to the bounds of tests/test_gpu_kf_store_sim3_graph.py: ids, counts and the loop
edge exact, nodes before and odometry edges within 1e-14, nodes after and stats to the solver's 1e-6 with exact counts. No state
tensor of the loop, the store or the database changes, and a loop stepped on after the query ends in the same bytes as one that
never asked."""
import numpy as np
import pytest

import pose_graph_sim3_reference as s3
import sim3_graph_reference as gr
from test_gpu_pose_graph_sim3 import _close
from test_gpu_vo_loop import NF, S, _full, _vo, frames, voc  # noqa: F401 (fixtures)
from test_gpu_vo_recover import _same_seq
from test_gpu_vo_reloc_sim3 import CAP, RELOC, REVISIT, _np, _same, _steps
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu

ITERS, W = 3, (1.0, 2.0, 0.5)


@pytest.fixture(scope="module")
def asked(frames, voc):
    """the loop run to the revisit, queried, and stepped on to the end"""
    vo = _vo(voc, CAP, None)
    out = {}
    try:
        vo.reset(frames["G0"])
        out["rc_before_a_step"] = vo.vo.loop_sim3_dev(vo.dev)[0]
        _steps(vo, frames, 0, REVISIT + 1)
        out["rc_without_relocalize"] = vo.vo.loop_sim3_dev(vo.dev)[0]
        vo.relocalize(**RELOC)
        out["rc_without_sim3"] = vo.vo.loop_sim3_dev(vo.dev)[0]
        out["win"] = _np(vo.relocalize_sim3(fixed_scale=True, min_consensus=20, seed=7))
        vo.synchronize()
        before = _full(vo)
        out["held"] = _np(vo.loop_sim3(ITERS, True, *W))
        out["free"] = _np(vo.loop_sim3(ITERS, False, *W))
        out["default"] = _np(vo.loop_sim3())
        vo.synchronize()
        out.update(before=before, after=_full(vo))
        out["store"] = _np(vo.keyframe_store())
        Tcw = vo.Tcw().contiguous()
        vo.synchronize()
        out["Tcw"] = Tcw.cpu().numpy()
        views = vo.store.sim3_graph(Tcw, ITERS, True, *W)
        vo.synchronize()                # the store's call runs on the loop's stream and returns views of the store's buffers
        out["store_held"] = _np(views)
        out["rc_bad"] = [vo.vo.loop_sim3_dev(vo.dev, **b)[0] for b in (dict(iters=-1), dict(iters=100), dict(fixed_scale=2), dict(w_rot=-1.0),
                                                                        dict(w_scale=float("nan")))]
        # no winner: an empty graph, nothing moved
        out["none_win"] = _np(vo.relocalize_sim3(fixed_scale=True, min_consensus=100000, seed=7))
        out["none"] = _np(vo.loop_sim3(ITERS, True, *W))
        vo.synchronize()
        _steps(vo, frames, REVISIT + 1, REVISIT + 2)
        out["rc_after_the_next_step"] = vo.vo.loop_sim3_dev(vo.dev)[0]
        _steps(vo, frames, REVISIT + 2, NF)
        out["end"] = _full(vo)
    finally:
        vo.close()
    return out


def test_the_query_equals_the_store_level_call(asked):
    a, b = asked["held"], asked["store_held"]
    for k, v in b.items():
        if k != "node_kf":
            assert a[k].tobytes() == v.tobytes(), k
    n = a["nnodes"]
    for s in range(S):
        assert a["node_kf"][s, n[s] - 1] == REVISIT and b["node_kf"][s, n[s] - 1] == -2
        assert np.array_equal(np.delete(a["node_kf"][s], n[s] - 1), np.delete(b["node_kf"][s], n[s] - 1))


@pytest.mark.parametrize("name", ["held", "free"])
def test_graph_and_solution_equal_the_reference(asked, name):
    g, st, win = asked[name], asked["store"], asked["win"]
    assert win["best_kf"][0] == 2
    for s in range(S):
        e = gr.query(st["Tcw"][s], st["kf_ids"][s], st["nadded"], asked["Tcw"][s], int(win["best_kf"][s]), win["best_srt"][s], ITERS,
                     name == "held", W, frame_id=REVISIT)
        nn, cnt = CAP + 1, e["count"]
        assert g["nnodes"][s] == e["nnodes"] and g["edge_counts"][s] == cnt and g["node_kf"][s].tolist() == e["node_kf"].tolist()
        assert g["before"].shape == (S, nn, 8) and np.abs(g["before"][s] - e["nodes"]).max() < 1e-14
        ge = g["edges"][s].view(s3.EDGE).reshape(-1)
        for f in ("a", "b", "w_rot", "w_trans", "w_scale"):
            assert np.array_equal(ge[f], e["edges"][f]), f
        assert np.abs(ge["srt"] - e["edges"]["srt"]).max() < 1e-14
        if cnt:
            assert ge["srt"][cnt - 1].tobytes() == win["best_srt"][s].tobytes() and ge["b"][cnt - 1] == cnt - 1
            _close(g["after"][s], e["after"], g["stats"][s], e["stats"])
            assert g["stats"][s, 2] < g["stats"][s, 1]
            k = int(ge["a"][cnt - 1])
            assert g["node_kf"][s, k] == win["best_kf"][s]
            target = s3.srt_to_matrix(win["best_srt"][s]) @ s3.srt_to_matrix(g["before"][s, k])
            d0 = np.linalg.norm(s3.log(s3.srt_to_matrix(g["before"][s, cnt - 1]) @ s3.inv(target)))
            d1 = np.linalg.norm(s3.log(s3.srt_to_matrix(g["after"][s, cnt - 1]) @ s3.inv(target)))
            print("sequence %d %s: chi2 %.4g -> %.4g, |Log(S_frame target^-1)| %.4g -> %.4g" % (s, name, g["stats"][s, 1], g["stats"][s, 2], d0, d1))
            assert d1 < d0
        else:
            assert g["after"][s].tobytes() == g["before"][s].tobytes() and not g["stats"][s].any()
        assert g["after"][s, 0].tobytes() == g["before"][s, 0].tobytes()
        if name == "held":
            assert np.all(g["after"][s, :, 7] == 1.0)
    assert g["edge_counts"][0] == g["nnodes"][0] >= 3       # sequence 0 is back at image 2: its loop is built


def test_no_winner_gives_an_empty_graph(asked):
    g = asked["none"]
    assert asked["none_win"]["best_kf"].tolist() == [-1] * S
    assert g["edge_counts"].tolist() == [0] * S and not g["stats"].any() and not g["edges"].any()
    assert g["after"].tobytes() == g["before"].tobytes() == asked["held"]["before"].tobytes()


def test_no_state_tensor_changes(asked):
    _same(asked["before"], asked["after"], "loop_sim3 is a query")


def test_a_loop_that_never_asked_ends_in_the_same_bytes(asked, frames, voc):
    vo = _vo(voc, CAP, None)
    try:
        vo.reset(frames["G0"])
        _steps(vo, frames, 0, NF)
        end = _full(vo)
        for s in range(S):      # another loop's buffers: every live entry (what lies beyond a count was never written)
            _same_seq(end, asked["end"], s, "stepped on without the query")
    finally:
        vo.close()


def test_state_and_argument_errors(asked):
    for k in ("rc_before_a_step", "rc_without_relocalize", "rc_without_sim3", "rc_after_the_next_step"):
        assert asked[k] == capi.TB_ESTATE, k
    assert asked["rc_bad"] == [capi.TB_EINVAL] * len(asked["rc_bad"])
    from trackingbench_slam_amd.vo import StereoVO
    vo = StereoVO(1, width=320, height=240, target=300)                     # optical flow: no store
    try:
        assert vo.vo.loop_sim3_dev(vo.dev)[0] == capi.TB_ESTATE
        with pytest.raises(capi.TBError) as e:
            vo.loop_sim3()
        assert e.value.code == capi.TB_ESTATE
    finally:
        vo.close()
