"""GPU tests (pytest -m gpu) of loop correction in the VO loop: StereoVO(tracker="bow", keyframe_db=N, relocalize=M, loop_close=...),
tb_vo_loop_enable / tb_vo_loop_state_dev. tests/test_vo_loop_reference.py's fixture at S = 2, keyframes every 2, capacity 4 and 8:
sequence 0 is shown out and back as images [0, 1, 2, 3, 4, 3, 2, 1, 0] and closes loops at frames 6 and 8; sequence 1 drives
straight on with its own nine frames and must never close.

After every step the CPU composition (tests/vo_loop_reference.py) is run from the GPU's previous state and its own ring, and every
tensor is compared: the loop's (tb_vo_state_dev, tb_vo_tracker_state_dev, tb_vo_bow_state_dev), the store, the database and
tb_vo_loop_state_dev -- integers and bytes exact, floats as bit patterns, poses by the rule of the VO tests. What
comes out of the optimiser -- the node poses after, chi2 -- is held to the solver's 1e-6 against tests/pose_graph_reference.py;
the composition then adopts the GPU's node poses, so the moved map points, the spawned points and the stored poses are compared
bit for bit. The solver's iteration and trial counts are not compared: these graphs converge inside their 10 iterations, and at
chi2's rounding floor the sign of rho is noise (tests/test_gpu_pose_graph.py compares counts, on cases that stop before it).
Sequence 1, and sequence 0 up to its first loop, equal a loop with correction off bit for bit; a loop with correction on and
min_inliers 1000 equals that loop in every tensor."""
import copy

import numpy as np
import pytest

import pose_graph_reference as pg
import reloc_reference as rr
import vo_bow_reference as vb
import vo_desc_reference as vd
import vo_loop_reference as vl
from test_gpu_vo_bow import _check_bow, _snap
from test_gpu_vo_desc import _check_step, _dev, _pose_close
from test_gpu_vo_recover import _kf_of, _np, _same_seq
from test_gpu_vo_reloc import _check_store
from trackingbench_slam_amd import capi, synth, synth_seq
from trackingbench_slam_amd.vo import LOOP_DEFAULTS, StereoVO

pytestmark = pytest.mark.gpu

W, H, K, TARGET, EVERY = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 2
S, NF = 2, 9
IX = [0, 1, 2, 3, 4, 3, 2, 1, 0]
LOOP = dict(topk=4, exclude_newest=1, min_inliers=42, iters=10, w_rot=1.0, w_trans=1.0)
TR = vb.Tracker()
P = vd.Params(width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY)
CLOSES = {6: 2, 8: 0}      # frame -> the keyframe sequence 0 closes with (tests/test_vo_loop_reference.py)


@pytest.fixture(scope="module")
def voc():
    return synth.vocabulary(1, 10, 5)


@pytest.fixture(scope="module")
def frames():
    """L, R [NF, S, H, W], G [., S, 4, 4] and the CPU extraction per (frame, sequence), each image extracted once"""
    a = synth_seq.sequence(0, 5, width=W, height=H, K=K, speed=0.1)
    b = synth_seq.sequence(1, NF, width=W, height=H, K=K, speed=0.1)
    L = np.stack([np.stack([a[0][IX[t]], b[0][t]]) for t in range(NF)])
    R = np.stack([np.stack([a[1][IX[t]], b[1][t]]) for t in range(NF)])
    G0 = np.stack([a[2][0], b[2][0]])
    oa, ob = [vd.extract(a[0][i], P) for i in range(5)], [vd.extract(b[0][t], P) for t in range(NF)]
    return dict(L=L, R=R, G0=G0, orb=lambda t, s: oa[IX[t]] if s == 0 else ob[t])


def _vo(voc, cap, loop):
    return StereoVO(S, width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY, tracker="bow", vocab=voc, keyframe_db=cap,
                    relocalize=cap, loop_close=loop)


def _full(vo):
    out = dict(snap=_snap(vo), store=_np(vo.keyframe_store()), db=_np(vo.keyframe_database()))
    if vo.loop_close is not None:
        out["loop"] = _np(vo.loop())
    return out


@pytest.fixture(scope="module")
def plain(frames, voc):
    """per capacity: the state after every step of a loop with correction off"""
    cache = {}

    def get(cap):
        if cap not in cache:
            vo = _vo(voc, cap, None)
            try:
                with pytest.raises(capi.TBError) as e:
                    vo.loop()
                assert e.value.code == capi.TB_ESTATE and vo.loop_close is None
                vo.reset(frames["G0"])
                out = []
                for t in range(NF):
                    vo.step(_dev(frames["L"][t]), _dev(frames["R"][t]) if t % EVERY == 0 else None)
                    out.append(_full(vo))
                assert vo.vo.loop_enable(capi.VOLoop(4, 1, 42, 10, 1.0, 1.0)) == capi.TB_ESTATE      # after a step
            finally:
                vo.close()
            cache[cap] = out
        return cache[cap]
    return get


def _check_loop_state(lp, s, res, t, cap, ring, where):
    """tb_vo_loop_state_dev of sequence s against the composition's stage"""
    n, ne = len(res["before"]), len(res["edges"])
    ids = [ring.kfs[slot]["kf_id"] for slot in res["slots"]]
    assert lp["closed"][s] == res["closed"] and lp["loop_kf"][s] == res["loop_kf"] and lp["loop_inliers"][s] == res["loop_inliers"], where
    assert lp["nnodes"][s] == n and lp["edge_counts"][s] == ne, where
    assert lp["node_kf"][s].tolist() == ids + [t] + [-1] * (cap - len(ids)), where
    assert lp["before"][s, :n - 1].tobytes() == res["before"][:n - 1].tobytes(), where           # the stored poses
    assert _pose_close(lp["before"][s, n - 1], res["before"][n - 1], 1e-6), where                 # the tracking step's pose
    assert np.array_equal(lp["before"][s, n:], np.broadcast_to(np.eye(4, dtype=np.float32), (cap + 1 - n, 4, 4))), where
    assert lp["after"][s, n:].tobytes() == lp["before"][s, n:].tobytes() and lp["after"][s, 0].tobytes() == lp["before"][s, 0].tobytes(), where
    st = lp["stats"][s]
    if ne == 0:
        assert not st.any() and lp["after"][s].tobytes() == lp["before"][s].tobytes(), where
        return
    e = np.frombuffer(lp["edges"][s].tobytes(), pg.EDGE)[:ne]
    assert np.array_equal(e["a"], res["edges"]["a"]) and np.array_equal(e["b"], res["edges"]["b"]), where
    assert np.all(e["w_rot"] == LOOP["w_rot"]) and np.all(e["w_trans"] == LOOP["w_trans"]), where
    # an edge of the stored float32 poses is the same arithmetic to rounding; the ones that touch the current pose inherit its 1e-6
    assert np.allclose(e["q"], res["edges"]["q"], rtol=0, atol=1e-6) and np.allclose(e["t"], res["edges"]["t"], rtol=1e-6, atol=1e-6), where
    assert np.allclose(e["q"][:ne - 2], res["edges"]["q"][:ne - 2], rtol=0, atol=1e-14), where
    # the initial chi2 is the loop edge's residual squared, a difference of two poses that each carry the tracking step's 1e-6
    assert st[7] == res["stats"][7] == 0 and np.isclose(st[1], res["stats"][1], rtol=1e-3) and st[2] < st[1], where
    for i in range(n):
        assert _pose_close(lp["after"][s, i], res["solved"][i], 1e-6), (where, i)


@pytest.mark.parametrize("cap", [4, 8])
def test_loops_close_and_correct_the_keyframes_and_the_other_sequence_is_untouched(frames, voc, plain, cap):
    L, R, G0, orb = frames["L"], frames["R"], frames["G0"], frames["orb"]
    off = plain(cap)
    rings = [rr.Keyframes(cap) for _ in range(S)]
    vo = _vo(voc, cap, LOOP)
    closed_at = {}
    try:
        assert vo.loop_close == dict(LOOP_DEFAULTS, **LOOP)
        vo.reset(G0)
        prev = None
        for t in range(NF):
            keyframe = t % EVERY == 0
            vo.step(_dev(L[t]), _dev(R[t]) if keyframe else None)
            full = _full(vo)
            g, lp = full["snap"], full["loop"]
            for s in range(S):
                where = "capacity %d frame %d seq %d" % (cap, t, s)
                cpu_in = vd.initial_state(G0[s]) if t == 0 else dict(t=t, Tcw=prev["snap"]["Tcw"][s], kf=_kf_of(prev["snap"], s, prev["snap"]["kf_frame"]))
                exp, info = vl.step(cpu_in, copy.deepcopy(rings[s]), L[t, s], R[t, s], P, TR, voc, LOOP, orb=orb(t, s), after=lp["after"][s],
                                    spawn_Tcw=g["Tcw"][s])
                res = info["loop"]
                assert g["kf_frame"] == t - t % EVERY, where
                _check_step(g, s, exp, info, where, P.K, cpu_in["Tcw"])
                _check_bow(g, s, exp, where)
                if res is not None:
                    print("%s: candidates %s, closed %d with kf %d (%d inliers), chi2 %.3g -> %.3g" % (
                        where, [(c["kf"], c["n_inliers"]) for c in res["reloc"]["cands"]], res["closed"], res["loop_kf"], res["loop_inliers"],
                        lp["stats"][s, 1], lp["stats"][s, 2]))
                    _check_loop_state(lp, s, res, t, cap, rings[s], where)
                    if res["closed"]:
                        closed_at[t, s] = res["loop_kf"]
                        assert g["Tcw"][s].tobytes() == lp["after"][s, len(res["before"]) - 1].tobytes(), where
                        vl.adopt_store(rings[s], res)
                if keyframe:
                    rings[s].add(_kf_of(g, s, t), g["Tcw"][s], t)
            _check_store(vo, rings, "capacity %d frame %d" % (cap, t))
            db, dbo = full["db"], off[t]["db"]                       # BowVectors do not read poses: the database is the plain loop's
            assert db["nadded"] == dbo["nadded"] and db["kf_ids"].tobytes() == dbo["kf_ids"].tobytes() and db["counts"].tobytes() == dbo["counts"].tobytes(), t
            for s in range(S):
                for slot, n in enumerate(db["counts"][s]):
                    assert db["words"][s, slot, :n].tobytes() == dbo["words"][s, slot, :n].tobytes(), (t, s, slot)
                    assert db["values"][s, slot, :n].tobytes() == dbo["values"][s, slot, :n].tobytes(), (t, s, slot)
            _same_seq(full, off[t], 1, "frame %d against the loop without correction" % t)
            if t < 6:
                _same_seq(full, off[t], 0, "frame %d against the loop without correction" % t)
                assert not lp["closed"].any() and (lp["loop_kf"] == -1).all()
            assert not lp["closed"][1] and lp["loop_kf"][1] == -1 and lp["edge_counts"][1] == 0
            prev = full
        assert closed_at == {(t, 0): kf for t, kf in CLOSES.items()}, closed_at
        # a reset clears the state
        vo.reset(G0)
        lp = _np(vo.loop())
        assert not lp["closed"].any() and (lp["loop_kf"] == -1).all() and not lp["loop_inliers"].any() and not lp["nnodes"].any()
        assert not lp["edge_counts"].any() and (lp["node_kf"] == -1).all() and not lp["stats"].any() and not lp["after"].any()
        vo.step(_dev(L[0]), _dev(R[0]))
        assert vo.vo.loop_enable(capi.VOLoop(4, 1, 42, 10, 1.0, 1.0)) == capi.TB_ESTATE          # after a step, and enabled already
    finally:
        vo.close()


def test_min_inliers_1000_is_the_loop_without_correction(frames, voc, plain):
    cap = 4
    off = plain(cap)
    vo = _vo(voc, cap, dict(LOOP, min_inliers=1000))
    try:
        vo.reset(frames["G0"])
        for t in range(NF):
            vo.step(_dev(frames["L"][t]), _dev(frames["R"][t]) if t % EVERY == 0 else None)
            full = _full(vo)
            for s in range(S):
                _same_seq(full, off[t], s, "frame %d" % t)
            lp = full["loop"]
            assert not lp["closed"].any() and (lp["loop_kf"] == -1).all() and not lp["edge_counts"].any() and not lp["stats"].any()
            if t >= 2:
                assert (lp["nnodes"] == min(t // 2, cap) + 1).all()
    finally:
        vo.close()


def test_enable_checks():
    kw = dict(width=320, height=240, target=300, tracker="bow")
    small = synth.vocabulary(1, 4, 3)
    ok = capi.VOLoop(2, 1, 50, 10, 1.0, 1.0)
    with pytest.raises(TypeError):
        StereoVO(1, vocab=small, keyframe_db=3, loop_close=True, **kw)                         # no relocalize
    with pytest.raises(TypeError):
        StereoVO(1, vocab=small, keyframe_db=3, relocalize=2, loop_close=dict(inliers=3), **kw)
    with pytest.raises(TypeError):
        StereoVO(1, vocab=small, keyframe_db=4, relocalize=4, recover=True, loop_close=True, **kw)
    vo = StereoVO(1, vocab=small, keyframe_db=3, **kw)
    try:
        assert vo.vo.loop_enable(ok) == capi.TB_ESTATE                                       # relocalisation is not enabled
        with pytest.raises(capi.TBError) as e:
            vo.vo.loop_state_dev()
        assert e.value.code == capi.TB_ESTATE
        assert vo.vo.reloc_enable(2) == 0
        assert vo.vo.loop_enable(None) == capi.TB_EINVAL
        for bad in ((0, 1, 50, 10, 1.0, 1.0), (3, 1, 50, 10, 1.0, 1.0), (2, -1, 50, 10, 1.0, 1.0), (2, 1, -1, 10, 1.0, 1.0), (2, 1, 50, -1, 1.0, 1.0),
                    (2, 1, 50, 100, 1.0, 1.0), (2, 1, 50, 10, -1.0, 1.0), (2, 1, 50, 10, 1.0, float("nan")), (2, 1, 50, 10, float("inf"), 1.0)):
            assert vo.vo.loop_enable(capi.VOLoop(*bad)) == capi.TB_EINVAL, bad
        assert vo.vo.loop_enable(ok) == 0
        assert vo.vo.loop_enable(ok) == capi.TB_ESTATE                                       # enabled already
        assert vo.vo.recover_enable(capi.VORecover(30, 2, 1, 50)) == capi.TB_ESTATE          # not combined with recovery
        assert all(vo.vo.loop_state_dev().values())
    finally:
        vo.close()
    vo = StereoVO(1, vocab=small, keyframe_db=3, relocalize=2, recover=dict(topk=2), **kw)
    try:
        assert vo.vo.loop_enable(ok) == capi.TB_ESTATE                                       # recovery is enabled
    finally:
        vo.close()
    vo = StereoVO(1, vocab=small, keyframe_db=64, relocalize=4, **kw)
    try:
        assert vo.vo.loop_enable(ok) == capi.TB_EINVAL                                       # 64 keyframes + the frame: 65 nodes
    finally:
        vo.close()
    with pytest.raises(capi.TBError) as e:
        StereoVO(1, vocab=small, keyframe_db=3, relocalize=3, loop_close=True, **kw)          # the default topk 4 > max_candidates 3
    assert e.value.code == capi.TB_EINVAL
    vo = StereoVO(1, vocab=small, keyframe_db=63, relocalize=4, loop_close=True, **kw)
    try:
        assert vo.loop_close == LOOP_DEFAULTS == dict(topk=4, exclude_newest=1, min_inliers=50, iters=10, w_rot=1.0, w_trans=1.0)
        lp = _np(vo.loop())
        assert not lp["closed"].any() and (lp["loop_kf"] == -1).all() and lp["before"].shape == (1, 64, 4, 4)
    finally:
        vo.close()
