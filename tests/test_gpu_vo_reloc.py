"""GPU tests (pytest -m gpu) of relocalisation in the VO loop: StereoVO(tracker="bow", keyframe_db=N, relocalize=M),
tb_vo_reloc_enable / tb_vo_relocalize_dev / tb_vo_kf_store_get. Two sequences (seeds 0 and 1) at 640 x 240 with 600 keys, 7 frames
of a slow drive with keyframes every 2 frames (0, 2, 4, 6), then frame 1's image again as frame 7 -- a jump back. Capacity 2 (the
ring wraps) and 4.

After every step the store is the ring of the snapshots taken at the keyframe steps; relocalize() equals tests/reloc_reference.py
run from the GPU's own state (match lists, rows, counts, flags, inliers, outlier flags, cand_kf, best_rank, best_kf exact; poses by
the rule of the VO tests); it changes no state tensor, and a loop with relocalisation enabled steps exactly as one
without. With capacity 4 the jump back is recovered: the winner is keyframe 0 or 2 with at least 40 inliers and at least twice the
tracking step's (tests/test_reloc_reference.py has the CPU figures)."""
import numpy as np
import pytest

import oracle
import reloc_reference as rr
import vo_bow_reference as vb
from test_gpu_kf_store import _rows
from test_gpu_vo_bow import _snap
from test_gpu_vo_bow_db import _live
from test_gpu_vo_desc import _dev, _i32, _pose_parity, _same_bits
from trackingbench_slam_amd import capi, synth, synth_seq
from trackingbench_slam_amd.vo import StereoVO

pytestmark = pytest.mark.gpu

W, H, K, TARGET, EVERY, T = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 2, 7
SEEDS = (0, 1)
S = len(SEEDS)
NLEVELS, SCALE = 5, 0.8
TR = vb.Tracker()
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def seqs():
    """[T + 1, S, ...]: frames 0..6, then frame 1 again (its right image is not needed: frame 7 is no keyframe)"""
    out = [synth_seq.sequence(s, T, width=W, height=H, K=K, speed=0.1) for s in SEEDS]
    L, R, G = (np.stack([o[i] for o in out], 1) for i in range(3))
    return np.concatenate([L, L[1:2]]), np.concatenate([R, R[1:2]]), G


@pytest.fixture(scope="module")
def voc():
    return synth.vocabulary(1, 10, 5)


def _vo(voc, cap, reloc):
    return StereoVO(S, width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY, tracker="bow", vocab=voc, keyframe_db=cap,
                    relocalize=reloc)


def _kf_of(g, s, Tcw, frame):
    """the keyframe snapshot of sequence s in a _snap as reloc_reference keeps a keyframe"""
    k, nf, nb = g["kf_cnt"][s], g["kf_fv_counts"][s], g["kf_bv_counts"][s]
    return dict(orb=g["kf_orb"][s, :k].copy().view(oracle.KEYPOINT).reshape(k), desc=g["kf_desc"][s, :k].copy(), mp=g["kf_mp"][s, :k].copy(),
                valid=g["kf_mv"][s, :k].astype(bool), frame=frame, fv_keys=g["kf_fv_keys"][s, :nf].copy(),
                bow=dict(fv=vb.fv_from_keys(g["kf_fv_keys"][s, :nf].view(np.uint64)),
                         bv=dict(zip(g["kf_bv_words"][s, :nb].tolist(), g["kf_bv_values"][s, :nb].tolist()))), Tcw=Tcw.copy())


def _check_store(vo, rings, what):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in vo.keyframe_store().items()}
    assert g["nadded"] == rings[0].ring.nadded, what
    for s, ring in enumerate(rings):
        assert g["kf_ids"][s].tolist() == ring.ring.kf_ids, (what, s)
        for slot, kf in enumerate(ring.kfs):
            w = (what, s, slot)
            if kf is None:
                assert g["counts"][s, slot] == 0 and g["fv_counts"][s, slot] == 0, w
                continue
            n, nf = len(kf["orb"]), len(kf["fv_keys"])
            assert g["counts"][s, slot] == n > 100 and g["fv_counts"][s, slot] == nf > 100, w
            assert g["keys"][s, slot, :n].tobytes() == _i32(kf["orb"]).tobytes(), w
            assert g["desc"][s, slot, :n].tobytes() == kf["desc"].tobytes(), w
            assert g["fv_keys"][s, slot, :nf].tobytes() == kf["fv_keys"].tobytes(), w
            assert g["map_points"][s, slot, :n].tobytes() == kf["mp"].tobytes(), w
            assert g["mp_valid"][s, slot, :n].tobytes() == kf["valid"].astype(np.uint8).tobytes(), w
            assert g["Tcw"][s, slot].tobytes() == kf["Tcw"].tobytes(), w


def _check_reloc(vo, g, rings, topk, excl, min_inliers, what):
    """relocalize() against the composition on the GPU's current frame and the ring; returns the output as numpy arrays"""
    out = vo.relocalize(topk, excl, min_inliers)
    vo.synchronize()
    work = vo.store.work(vo.dev, topk)
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o.update({k: v.cpu().numpy() for k, v in work.items()})
    for s, ring in enumerate(rings):
        n, nf = g["ocnt"][s], g["fv_counts"][s]
        kps = g["orb"][s, :n].copy().view(oracle.KEYPOINT).reshape(n)
        bow = dict(fv=vb.fv_from_keys(g["fv_keys"][s, :nf].view(np.uint64)))
        slots = o["top_slot"][s]
        ranked = ring.ring.ranked_slots(excl)
        cnt = min(topk, len(ranked))
        assert o["top_count"][s] == cnt and set(slots[:cnt]) <= set(ranked) and (slots[cnt:] == -1).all(), (what, s)
        e = rr.relocalize(kps, g["desc"][s, :n], bow, ring, slots, TR, K, NLEVELS, SCALE, min_inliers)
        for r, c in enumerate(e["cands"]):
            p, w = s * topk + r, (what, s, r)
            nm, no = len(c["matches"]), len(c["obs"])
            assert o["cand_kf"][s, r] == c["kf"] == o["top_kf"][s, r] and o["cand_flags"][s, r] == 0, w
            assert o["cand_matches"][s, r] == nm == o["match_counts"][p], w
            assert np.array_equal(o["matches"][p, :nm], _i32(c["matches"]).reshape(nm, 4)), w
            assert o["cand_rows"][s, r] == no == o["row_counts"][p], w
            assert _same_bits(o["rows"][p, :no], _rows(c["obs"])), w
            assert o["cand_inliers"][s, r] == c["n_inliers"], w
            assert np.array_equal(o["outlier"][p, :no], c["outlier"][:no]), w
            if c["kf"] < 0 or no < 3:
                assert o["cand_Tcw"][s, r].tobytes() == c["Tcw"].tobytes(), w
            else:
                assert _pose_parity(o["cand_Tcw"][s, r], c["Tcw"], K, ring.kfs[slots[r]]["Tcw"], c["obs"]), w
        assert o["best_rank"][s] == e["best_rank"] and o["best_kf"][s] == e["best_kf"], (what, s)
        want = o["cand_Tcw"][s, e["best_rank"]] if e["best_rank"] >= 0 else EYE
        assert o["best_Tcw"][s].tobytes() == want.tobytes(), (what, s)
    return o


def _same_snap(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        for s in range(S):
            x, y = _live(a, k, s), _live(b, k, s)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, s)


@pytest.fixture(scope="module")
def plain(seqs, voc):
    """the _snap of every step of a loop with the database but without relocalisation"""
    L, R, G = seqs
    vo = _vo(voc, 4, 0)
    snaps = []
    try:
        assert vo.store is None
        with pytest.raises(capi.TBError) as e:
            vo.relocalize()
        assert e.value.code == capi.TB_ESTATE
        with pytest.raises(capi.TBError) as e:
            vo.vo.kf_store()
        assert e.value.code == capi.TB_ESTATE
        vo.reset(G[0])
        for t in range(T + 1):
            vo.step(_dev(L[t]), _dev(R[t]) if t % EVERY == 0 else None)
            snaps.append(_snap(vo))
        assert vo.vo.reloc_enable(2) == capi.TB_ESTATE                     # after a step
    finally:
        vo.close()
    return snaps


@pytest.mark.parametrize("cap", [2, 4])
def test_store_follows_the_keyframes_and_relocalize_matches_the_composition(seqs, voc, plain, cap):
    L, R, G = seqs
    rings = [rr.Keyframes(cap) for _ in range(S)]
    vo = _vo(voc, cap, cap)
    try:
        assert (vo.store.nseq, vo.store.capacity, vo.store.pitch, vo.store.max_candidates) == (S, cap, vo.key_pitch, cap)
        with pytest.raises(capi.TBError) as e:
            vo.relocalize()                                                # before the first step
        assert e.value.code == capi.TB_ESTATE
        vo.reset(G[0])
        for t in range(T + 1):
            vo.step(_dev(L[t]), _dev(R[t]) if t % EVERY == 0 else None)
            g = _snap(vo)
            _same_snap(g, plain[t], "frame %d: the loop with relocalisation against the loop without" % t)
            if t % EVERY == 0:
                for s in range(S):
                    rings[s].add(_kf_of(g, s, g["Tcw"][s], t), g["Tcw"][s], t)
            _check_store(vo, rings, "frame %d" % t)
            for excl in (0, 1):
                _check_reloc(vo, g, rings, 2, excl, 50, "frame %d exclude_newest %d" % (t, excl))
            _same_snap(_snap(vo), g, "frame %d: relocalize is a query" % t)
            _check_store(vo, rings, "frame %d after relocalize" % t)
        # the jump back (frame 7 shows frame 1 again)
        assert vo.frame == T and g["kf_frame"] == 6
        if cap == 4:
            o = _check_reloc(vo, g, rings, 4, 0, 50, "jump back")
            for s in range(S):
                inl = dict(zip(o["cand_kf"][s].tolist(), o["cand_inliers"][s].tolist()))
                print("seq %d: tracker %d inliers; candidates %s -> kf %d" % (s, g["ninl"][s], inl, o["best_kf"][s]))
                assert sorted(inl) == [0, 2, 4, 6] and inl[6] == g["ninl"][s]
                assert o["best_kf"][s] in (0, 2) and o["cand_kf"][s, o["best_rank"][s]] == o["best_kf"][s]
                best = o["cand_inliers"][s, o["best_rank"][s]]
                assert best == max(inl.values()) >= 40 and best >= 2 * g["ninl"][s]
            o = _check_reloc(vo, g, rings, 4, 0, 1000, "jump back, 1000 inliers asked")
            assert (o["best_rank"] == -1).all() and (o["best_kf"] == -1).all()
            assert all(o["best_Tcw"][s].tobytes() == EYE.tobytes() for s in range(S))
        # on a non-keyframe step with exclude_newest 0, the candidate that is the loop's keyframe is the tracking step itself
        o = _check_reloc(vo, g, rings, cap, 0, 50, "the keyframe as a candidate")
        for s in range(S):
            r = o["cand_kf"][s].tolist().index(6)
            p, nm, no = s * cap + r, g["mc"][s], g["oc"][s]
            assert o["cand_matches"][s, r] == nm > 0 and o["matches"][p, :nm].tobytes() == g["mt"][s, :nm].tobytes()
            assert o["cand_rows"][s, r] == no > 0 and o["rows"][p, :no].tobytes() == g["obs"][s, :no].tobytes()
        # topk beyond max_candidates, and a reset
        with pytest.raises(capi.TBError) as e:
            vo.relocalize(cap + 1)
        assert e.value.code == capi.TB_EINVAL
        vo.reset(G[0])
        st = vo.keyframe_store()
        assert st["nadded"] == 0 and (st["kf_ids"] == -1).all() and (st["counts"] == 0).all() and (st["fv_counts"] == 0).all()
        vo.step(_dev(L[0]), _dev(R[0]))
        st = vo.keyframe_store()
        assert st["nadded"] == 1 and st["kf_ids"].cpu().numpy().tolist() == [[0] + [-1] * (cap - 1)] * S
        assert vo.vo.reloc_enable(cap) == capi.TB_ESTATE                   # after a step, and enabled already
    finally:
        vo.close()


def test_enable_needs_a_bow_loop_with_a_database_before_the_first_step(voc):
    vo = StereoVO(1, width=320, height=240, target=300)                     # optical flow
    try:
        assert vo.vo.reloc_enable(2) == capi.TB_ESTATE
    finally:
        vo.close()
    vo = StereoVO(1, width=320, height=240, target=300, tracker="violence")
    try:
        assert vo.vo.reloc_enable(2) == capi.TB_ESTATE
    finally:
        vo.close()
    with pytest.raises(TypeError):
        StereoVO(1, width=320, height=240, target=300, tracker="bow", vocab=voc, relocalize=2)      # no keyframe_db
    vo = StereoVO(1, width=320, height=240, target=300, tracker="bow", vocab=synth.vocabulary(1, 4, 3))
    try:
        assert vo.vo.reloc_enable(2) == capi.TB_ESTATE                      # no database
        assert vo.vo.bow_db_enable(3) == 0
        for bad in (0, -1, 4):
            assert vo.vo.reloc_enable(bad) == capi.TB_EINVAL                # 1..capacity
        assert vo.vo.reloc_enable(3) == 0
        assert vo.vo.reloc_enable(3) == capi.TB_ESTATE                      # enabled already
        st = vo.vo.kf_store()
        assert (st.nseq, st.capacity, st.pitch, st.max_candidates) == (1, 3, vo.key_pitch, 3)
    finally:
        vo.close()
