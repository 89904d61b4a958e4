"""GPU tests (pytest -m gpu) of the Sim(3) query in the VO loop: StereoVO.relocalize_sim3, tb_vo_relocalize_sim3_dev. The
out-and-back fixture of tests/test_gpu_vo_loop.py at 640 x 240, S = 2, keyframes every 2, capacity 4, run to the revisit: frame 6
shows image 2 again.

vo.relocalize() then vo.relocalize_sim3() equals, bit for bit, the store-level call (KeyframeStore.sim3) fed with the loop's own
current ORB keys, carried map points, pose and the verification's top_slot; with fixed_scale=True the scale is exactly 1; no state
tensor of the loop, the store or the database changes; a loop stepped on after the query produces the same bytes as one that
never asked. The scale the unfixed solver finds on this stereo map is printed, not asserted (DESIGN.md 9n records it)."""
import numpy as np
import pytest

from test_gpu_vo_desc import _dev
from test_gpu_vo_loop import EVERY, K, NF, S, _full, _vo, frames, voc  # noqa: F401 (fixtures)
from test_gpu_vo_recover import _same_seq
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu

CAP, REVISIT, TOPK = 4, 6, 4
RELOC = dict(topk=TOPK, exclude_newest=1, min_inliers=42)


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for part in a:
        assert a[part].keys() == b[part].keys(), (what, part)
        for k in a[part]:
            x, y = a[part][k], b[part][k]
            assert (x.tobytes() == y.tobytes()) if hasattr(x, "tobytes") else (x == y), (what, part, k)


def _steps(vo, frames, t0, t1):
    for t in range(t0, t1):
        vo.step(_dev(frames["L"][t]), _dev(frames["R"][t]) if t % EVERY == 0 else None)


@pytest.fixture(scope="module")
def asked(frames, voc):
    """the loop run to the revisit, queried, and stepped on to the end"""
    vo = _vo(voc, CAP, None)
    out = {}
    try:
        vo.reset(frames["G0"])
        out["rc_before_a_step"] = vo.vo.relocalize_sim3_dev(vo.dev)[0]
        _steps(vo, frames, 0, REVISIT + 1)
        out["rc_without_relocalize"] = vo.vo.relocalize_sim3_dev(vo.dev)[0]
        before = _full(vo)
        reloc = _np(vo.relocalize(**RELOC))
        mid = _full(vo)
        out["fixed"] = _np(vo.relocalize_sim3(fixed_scale=True, min_consensus=20, seed=7))
        out["free"] = _np(vo.relocalize_sim3(fixed_scale=False, min_consensus=20, seed=7))
        vo.synchronize()
        after = _full(vo)
        # the store-level call fed from the loop's state (tb_vo_state_dev / tb_vo_tracker_state_dev, copied out)
        orb, _, ocnt = vo.orb()
        mp, valid = vo.map_points()
        Tcw = vo.Tcw()
        top = _dev(reloc["top_slot"])
        vo.synchronize()
        p = vo.params
        for name, fs in (("store_fixed", True), ("store_free", False)):
            o = vo.store.sim3(K, p.nlevels, p.scale, orb.contiguous(), ocnt.contiguous(), mp.contiguous(), valid.contiguous(),
                              Tcw.contiguous(), top.contiguous(), min_consensus=20, fixed_scale=fs, seed=7)
            vo.synchronize()                # the store's call runs on the loop's stream
            out[name] = _np(o)
        out["rc_bad"] = vo.vo.relocalize_sim3_dev(vo.dev, hypotheses=0)[0]
        out.update(before=before, mid=mid, after=after, reloc=reloc)
        # a verification of fewer candidates than the store holds room for: the query follows it, and refuses any other count
        out["reloc2"] = _np(vo.relocalize(**dict(RELOC, topk=2)))
        out["fixed2"] = _np(vo.relocalize_sim3(fixed_scale=True, min_consensus=20, seed=7))
        out["rc_other_topk"] = [vo.vo.relocalize_sim3_dev(vo.dev, topk=k)[0] for k in (4, 1, 3, 0)]
        out["after2"] = _full(vo)
        _steps(vo, frames, REVISIT + 1, REVISIT + 2)
        out["rc_after_the_next_step"] = vo.vo.relocalize_sim3_dev(vo.dev)[0]
        _steps(vo, frames, REVISIT + 2, NF)
        out["end"] = _full(vo)
    finally:
        vo.close()
    return out


def test_the_query_equals_the_store_level_call(asked):
    for a, b in (("fixed", "store_fixed"), ("free", "store_free")):
        for k, v in asked[b].items():
            assert asked[a][k].tobytes() == v.tobytes(), (a, k)
        for k in ("S12", "srt", "consensus", "best_rank", "best_kf", "cand_rows", "cand_consensus", "cand_flags", "cand_S12", "cand_srt"):
            assert k in asked[a], k
    f, r = asked["fixed"], asked["reloc"]
    assert (f["cand_srt"][..., 7] == 1.0).all() and (f["srt"][:, 7] == 1.0).all()
    # sequence 0 is back at image 2: its map and keyframe 2's agree, the transform is close to the relative pose of the two frames
    kfs = dict(zip(r["top_kf"][0].tolist(), f["cand_consensus"][0].tolist()))
    print("sequence 0 at the revisit: consensus per candidate keyframe %s, rows %s, best kf %d; free scale %s" %
          (kfs, f["cand_rows"][0].tolist(), f["best_kf"][0], asked["free"]["cand_srt"][0, :, 7].tolist()))
    assert f["best_kf"][0] == 2 and f["best_rank"][0] >= 0 and f["consensus"][0] >= 20
    assert f["consensus"][0] == f["cand_consensus"][0, f["best_rank"][0]] == max(kfs.values())
    assert np.array_equal(f["S12"][0], f["cand_S12"][0, f["best_rank"][0]]) and np.array_equal(f["srt"][0], f["cand_srt"][0, f["best_rank"][0]])
    assert np.abs(f["srt"][0, 4:7]).max() < 0.5 and f["srt"][0, 0] > 0.999        # image 2 again: nearly the identity
    for s in range(S):                                                          # no answer: the identity, consensus 0
        if f["best_rank"][s] < 0:
            assert f["consensus"][s] == 0 and np.array_equal(f["S12"][s], np.eye(4, dtype=np.float32))


def test_the_query_follows_the_verifications_topk(asked):
    """relocalize(topk=2) on a store with room for 4: relocalize_sim3() at its defaults returns [S, 2] outputs, the same bits as
    the first two candidates of the topk = 4 query, and the library refuses every other count before it writes"""
    f4, f2, r4, r2 = asked["fixed"], asked["fixed2"], asked["reloc"], asked["reloc2"]
    assert np.array_equal(r2["top_slot"], r4["top_slot"][:, :2])
    assert f2["cand_rows"].shape == (S, 2) and f2["cand_S12"].shape == (S, 2, 4, 4) and f2["cand_srt"].shape == (S, 2, 8)
    for k in ("cand_rows", "cand_consensus", "cand_flags", "cand_S12", "cand_srt"):
        assert f2[k].tobytes() == np.ascontiguousarray(f4[k][:, :2]).tobytes(), k
    assert f2["best_kf"][0] == 2 and f2["consensus"][0] == f4["consensus"][0]
    assert asked["rc_other_topk"] == [capi.TB_EINVAL] * 4
    _same(asked["after"], asked["after2"], "the second pair of queries")


def test_no_state_tensor_changes(asked):
    _same(asked["before"], asked["mid"], "relocalize is a query")
    _same(asked["mid"], asked["after"], "relocalize_sim3 is a query")


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


def test_state_errors(asked, voc):
    assert asked["rc_before_a_step"] == capi.TB_ESTATE
    assert asked["rc_without_relocalize"] == capi.TB_ESTATE
    assert asked["rc_after_the_next_step"] == capi.TB_ESTATE
    assert asked["rc_bad"] == capi.TB_EINVAL
    from trackingbench_slam_amd.vo import StereoVO
    vo = StereoVO(1, width=320, height=240, target=300)                     # optical flow: no store
    try:
        assert vo.vo.relocalize_sim3_dev(vo.dev)[0] == capi.TB_ESTATE
        with pytest.raises(capi.TBError) as e:
            vo.relocalize_sim3()
        assert e.value.code == capi.TB_ESTATE
    finally:
        vo.close()
