"""GPU tests of the VO loop's searchByNN tracker (StereoVO(tracker="lsh"), tb_vo_create_lsh) against the CPU composition in
tests/vo_lsh_reference.py: S = 2 at 640 x 240 with 600 keys (key pitch 715), seeds 0 and 1 of the slow synthetic drive,
keyframe_every = 3, 7 frames -- the fixture of tests/test_vo_lsh_reference.py."""
import numpy as np
import pytest

import vo_lsh_reference as vl
from test_gpu_vo_desc import _check_step, _cpu_state, _dev, _snapshot
from test_gpu_vo_ragged import _full, _same_seq
from trackingbench_slam_amd import capi, synth_seq
from trackingbench_slam_amd import vo as vo_mod
from trackingbench_slam_amd.vo import StereoVO

pytestmark = pytest.mark.gpu

W, H, K, TARGET, EVERY, T = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 3, 7
SEEDS = (0, 1)
S = 2


@pytest.fixture(scope="module")
def seqs():
    out = [synth_seq.sequence(s, T, width=W, height=H, K=K, speed=0.1) for s in SEEDS]
    return tuple(np.stack([o[i] for o in out], 1) for i in range(3))   # L, R [T, 2, H, W], G [T, 2, 4, 4]


def _vo(nseq=S, **kw):
    return StereoVO(nseq, width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY, tracker="lsh", **kw)


def _run(vo, L, R, G, n=T):
    vo.reset(G[0])
    out = []
    for t in range(n):
        vo.step(_dev(L[t]), _dev(R[t]) if t % EVERY == 0 else None)
        out.append(_full(vo))
    return out


@pytest.fixture(scope="module")
def batch(seqs):
    """the batch's snapshots after every frame (with kf_frame, as _check_step reads them)"""
    L, R, G = seqs
    vo = _vo()
    try:
        assert vo.key_pitch == 715
        vo.reset(G[0])
        out = []
        for t in range(T):
            vo.step(_dev(L[t]), _dev(R[t]) if t % EVERY == 0 else None)
            g = _full(vo)
            g["kf_frame"] = vo.keyframe()["frame"]
            out.append(g)
        return out
    finally:
        vo.close()


def test_every_step_equals_the_cpu_step_from_the_gpu_state(seqs, batch):
    """ORB records, matches and counts, keys, map points, rows, outlier flags, n_inliers and the keyframe snapshot exact; Tcw by
    the descriptor frame's rule (tests/test_gpu_vo_desc.py)."""
    L, R, G = seqs
    P, tr = vl.Params(width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY), vl.Tracker()
    tracked = 0
    for t in range(T):
        g = {k: v for k, v in batch[t].items() if k not in ("frames", "kf_frames")}
        for s in range(S):
            cpu_in = vl.initial_state(G[0, s]) if t == 0 else _cpu_state(batch[t - 1], s, t)
            exp, info = vl.step(cpu_in, L[t, s], R[t, s], P, tr, spawn_Tcw=g["Tcw"][s])
            _check_step(g, s, exp, info, "lsh frame %d seq %d" % (t, s), P.K, cpu_in["Tcw"])
            m = info["matches"]
            assert (np.diff(m["queryIdx"]) > 0).all()
            tracked += t > 0 and len(info["obs"]) >= 3
    assert tracked >= 1, "some frame tracks with at least 3 rows"


def test_sequence_1_alone_equals_the_batch(seqs, batch):
    """... by its bits; the lone loop takes the bit table explicitly, the batch drew it from the seed"""
    L, R, G = seqs
    one = _vo(1, bits=capi.lsh_draw_bits(20, 10, 0), seed=77)
    try:
        alone = _run(one, L[:, 1:2], R[:, 1:2], G[:, 1:2])
    finally:
        one.close()
    for t in range(T):
        g = {k: v for k, v in batch[t].items() if k != "kf_frame"}
        _same_seq(g, 1, alone[t], 0, ("alone", t))
    assert alone[-1]["mc"][0] > 0


def test_another_bit_table_is_another_tracker(seqs, batch):
    L, R, G = seqs
    vo = _vo(tables=2, key_size=10, multi_probe_level=0, seed=3)
    try:
        got = _run(vo, L, R, G, 3)
    finally:
        vo.close()
    assert any(got[t]["mc"].tolist() != batch[t]["mc"].tolist() for t in (1, 2))


def test_ragged_schedule_equals_the_lone_runs(seqs):
    """sequence 1 joins at step 1, idles at step 2 and takes a forced keyframe at step 3 (its frame 1, off the cadence), where
    sequence 0 has its cadence keyframe; its own cadence keyframe (frame 3) comes at step 5 all the same. Each sequence equals
    its lone run after every step, bit for bit."""
    L, R, G = seqs
    vo, solo = _vo(), [_vo(1), _vo(1)]
    try:
        vo.reset(G[0, 0][None], which=[0])
        for s in range(S):
            solo[s].reset(G[0, s][None])
        frame = [0, 0]
        want, prev = {}, None
        #            active, forced keyframes
        schedule = [((0,), ()), ((0, 1), ()), ((0,), ()), ((0, 1), (1,)), ((0, 1), ()), ((0, 1), ())]
        for step, (act, forced) in enumerate(schedule):
            if step == 1:
                vo.reset(G[0, 1][None], which=[1])
                g = _full(vo)
                _same_seq(g, 0, prev, 0, ("late join leaves sequence 0", step))
                assert g["frames"][1] == -1 and g["kc"][1] == 0
            l = np.full((S, H, W), 0xFF, np.uint8); r = np.full((S, H, W), 0xFF, np.uint8)
            need_right = False
            for s in act:
                t = frame[s]
                kf = t % EVERY == 0 or s in forced
                need_right |= kf
                l[s], r[s] = L[t, s], R[t, s]
                solo[s].step(_dev(L[t, s][None]), _dev(R[t, s][None]) if kf else None, keyframe=[0] if s in forced else None)
                want[s] = _full(solo[s])
                frame[s] += 1
            vo.step(_dev(l), _dev(r) if need_right else None, active=list(act), keyframe=list(forced) or None)
            g = _full(vo)
            for s in want:
                if s in act:
                    _same_seq(g, s, want[s], 0, ("step", step, "seq", s))
                else:
                    _same_seq(g, s, prev, s, ("idle at step", step, "seq", s))
            prev = g
        assert g["frames"].tolist() == [5, 3] and g["kf_frames"].tolist() == [3, 3]   # sequence 1: frame 0, forced at 1, cadence at 3
        assert g["mc"].max() > 0
    finally:
        vo.close()
        for v in solo:
            v.close()


def test_create_time_status_codes(seqs):
    def code(**kw):
        with pytest.raises(capi.TBError) as e:
            _vo(**kw)
        return e.value.code

    for ml in (dict(max_level=4), dict(max_level=6), dict(min_level=1)):
        assert code(**ml) == capi.TB_EUNSUPPORTED, ml
    for bad in (dict(tables=0), dict(tables=33), dict(key_size=0), dict(key_size=33), dict(multi_probe_level=-1),
                dict(multi_probe_level=11), dict(ratio=float("nan")), dict(ratio=float("inf"))):
        assert code(**bad) == capi.TB_EINVAL, bad
    bits = capi.lsh_draw_bits(20, 10, 0)
    b = bits.copy(); b[0, 0] = 256
    assert code(bits=b) == capi.TB_EINVAL
    b = bits.copy(); b[19, 0] = b[19, 9]
    assert code(bits=b) == capi.TB_EINVAL
    with pytest.raises(TypeError):
        _vo(keyframe_db=4)
    with pytest.raises(TypeError):
        _vo(window_ba=True)
    with pytest.raises(TypeError):
        _vo(vocab=object())
    for ok in (dict(), dict(max_level=5), dict(tables=32, key_size=32, multi_probe_level=32), dict(tables=1, key_size=1, multi_probe_level=0)):
        _vo(**ok).close()
    vo = _vo()
    try:
        # tb_vo_tracker keeps its layout: tb_vo_create_ex answers kind 6 with TB_EINVAL and names the entry
        tr = capi.VOTracker()
        tr.kind = capi.TB_VO_NN
        with pytest.raises(capi.TBError) as e:
            capi.VO(vo.ctx, vo.params, S, tr, use_ex=True)
        assert e.value.code == capi.TB_EINVAL and "tb_vo_create_lsh" in str(e.value)
        # StereoVO's own min_th= is the extractor's (as for "bf"), so searchByNN's minTh is checked at the C entry
        for bad in (float("inf"), float("nan")):
            with pytest.raises(capi.TBError) as e:
                capi.VO(vo.ctx, vo.params, S, lsh=vo_mod._tracker("lsh", 5, dict(min_th=bad)))
            assert e.value.code == capi.TB_EINVAL, bad
        capi.VO(vo.ctx, vo.params, S, lsh=vo_mod._tracker("lsh", 5, dict(min_th=64.0))).close()
        # the loop refuses what a searchByBF loop refuses
        for call in (lambda: vo.vo.bow_state_dev(), lambda: vo.ctx.check(vo.vo.bow_db_enable(4)),
                     lambda: vo.ctx.check(vo.vo.window_ba_enable(capi.VOWindowBA(10, 1, 2, 3)))):
            with pytest.raises(capi.TBError) as e:
                call()
            assert e.value.code == capi.TB_ESTATE
        L, R, G = seqs
        assert vo.keyframe()["frame"] == -1
        assert vo.step_rc(_dev(L[0])) == capi.TB_ESTATE              # before reset
        vo.reset(G[0])
        assert vo.step_rc(_dev(L[0]), None) == capi.TB_EINVAL        # frame 0 is a keyframe: right images required
        assert vo.step_rc(_dev(L[0]), _dev(R[0])) == 0
        assert vo.step_rc(_dev(L[1]), None) == 0
        assert vo.keyframe()["frame"] == 0
    finally:
        vo.close()
