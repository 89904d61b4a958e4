"""GPU tests (pytest -m gpu) of ragged batches in the VO loop: tb_vo_reset_seq_dev / tb_vo_step_ragged_dev / tb_vo_frames,
StereoVO.reset(which=) / step(active=, keyframe=) / frames(). S = 3 at 640 x 240 with 600 keys (key pitch 715, no multiple of 4: the
copy kernels take their 4-byte and 1-byte lanes), keyframe_every = 3, seeds 0..3 of the slow synthetic drive, 8 frames.

Every tensor of the state views is compared over its live entries (what the counts cover; map points and their descriptors where
the validity flag is set -- the rest is never written and is whatever the allocation held), integers, bytes and floats by their
bits, poses included: a sequence gives the same bits alone and in a batch (test_batch_independence of the tracker tests), so a
sequence of a ragged batch must equal the same sequence run alone, bit for bit.

The staggered schedule: sequence 0 starts at step 0, sequence 1 is reset at step 2, sequence 2 at step 3 and idles
at step 5, sequence 1 is reset again at step 6 into seed 3's frames. With keyframe_every = 3 sequence 0 has its own keyframes at
steps 3 and 6, so those steps carry two keyframes of three sequences (index lists [0, 2] and [0, 1]); the steps that carry one
keyframe among tracking frames are 2 (list [1]) and 5 (list [1], next to an idle sequence)."""
import numpy as np
import pytest

import vo_bow_reference as vb
import vo_reference as vr
from test_gpu_vo_bow import _bow_snapshot, _check_bow, _cpu_bow_state
from test_gpu_vo_desc import _check_step, _dev, _same_bits, _snapshot
from trackingbench_slam_amd import capi, synth, synth_seq
from trackingbench_slam_amd.vo import StereoVO

pytestmark = pytest.mark.gpu

W, H, K, TARGET, EVERY, T = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 3, 8
SEEDS = (0, 1, 2, 3)
S = 3
KINDS = ("opflow", "bf", "violence", "projection", "bow")

# array -> (the count that says how many rows are live, the flag array that says which of those mean something)
_LIVE = dict(Tcw=(None, None), ninl=(None, None), kc=(None, None), oc=(None, None), xy=("kc", None), mv=("kc", None), mp=("kc", "mv"),
             obs=("oc", None), outl=("oc", None),
             ocnt=(None, None), mc=(None, None), fl=(None, None), kf_cnt=(None, None), orb=("ocnt", None), desc=("ocnt", None),
             mt=("mc", None), kf_orb=("kf_cnt", None), kf_desc=("kf_cnt", None), kf_mv=("kf_cnt", None), kf_mp=("kf_cnt", "kf_mv"),
             mp_desc=("kc", "mv"), kf_mp_desc=("kf_cnt", "kf_mv"),
             fv_counts=(None, None), bv_counts=(None, None), kf_fv_counts=(None, None), kf_bv_counts=(None, None),
             word_ids=("ocnt", None), node_ids=("ocnt", None), kf_word_ids=("kf_cnt", None), kf_node_ids=("kf_cnt", None),
             fv_keys=("fv_counts", None), kf_fv_keys=("kf_fv_counts", None), bv_words=("bv_counts", None),
             bv_values=("bv_counts", None), kf_bv_words=("kf_bv_counts", None), kf_bv_values=("kf_bv_counts", None))


@pytest.fixture(scope="module")
def seqs():
    out = [synth_seq.sequence(s, T, width=W, height=H, K=K, speed=0.1) for s in SEEDS]
    return tuple(np.stack([o[i] for o in out], 1) for i in range(3))   # L, R [T, 4, H, W], G [T, 4, 4, 4]


@pytest.fixture(scope="module")
def voc():
    return synth.vocabulary(1, 10, 5)


def _vo(kind, voc, nseq=S, **kw):
    if kind == "bow":
        kw["vocab"] = voc
    return StereoVO(nseq, width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY, tracker=kind, **kw)


def _full(vo):
    """every tensor of tb_vo_state_dev, tb_vo_tracker_state_dev, tb_vo_mp_desc_dev, tb_vo_bow_state_dev, and frames()"""
    if vo.tracker == "opflow":
        xy, kc = vo.keys()
        mp, mv = vo.map_points()
        o, oc = vo.obs()
        g = dict(Tcw=vo.Tcw(), xy=xy, kc=kc, mp=mp, mv=mv, obs=o, oc=oc, ninl=vo.n_inliers(), outl=vo.outlier())
        g = {k: v.cpu().numpy() for k, v in g.items()}
    else:
        g = _snapshot(vo)
        g.pop("kf_frame")
    if vo.tracker == "projection":
        g["mp_desc"], g["kf_mp_desc"] = (x.cpu().numpy() for x in vo.mp_desc())
    if vo.tracker == "bow":
        g.update(_bow_snapshot(vo))
    assert set(g) <= set(_LIVE)
    g["frames"], g["kf_frames"] = vo.frames()
    return g


def _live(g, k, s):
    cnt, flag = _LIVE[k]
    x = g[k][s] if cnt is None else g[k][s, :g[cnt][s]]
    return x if flag is None else x[_live(g, flag, s).astype(bool)]


def _same_seq(a, sa, b, sb, what):
    """sequence sa of snapshot a equals sequence sb of snapshot b, bit for bit"""
    assert a.keys() == b.keys(), what
    for k in a:
        if k in ("frames", "kf_frames"):
            assert a[k][sa] == b[k][sb], (what, k, a[k], b[k])
            continue
        x, y = _live(a, k, sa), _live(b, k, sb)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("kind", KINDS)
def test_null_masks_are_the_lock_step_loop(seqs, voc, kind):
    """7 frames through tb_vo_step_ragged_dev with both masks NULL equal 7 tb_vo_step_dev frames of a second loop after every
    step: frame 0, tracking frames and the keyframes 3 and 6."""
    L, R, G = seqs
    a, b = _vo(kind, voc), _vo(kind, voc)
    try:
        a.reset(G[0, :S]); b.reset(G[0, :S])
        for t in range(7):
            l, r = _dev(L[t, :S]), _dev(R[t, :S]) if t % EVERY == 0 else None
            a.step(l, r)
            assert b.vo.step_ragged_dev(l.data_ptr(), r.data_ptr() if r is not None else None, W, W * H) == 0, t
            ga, gb = _full(a), _full(b)
            for s in range(S):
                _same_seq(gb, s, ga, s, (kind, t, s))
            assert gb["frames"].tolist() == [t] * S and gb["kf_frames"].tolist() == [t - t % EVERY] * S
            assert b.vo.state_dev()["frame"] == t
        assert ga["kc"].min() > 100 and ga["oc"].min() > 3, "the loops tracked"
        assert b.vo.step_dev(_dev(L[7, :S]).data_ptr(), None, W, W * H) == 0, "still a lock-step loop"
    finally:
        a.close(); b.close()


# step -> {slot: (seed, frame)} of the active sequences; resets: step -> {slot: seed}
RESETS = {0: {0: 0}, 2: {1: 1}, 3: {2: 2}, 6: {1: 3}}
IDLE = {5: (2,)}


def _schedule():
    where, out = {}, []
    for step in range(T):
        for slot, seed in RESETS.get(step, {}).items():
            where[slot] = [seed, 0]
        act = {slot: tuple(v) for slot, v in where.items() if slot not in IDLE.get(step, ())}
        out.append(act)
        for slot in act:
            where[slot][1] += 1
    return out


# searchByBF is left out: with these shapes the test's last assertion does not hold for it (seed 3's frame 1 yields no pose row
# against its frame-0 keyframe, in the solo run as in the batch), whatever the batch does
@pytest.mark.parametrize("kind", ("opflow", "violence", "projection", "bow"))
def test_staggered_sequences_equal_their_solo_runs(seqs, voc, kind):
    L, R, G = seqs
    sched = _schedule()
    assert sched[3] == {0: (0, 3), 1: (1, 1), 2: (2, 0)} and sched[5] == {0: (0, 5), 1: (1, 3)} and sched[6][1] == (3, 0)
    vo = _vo(kind, voc)
    solo = {seed: _vo(kind, voc, 1) for seed in SEEDS}
    try:
        want, prev, nkf = {}, None, []
        for step, act in enumerate(sched):
            for slot, seed in RESETS.get(step, {}).items():
                vo.reset(G[0, seed][None], which=[slot])
                solo[seed].reset(G[0, seed][None])
                if prev is not None:   # a reset leaves the other sequences alone
                    g = _full(vo)
                    for s in want:
                        if s != slot:
                            _same_seq(g, s, prev, s, (kind, "reset at", step, s))
                    assert g["frames"][slot] == -1 and g["kf_frames"][slot] == -1 and g["kc"][slot] == 0
                    assert g["Tcw"][slot].tobytes() == G[0, seed].astype(np.float32).tobytes()
            l = np.full((S, H, W), 0xFF, np.uint8); r = np.full((S, H, W), 0xFF, np.uint8)
            kfs = [slot for slot, (seed, t) in act.items() if t % EVERY == 0]
            nkf.append(len(kfs))
            for slot, (seed, t) in act.items():
                l[slot], r[slot] = L[t, seed], R[t, seed]
                solo[seed].step(_dev(L[t, seed][None]), _dev(R[t, seed][None]) if t % EVERY == 0 else None)
                want[slot] = _full(solo[seed])
            vo.step(_dev(l), _dev(r) if kfs else None, active=sorted(act))
            g = _full(vo)
            for slot in want:
                if slot in act:
                    _same_seq(g, slot, want[slot], 0, (kind, "step", step, "slot", slot, act[slot]))
                else:
                    _same_seq(g, slot, prev, slot, (kind, "idle at step", step, "slot", slot))
            prev = g
        assert nkf == [1, 0, 1, 2, 0, 1, 2, 1]
        assert g["frames"].tolist() == [7, 1, 3] and g["kf_frames"].tolist() == [6, 0, 3]
        assert g["kc"].min() > 100 and g["oc"].min() > 3, "every sequence tracked"
        st = vo.vo.state_dev()
        assert st["frame"] == 7 and (kind == "opflow" or vo.vo.tracker_state_dev()["kf_frame"] == 6)
    finally:
        vo.close()
        for v in solo.values():
            v.close()


@pytest.mark.parametrize("kind", ("opflow", "bow"))
def test_forced_keyframe(seqs, voc, kind):
    """force_keyframe for sequence 1 at its frame 2 (off the cadence of 3): the state after that step equals the CPU composition
    run from the GPU's previous state with keyframe_every = 1 (integers and bytes exact, Tcw within 1e-6: the rule of
    tests/test_gpu_vo.py); sequences 0 and 2 equal a run without the flag, bit for bit; the next cadence keyframe still comes."""
    L, R, G = seqs
    a, b = _vo(kind, voc), _vo(kind, voc)
    P1 = vr.Params(width=W, height=H, K=K, target=TARGET, keyframe_every=1)
    try:
        a.reset(G[0, :S]); b.reset(G[0, :S])
        for t in range(2):
            for v in (a, b):
                v.step(_dev(L[t, :S]), _dev(R[t, :S]) if t == 0 else None)
        prev = _full(a)
        prev_d = None if kind == "opflow" else dict(prev, kf_frame=0)
        a.step(_dev(L[2, :S]), _dev(R[2, :S]), keyframe=[1])
        b.step(_dev(L[2, :S]))
        ga, gb = _full(a), _full(b)
        for s in (0, 2):
            _same_seq(ga, s, gb, s, (kind, "unflagged", s))
        assert ga["frames"].tolist() == [2, 2, 2] and ga["kf_frames"].tolist() == [0, 2, 0]
        assert _live(ga, "mp", 1).tobytes() != _live(gb, "mp", 1).tobytes(), "the keyframe changed the sequence's points"
        where = "%s forced keyframe" % kind
        if kind == "opflow":
            n = prev["kc"][1]
            cpu_in = dict(t=2, Tcw=prev["Tcw"][1], keys=prev["xy"][1, :n].copy(), mp=prev["mp"][1, :n].copy(),
                          valid=prev["mv"][1, :n].astype(bool), last_img=L[1, 1])
            exp, info = vr.step(cpu_in, L[2, 1], R[2, 1], P1, spawn_Tcw=ga["Tcw"][1])
            assert info["keyframe"] and (info["depth"] > 0).sum() > 100, "points are spawned at this frame"
            m = ga["kc"][1]
            assert m == len(exp["keys"]) and _same_bits(ga["xy"][1, :m], exp["keys"]), where
            assert np.array_equal(ga["mv"][1, :m].astype(bool), exp["valid"]), where
            assert _same_bits(ga["mp"][1, :m][exp["valid"]], exp["mp"][exp["valid"]]), where
            no = len(info["obs"])
            rows = np.stack([info["obs"][k] for k in ("u", "v", "X", "Y", "Z", "inv_sigma2")], -1)
            assert ga["oc"][1] == no >= 3 and _same_bits(ga["obs"][1, :no], rows), where
            assert ga["ninl"][1] == info["n_inliers"] and np.array_equal(ga["outl"][1, :no], info["outlier"][:no]), where
            assert np.allclose(ga["Tcw"][1], exp["Tcw"], rtol=1e-6, atol=1e-6), where
        else:
            vocx = a.ctx.vocab_export(a.vocab)
            cpu_in = _cpu_bow_state(prev_d, 1, 2)
            exp, info = vb.step(cpu_in, L[2, 1], R[2, 1], P1, vb.Tracker(), vocx, spawn_Tcw=ga["Tcw"][1])
            assert info["keyframe"] and exp["kf"]["frame"] == 2 and (info["depth"] > 0).sum() > 100
            gd = dict(ga, kf_frame=2)
            _check_step(gd, 1, exp, info, where, P1.K, cpu_in["Tcw"])
            _check_bow(gd, 1, exp, where)
            assert a.vo.tracker_state_dev()["kf_frame"] == 2
        # frame 3 is on the cadence: every sequence takes its keyframe, the forced one included
        a.step(_dev(L[3, :S]), _dev(R[3, :S]))
        assert a.frames()[1].tolist() == [3, 3, 3]
    finally:
        a.close(); b.close()


def test_errors_and_edges(seqs, voc):
    L, R, G = seqs
    l0, r0 = _dev(L[0, :S]), _dev(R[0, :S])
    ptr = lambda x: x.data_ptr()
    for kind, kw in (("projection_map", {}), ("bow", dict(keyframe_db=4))):
        vo = _vo(kind, voc, **kw)
        try:
            vo.reset(G[0, :S])
            T0 = _dev(G[0, :S].astype(np.float32).reshape(S, 16))
            assert vo.vo.reset_seq_dev([True] * S, ptr(T0)) == capi.TB_EUNSUPPORTED, kind
            assert vo.vo.step_ragged_dev(ptr(l0), ptr(r0), W, W * H) == capi.TB_EUNSUPPORTED, kind
            with pytest.raises(TypeError):
                vo.step(l0, r0, active=[0])
            with pytest.raises(TypeError):
                vo.reset(G[0, :S], which=[0])
        finally:
            vo.close()
    vo, fresh = _vo("opflow", voc), _vo("opflow", voc)
    try:
        assert vo.vo.step_ragged_dev(ptr(l0), ptr(r0), W, W * H) == capi.TB_ESTATE, "before any reset"
        assert vo.frames()[0].tolist() == [-1] * S
        vo.reset(G[0, :2], which=[True, True, False])
        assert vo.vo.step_ragged_dev(ptr(l0), ptr(r0), W, W * H) == capi.TB_ESTATE, "sequence 2 was never reset"
        assert vo.vo.step_dev(ptr(l0), ptr(r0), W, W * H) == capi.TB_ESTATE, "tb_vo_step_dev in ragged mode"
        assert vo.vo.step_ragged_dev(ptr(l0), None, W, W * H, [1, 1, 0]) == capi.TB_EINVAL, "frame 0 needs the right images"
        assert vo.vo.step_ragged_dev(None, ptr(r0), W, W * H, [1, 1, 0]) == capi.TB_EINVAL
        assert vo.frames()[0].tolist() == [-1] * S, "a refused step counts nothing"
        vo.step(l0, r0, active=[0, 1])
        vo.step(_dev(L[1, :S]), active=[0])
        g = _full(vo)
        assert g["frames"].tolist() == [1, 0, -1] and g["kf_frames"].tolist() == [0, 0, -1]
        assert vo.vo.step_ragged_dev(ptr(l0), None, W, W * H, [0, 0, 0]) == 0, "every sequence idle"
        assert vo.vo.step_ragged_dev(None, None, W, W * H, [0, 0, 0]) == 0, "... and nothing is looked at"
        h = _full(vo)
        for s in range(S):
            _same_seq(h, s, g, s, ("all idle", s))
        # back to lock-step: equal to a loop that never was ragged
        for v in (vo, fresh):
            v.reset(G[0, :S])
            for t in range(4):
                v.step(_dev(L[t, :S]), _dev(R[t, :S]) if t % EVERY == 0 else None)
        g, h = _full(vo), _full(fresh)
        for s in range(S):
            _same_seq(g, s, h, s, ("after tb_vo_reset_dev", s))
        assert g["frames"].tolist() == [3] * S
    finally:
        vo.close(); fresh.close()
