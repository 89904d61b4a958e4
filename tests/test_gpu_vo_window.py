"""GPU tests (pytest -m gpu) of the window BA in the optical-flow VO loop: tb_vo_window_ba_enable / tb_vo_window_state_dev,
StereoVO(window_ba=...) / window(), against tests/vo_window_reference.py. S = 3 at 640 x 240 with 600 keys (key pitch 715: rows fall
off 16-byte boundaries), keyframe_every = 3 (a window is 4 frames), seeds 0..2 of the slow synthetic drive, 7 frames: keyframes at
0, 3 and 6, so two windows.

The segment log, the window and the adoption are compared by their bits. The refined segment is compared with oracle.local_ba run
on the GPU's own window at the project's BA bar (tools/fuzz_parity.py): 1e-6 relative, entries near zero at 1e-6 of
the array's largest entry -- or, for a window the CPU solver itself resolves no closer, within twice the CPU solver's own movement
when its input points change by one ulp."""
import functools

import numpy as np
import pytest

import oracle
import vo_reference as vr
import vo_window_reference as vw
from test_gpu_vo import _dev, _gpu_state, _same_bits
from trackingbench_slam_amd import capi, synth_seq
from trackingbench_slam_amd.vo import StereoVO

pytestmark = pytest.mark.gpu

W, H, K, TARGET, EVERY, T = 640, 240, (360.0, 360.0, 320.0, 120.0), 600, 3, 7
SEEDS = (0, 1, 2)
S = 3
N = EVERY + 1
PITCH = 715


@functools.lru_cache(maxsize=None)
def _sequence(seed):
    """One slow synthetic drive, rendered once per session (tests/test_gpu_gauge.py runs one more seed from other start poses)."""
    return synth_seq.sequence(seed, T, width=W, height=H, K=K, speed=0.1)


def _sequences(seeds):
    out = [_sequence(s) for s in seeds]
    return tuple(np.stack([o[i] for o in out], 1) for i in range(3))   # L, R [T, S, H, W], G [T, S, 4, 4]


@pytest.fixture(scope="module")
def seqs():
    return _sequences(SEEDS)


def _vo(nseq=S, **kw):
    return StereoVO(nseq, width=W, height=H, K=K, target=TARGET, keyframe_every=EVERY, **kw)


def _window(vo):
    w = vo.window()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in w.items()}


def _state(vo):
    """every tensor of tb_vo_state_dev"""
    xy, kc = vo.keys()
    mp, mv = vo.map_points()
    o, oc = vo.obs()
    g = dict(Tcw=vo.Tcw(), xy=xy, kc=kc, mp=mp, mv=mv, obs=o, oc=oc, ninl=vo.n_inliers(), outl=vo.outlier())
    return {k: v.cpu().numpy() for k, v in g.items()}


def _seg_of(w, s, n, kf_t):
    """sequence s's running segment of a window() snapshot as a vo_window_reference segment (n keys, slots 0..w['slots'])"""
    j = w["slots"] + 1
    return dict(kf_t=kf_t, keys=[w["keys"][s, k, :n].copy() for k in range(j)], ok=[w["ok"][s, k, :n].astype(bool) for k in range(j)],
                poses=[w["poses"][s, k].copy() for k in range(j)], pts=w["points"][s, :n].copy(), spawned=w["spawned"][s, :n].astype(bool))


def _obs_rows(obs):
    """oracle.BA_OBS records as the int32 rows window() returns"""
    obs = np.ascontiguousarray(obs)
    return obs.view(np.int32).reshape(len(obs), 5)


def _ba_close(g, e):
    return np.allclose(g, e, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(e).max())))


def _ba_parity(gP, gX, poses, pts, obs, prm, where):
    """the refined segment against oracle.local_ba on the same window; returns (GPU vs CPU, the CPU's 1-ulp movement or None)"""
    eP, eX, st = vw.refine(K, poses, pts, obs, prm)
    dg = max(float(np.abs(gP - eP).max()), float(np.abs(gX - eX).max()))
    if _ba_close(gP, eP) and _ba_close(gX, eX):
        return dg, None, st
    ds = 0.0
    for toward in (1e9, -1e9):
        P2, X2, _ = vw.refine(K, poses, np.nextafter(pts, np.float32(toward)), obs, prm)
        ds = max(ds, float(np.abs(P2 - eP).max()), float(np.abs(X2 - eX).max()))
    print(where, "window misses 1e-6: GPU vs CPU %.3e, CPU vs CPU at +-1 ulp %.3e" % (dg, ds))
    assert dg <= 2.0 * ds, (where, dg, ds)
    return dg, ds, st


def _window_step_parity(seqs, nframes=T, min_obs=518, min_points=132):
    """After every step the CPU step runs from the GPU's previous state, segment included. seqs: (L, R, G) of any number of
    sequences, G[0] the start poses; min_obs / min_points: the floors every window of these drives is known to clear.
    Returns the number of windows closed."""
    L, R, G = seqs
    S, T = L.shape[1], nframes
    P = vr.Params(W, H, K, target=TARGET, keyframe_every=EVERY)
    prm = vw.DEFAULTS
    vo = _vo(S, window_ba=True)
    try:
        assert vo.key_pitch == PITCH
        vo.reset(G[0])
        prev = [vw.initial_state(G[0, s]) for s in range(S)]
        pw, nwin = None, 0
        for t in range(T):
            kf = t % EVERY == 0
            vo.step(_dev(L[t]), _dev(R[t]) if kf else None)
            got, w, g = _gpu_state(vo), _window(vo), _state(vo)
            assert w["nslots"] == N and w["slots"] == t % EVERY, t
            for s in range(S):
                where = "frame %d seq %d" % (t, s)
                cpu_in = dict(prev[s], last_img=L[t - 1, s] if t else None)
                exp, info = vw.step(cpu_in, L[t, s], R[t, s], P, prm)
                n = len(exp["keys"])
                assert g["kc"][s] == n and _same_bits(got[s]["keys"], exp["keys"]), where
                j = t % EVERY or (EVERY if t else 0)      # the slot this frame's tracking half was logged to
                if t:
                    # this frame's slot: the tracked keys, ok, and the pose the tracker gave (the GPU's own, bit for bit)
                    seg = info["window"]["seg"] if kf else exp["seg"]
                    m = len(seg["keys"][j])
                    assert _same_bits(w["keys"][s, j, :m], seg["keys"][j]), where
                    assert np.array_equal(w["ok"][s, j, :m].astype(bool), seg["ok"][j]) and not w["ok"][s, j, m:].any(), where
                    assert np.allclose(w["poses"][s, j], seg["poses"][j], rtol=1e-6, atol=1e-6), where
                    assert seg["ok"][j].sum() >= 100, where     # the synthetic drives track
                    # the earlier slots of the segment keep their bits
                    for k in range(0 if not kf else 1, j):
                        assert w["keys"][s, k].tobytes() == pw["keys"][s, k].tobytes() and w["ok"][s, k].tobytes() == pw["ok"][s, k].tobytes(), where
                        assert w["poses"][s, k].tobytes() == pw["poses"][s, k].tobytes(), where
                if t and not kf:
                    assert w["poses"][s, j].tobytes() == g["Tcw"][s].tobytes(), where
                    assert w["points"][s].tobytes() == pw["points"][s].tobytes() and w["spawned"][s].tobytes() == pw["spawned"][s].tobytes(), where
                    assert w["adopted"][s] == pw["adopted"][s] and w["obs_counts"][s] == pw["obs_counts"][s], where
                if kf and t:
                    nwin += 1
                    win = info["window"]
                    # the window, exactly
                    no = len(win["obs"])
                    assert w["obs_counts"][s] == no and w["n_points"][s] == win["n_points"], where
                    assert np.array_equal(w["obs"][s, :no], _obs_rows(win["obs"])), where
                    assert no >= min_obs and win["n_points"] >= min_points, where
                    # the refined segment against the CPU solver on the GPU's own window
                    poses = np.stack([pw["poses"][s, k] for k in range(EVERY)] + [w["poses"][s, EVERY]])
                    pts = pw["points"][s]                       # all PITCH rows: pt is the key index
                    gobs = w["obs"][s, :no].copy().view(oracle.BA_OBS).reshape(no)
                    dg, ds, st = _ba_parity(w["refined_poses"][s], w["refined_points"][s], poses, pts, gobs, prm, where)
                    print(where, "BA: GPU vs CPU %.3e%s, chi2 %.1f -> %.1f" % (dg, "" if ds is None else " (1-ulp %.3e)" % ds, st[1], st[2]))
                    assert w["stats"][s, 7] == 0 and w["stats"][s, 2] < w["stats"][s, 1], where
                    assert _ba_close(w["refined_poses"][s, 0], poses[0]), where   # the fixed keyframe
                    # adoption: exactly the rule, and the adopted pose is the refined last slot, bit for bit
                    _, adopted = vw.adopt(w["poses"][s, EVERY], w["refined_poses"][s, EVERY], int(w["n_points"][s]), w["stats"][s], prm["min_points"])
                    assert bool(w["adopted"][s]) == adopted and adopted, where
                    assert g["Tcw"][s].tobytes() == w["refined_poses"][s, EVERY].tobytes(), where
                    assert g["Tcw"][s].tobytes() != w["poses"][s, EVERY].tobytes(), where
                if kf:
                    # the keyframe's points against the CPU spawn at the GPU's pose (the adopted one), exactly
                    base = {k: v for k, v in cpu_in.items() if k != "seg"}
                    sp, sinfo = vr.step(base, L[t, s], R[t, s], P, spawn_Tcw=g["Tcw"][s])
                    assert np.array_equal(got[s]["valid"], sp["valid"]) and _same_bits(got[s]["mp"][sp["valid"]], sp["mp"][sp["valid"]]), where
                    # the segment starts: slot 0 = the keyframe
                    d = np.asarray(sinfo["depth"], np.float32)
                    spawned = (d > 0) & np.isfinite(d)
                    assert np.array_equal(w["spawned"][s, :n].astype(bool), spawned) and not w["spawned"][s, n:].any(), where
                    assert w["ok"][s, 0].tobytes() == w["spawned"][s].tobytes(), where
                    assert w["keys"][s, 0, :n].tobytes() == g["xy"][s, :n].tobytes(), where
                    mv = g["mv"][s, :n] > 0
                    assert w["points"][s, :n][mv].tobytes() == g["mp"][s, :n][mv].tobytes(), where
                    assert not w["points"][s, :n][~mv].any() and not w["points"][s, n:].any(), where
                    assert w["poses"][s, 0].tobytes() == g["Tcw"][s].tobytes(), where
                    assert spawned.sum() >= 200, where
                # the next CPU step starts from the GPU's state, segment included
                got[s]["seg"] = _seg_of(w, s, n, t - t % EVERY)
            prev, pw = got, w
    finally:
        vo.close()
    return nwin


def test_step_parity_two_windows(seqs):
    assert _window_step_parity(seqs) == 2 * S


def _run(vo, L, R, G, nframes):
    vo.reset(G[0])
    out = []
    for t in range(nframes):
        vo.step(_dev(L[t]), _dev(R[t]) if t % EVERY == 0 else None)
        out.append((_state(vo), _window(vo) if vo.window_ba else None))
    return out


_LIVE = dict(xy="kc", mv="kc", mp="kc", obs="oc", outl="oc")


def _same_state(a, sa, b, sb, what):
    for k in a:
        x, y = a[k][sa], b[k][sb]
        if k in _LIVE:
            x, y = x[:a[_LIVE[k]][sa]], y[:b[_LIVE[k]][sb]]
        if k == "mp":
            x, y = x[a["mv"][sa, :len(x)] > 0], y[b["mv"][sb, :len(y)] > 0]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def _same_window(a, sa, b, sb, what):
    assert a["slots"] == b["slots"] and a["nslots"] == b["nslots"], what
    for k in a:
        if k in ("slots", "nslots"):
            continue
        x, y = a[k][sa], b[k][sb]
        if k == "obs":
            x, y = x[:a["obs_counts"][sa]], y[:b["obs_counts"][sb]]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def test_batch_independence(seqs):
    """Sequence 1 alone gives the bits it gives inside the batch: state, log, window, refined segment and adoption."""
    L, R, G = seqs
    a, b = _vo(window_ba=True), _vo(1, window_ba=True)
    try:
        together = _run(a, L, R, G, T)
        alone = _run(b, L[:, 1:2], R[:, 1:2], G[:, 1:2], T)
    finally:
        a.close(); b.close()
    for t in range(T):
        _same_state(together[t][0], 1, alone[t][0], 0, ("state", t))
        _same_window(together[t][1], 1, alone[t][1], 0, ("window", t))
    assert together[6][1]["adopted"].all()


def test_a_loop_without_window_ba_is_todays_loop(seqs):
    """A loop without window_ba, stepped beside an enabled one, equals it on every state view up to and including the tracking
    half of the first keyframe step t = 3: the two differ only from the adoption on."""
    L, R, G = seqs
    a, b = _vo(), _vo(window_ba=True)
    try:
        off, on = _run(a, L, R, G, T), _run(b, L, R, G, T)
        with pytest.raises(capi.TBError) as e:
            a.window()
        assert e.value.code == capi.TB_ESTATE
        with pytest.raises(capi.TBError) as e:
            a.vo.window_state_dev()
        assert e.value.code == capi.TB_ESTATE
    finally:
        a.close(); b.close()
    for t in range(EVERY):
        for s in range(S):
            _same_state(off[t][0], s, on[t][0], s, (t, s))
    # frame 3: the tracking half is the same -- rows, outlier flags, inliers, the tracked keys and the tracked pose (the log's slot 3)
    so, sn = off[EVERY][0], on[EVERY][0]
    for s in range(S):
        for k in ("xy", "kc", "obs", "oc", "ninl", "outl"):
            x, y = so[k][s], sn[k][s]
            if k in _LIVE:
                x, y = x[:so[_LIVE[k]][s]], y[:sn[_LIVE[k]][s]]
            assert x.tobytes() == y.tobytes(), (k, s)
        assert on[EVERY][1]["poses"][s, EVERY].tobytes() == so["Tcw"][s].tobytes(), s
        assert on[EVERY][1]["adopted"][s] == 1 and sn["Tcw"][s].tobytes() != so["Tcw"][s].tobytes(), s


def test_status_codes(seqs):
    L, R, G = seqs
    ok = capi.VOWindowBA(10, 1, 2, 3)
    # not an optical-flow loop
    vo = _vo(1, tracker="bf")
    try:
        assert vo.vo.window_ba_enable(ok) == capi.TB_ESTATE
    finally:
        vo.close()
    vo = _vo(1)
    try:
        assert vo.vo.window_ba_enable(None) == capi.TB_EINVAL
        for bad in ((0, 1, 2, 3), (100, 1, 2, 3), (10, 0, 2, 3), (10, EVERY + 1, 2, 3), (10, 1, 1, 3), (10, 1, 2, 0)):
            assert vo.vo.window_ba_enable(capi.VOWindowBA(*bad)) == capi.TB_EINVAL, bad
        assert vo.vo.window_ba_enable(capi.VOWindowBA(10, EVERY, 2, 3)) == 0          # fixed = keyframe_every is the upper end
        assert vo.vo.window_ba_enable(ok) == capi.TB_ESTATE                            # enabled already
        vo.reset(G[0, :1])
        T0 = _dev(G[0, :1].reshape(1, 16).astype(np.float32))
        assert vo.vo.reset_seq_dev([True], T0.data_ptr()) == capi.TB_EUNSUPPORTED
        l, r = _dev(L[0, :1]), _dev(R[0, :1])
        assert vo.vo.step_ragged_dev(l.data_ptr(), r.data_ptr(), W, W * H) == capi.TB_EUNSUPPORTED
        assert vo.vo.step_ragged_dev(l.data_ptr(), r.data_ptr(), W, W * H, active=[True]) == capi.TB_EUNSUPPORTED
        assert vo.vo.step_dev(l.data_ptr(), r.data_ptr(), W, W * H) == 0
        vo.window_ba = dict(vw.DEFAULTS)               # the wrapper refuses the same before any call
        for kw in (dict(active=[0]), dict(keyframe=[0])):
            with pytest.raises(TypeError):
                vo.step(l, r, **kw)
        with pytest.raises(TypeError):
            vo.reset(G[0, :1], which=[0])
    finally:
        vo.close()
    # after the first step
    vo = _vo(1)
    try:
        vo.reset(G[0, :1])
        vo.step(_dev(L[0, :1]), _dev(R[0, :1]))
        assert vo.vo.window_ba_enable(ok) == capi.TB_ESTATE
    finally:
        vo.close()
    # keyframe_every + 1 - fixed > 64: the BA's limit on free keyframes
    vo = StereoVO(1, width=W, height=H, K=K, target=TARGET, keyframe_every=70)
    try:
        assert vo.vo.window_ba_enable(capi.VOWindowBA(10, 6, 2, 3)) == capi.TB_EUNSUPPORTED
        assert vo.vo.window_ba_enable(capi.VOWindowBA(10, 7, 2, 3)) == 0
    finally:
        vo.close()


def test_reset_restarts_the_window_state(seqs):
    """tb_vo_reset_dev on an enabled loop after 5 frames, then 4 frames: every view equals a fresh enabled loop's."""
    L, R, G = seqs
    a, b = _vo(window_ba=True), _vo(window_ba=True)
    try:
        _run(a, L, R, G, 5)
        again, fresh = _run(a, L, R, G, 4), _run(b, L, R, G, 4)
    finally:
        a.close(); b.close()
    for t in range(4):
        for s in range(S):
            _same_state(again[t][0], s, fresh[t][0], s, (t, s))
            _same_window(again[t][1], s, fresh[t][1], s, (t, s))
