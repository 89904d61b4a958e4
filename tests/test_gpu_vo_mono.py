"""GPU tests of the mono mode of the optical-flow VO loop (StereoVO(mono=True), tb_vo_mono_enable) against the CPU composition
in tests/vo_mono_reference.py, on synthetic KITTI-geometry sequences (1241 x 376): seeds 0 and 1, keyframe_every = 5, the
right image passed at frame 0 only."""
import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi, synth_seq
from trackingbench_slam_amd.vo import StereoVO

import vo_mono_reference as vm
import vo_reference as vr

pytestmark = pytest.mark.gpu

T = 16
EVERY = 5
SEEDS = (0, 1)
GT_BOUND = 0.25   # tests/test_vo_reference.py


@pytest.fixture(scope="module")
def seqs():
    out = [synth_seq.sequence(s, T) for s in SEEDS]
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1), np.stack([o[2] for o in out], 1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _snapshot(vo, mono=True):
    xy, kc = vo.keys()
    mp, mv = vo.map_points()
    o, oc = vo.obs()
    out = dict(Tcw=vo.Tcw(), xy=xy, kc=kc, mp=mp, mv=mv, obs=o, oc=oc, ninl=vo.n_inliers(), outl=vo.outlier())
    if mono:
        out.update(vo.mono())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _cpu_state(g, s, t, last_img):
    """The GPU's state of sequence s after frame t - 1 as a vo_mono_reference state"""
    n = g["kc"][s]
    return dict(t=t, Tcw=g["Tcw"][s], keys=g["xy"][s, :n].copy(), mp=g["mp"][s, :n].copy(), valid=g["mv"][s, :n].astype(bool),
                last_img=last_img, kf_keys=g["kf_keys"][s, :n].copy(), kf_Tcw=g["kf_Tcw"][s].copy(), alive=g["alive"][s, :n].astype(bool))


def test_step_parity_11_frames(seqs):
    L, R, G = seqs
    S, nframes = L.shape[1], 11
    P = vr.Params(keyframe_every=EVERY)
    vo = StereoVO(S, keyframe_every=EVERY, mono=True)
    accepted = 0
    try:
        M = vm.MonoParams(capacity=vo.key_pitch)
        vo.reset(G[0])
        prev = None
        for t in range(nframes):
            vo.step(_dev(L[t]), _dev(R[t]) if t == 0 else None)
            g = _snapshot(vo)
            for s in range(S):
                where = "frame %d seq %d" % (t, s)
                cpu_in = vm.initial_state(G[0, s]) if t == 0 else _cpu_state(prev, s, t, L[t - 1, s])
                exp, info = vm.step(cpu_in, L[t, s], R[t, s] if t == 0 else None, P, M, tri_Tcw=g["Tcw"][s], spawn_Tcw=g["Tcw"][s])
                n = len(exp["keys"])
                assert g["kc"][s] == n, where
                assert _same_bits(g["xy"][s, :n], exp["keys"]), where
                assert np.array_equal(g["mv"][s, :n].astype(bool), exp["valid"]), where
                assert _same_bits(g["mp"][s, :n][exp["valid"]], exp["mp"][exp["valid"]]), where
                assert np.array_equal(g["alive"][s, :n].astype(bool), exp["alive"]), where
                assert _same_bits(g["kf_keys"][s, :n], exp["kf_keys"]), where
                assert _same_bits(g["kf_Tcw"][s], exp["kf_Tcw"]), where
                no = len(info["obs"])
                assert g["oc"][s] == no, where
                rows = np.stack([info["obs"][k] for k in ("u", "v", "X", "Y", "Z", "inv_sigma2")], -1) if no else np.zeros((0, 6), np.float32)
                assert _same_bits(g["obs"][s, :no], rows), where
                assert g["ninl"][s] == info["n_inliers"], where
                assert np.array_equal(g["outl"][s, :no], info["outlier"][:no]), where
                assert np.allclose(g["Tcw"][s], exp["Tcw"], rtol=1e-6, atol=1e-6), where
                if t and t % EVERY == 0:
                    m = len(info["tri_flags"])
                    assert np.array_equal(g["tri_flags"][s, :m], info["tri_flags"]) and (g["tri_flags"][s, m:] == 0).all(), where
                    assert np.array_equal(g["tri_tally"][s], info["tri_tally"]), where
                    acc = info["tri_flags"] == 1
                    assert _same_bits(g["tri_points"][s, :m][acc], info["tri_points"][acc]), where
                    assert g["survivors"][s] == info["survivors"] and g["added"][s] == info["added"], where
                    accepted += int(acc.sum())
                elif prev is not None:   # the last mono keyframe's outputs stay readable
                    for k in ("tri_flags", "tri_tally", "survivors", "added", "kf_keys", "kf_Tcw"):
                        a, b = (g[k][s, :n], prev[k][s, :n]) if k == "kf_keys" else (g[k][s], prev[k][s])   # past the count: not state
                        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (where, k)
                else:
                    assert not g["tri_flags"][s].any() and not g["tri_tally"][s].any() and g["survivors"][s] == 0 and g["added"][s] == 0
            prev = g
    finally:
        vo.close()
    assert accepted >= 200   # frames 5 and 10 of two sequences (the CPU composition alone: 63 + 230 and 34 + 283)


def test_enabled_loop_equals_a_plain_one_until_the_first_mono_keyframe(seqs):
    L, R, G = seqs
    S = L.shape[1]
    runs = []
    for mono in (None, True):
        vo = StereoVO(S, keyframe_every=EVERY, mono=mono)
        try:
            vo.reset(G[0])
            out = []
            for t in range(EVERY):
                vo.step(_dev(L[t]), _dev(R[t]) if t == 0 else None)
                out.append(_snapshot(vo, mono=False))
            runs.append(out)
        finally:
            vo.close()
    for t in range(EVERY):
        a, b = runs[0][t], runs[1][t]
        for s in range(S):
            n, no = a["kc"][s], a["oc"][s]
            assert b["kc"][s] == n and b["oc"][s] == no and a["ninl"][s] == b["ninl"][s], (t, s)
            assert _same_bits(a["Tcw"][s], b["Tcw"][s]) and _same_bits(a["xy"][s, :n], b["xy"][s, :n]), (t, s)
            assert np.array_equal(a["mv"][s, :n], b["mv"][s, :n]), (t, s)
            v = a["mv"][s, :n] > 0
            assert _same_bits(a["mp"][s, :n][v], b["mp"][s, :n][v]), (t, s)
            assert _same_bits(a["obs"][s, :no], b["obs"][s, :no]) and np.array_equal(a["outl"][s, :no], b["outl"][s, :no]), (t, s)


def test_refusals(seqs):
    L, R, G = seqs

    def code(**kw):
        with pytest.raises(capi.TBError) as e:
            StereoVO(2, keyframe_every=EVERY, **kw)
        return e.value.code

    for kind in ("bf", "violence", "projection"):
        assert code(tracker=kind, mono=True) == capi.TB_EUNSUPPORTED, kind
    assert code(mono=True, window_ba=True) == capi.TB_EUNSUPPORTED            # the window BA first, then mono
    assert code(mono=dict(cell=0)) == capi.TB_EINVAL and code(mono=dict(cell=-8)) == capi.TB_EINVAL
    assert code(mono=dict(cell=1)) == capi.TB_EINVAL                          # 1241 x 376 bits: 58 KB of bitmap
    assert code(mono=dict(chi2_max=float("nan"))) == capi.TB_EINVAL
    vo = StereoVO(2, keyframe_every=EVERY, mono=True)
    try:
        assert vo.vo.window_ba_enable(capi.VOWindowBA(10, 1, 2, 3)) == capi.TB_EUNSUPPORTED    # mono first, then the window BA
        assert vo.vo.mono_enable(capi.VOMono(0.9998, 5.991, 8)) == capi.TB_ESTATE              # enabled already
        assert vo.vo.mono_enable(None) == capi.TB_ESTATE
        vo.reset(G[0])
        T0 = _dev(G[0].reshape(2, 16))
        assert vo.vo.reset_seq_dev([True, False], T0.data_ptr()) == capi.TB_EUNSUPPORTED
        left, right = _dev(L[0]), _dev(R[0])
        assert vo.vo.step_ragged_dev(left.data_ptr(), right.data_ptr(), vo.width, vo.width * vo.height, [True, False]) == capi.TB_EUNSUPPORTED
        assert vo.step_rc(left, None) == capi.TB_EINVAL      # frame 0 fixes the scale: it needs the right images
        assert vo.step_rc(left, right) == 0
        torch.cuda.synchronize()
    finally:
        vo.close()
    plain = StereoVO(2, keyframe_every=EVERY)
    try:
        assert plain.vo.mono_enable(None) == capi.TB_EINVAL
        with pytest.raises(capi.TBError) as e:
            plain.vo.mono_state_dev()
        assert e.value.code == capi.TB_ESTATE
        plain.reset(G[0])
        assert plain.vo.mono_enable(capi.VOMono(0.9998, 5.991, 8)) == capi.TB_ESTATE           # after a reset
    finally:
        plain.close()


def test_free_run_matches_cpu_and_ground_truth(seqs):
    L, R, G = seqs
    S = L.shape[1]
    P = vr.Params(keyframe_every=EVERY)
    vo = StereoVO(S, keyframe_every=EVERY, mono=True)
    try:
        M = vm.MonoParams(capacity=vo.key_pitch)
        vo.reset(G[0])
        traj = []
        for t in range(T):
            vo.step(_dev(L[t]), _dev(R[t]) if t == 0 else None)
            traj.append(vo.Tcw().cpu().numpy())
        tally = vo.mono()["tri_tally"].cpu().numpy()
    finally:
        vo.close()
    for s in range(S):
        states, infos = vm.run(L[:, s], R[:, s], G[0, s], P, M)
        for t in range(T):
            assert np.allclose(traj[t][s], states[t]["Tcw"], rtol=1e-4, atol=1e-4), (s, t)
        assert vr.translation_error(traj[T - 1][s], G[T - 1, s]) < GT_BOUND, s
        assert tally[s, 1] >= 100, s
