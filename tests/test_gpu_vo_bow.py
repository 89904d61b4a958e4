"""GPU tests of the VO loop's searchByBow tracker (StereoVO(tracker="bow", vocab=...), tb_vo_create_bow) against the CPU
composition in tests/vo_bow_reference.py, on synthetic KITTI-geometry sequences (1241 x 376): after every step the CPU step is run
from the GPU's previous state and everything the loop exposes is compared exactly -- doubles as bit patterns -- except Tcw, which
follows the descriptor trackers' rule (tests/test_gpu_vo_desc.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi, synth, synth_seq
from trackingbench_slam_amd.vo import BOW_TEST_VO_1, StereoVO

import vo_bow_reference as vb
import vo_desc_reference as vd
from test_gpu_vo_desc import _check_step, _cpu_state, _dev, _pose_close, _snapshot

pytestmark = pytest.mark.gpu

T = 21
SEEDS = (0, 1, 2, 3)
SETS = {"test_kitti": ({}, vb.Tracker()), "test_vo_1": (BOW_TEST_VO_1, vb.Tracker.test_vo_1())}


@pytest.fixture(scope="module")
def seqs():
    out = [synth_seq.sequence(s, T) for s in SEEDS]
    L = np.stack([o[0] for o in out], 1)   # [T, S, H, W]
    R = np.stack([o[1] for o in out], 1)
    G = np.stack([o[2] for o in out], 1)   # [T, S, 4, 4]
    return L, R, G


@pytest.fixture(scope="module")
def orb_cache(seqs):
    """the CPU extraction of frame (t, s), shared by every configuration (each GPU step is compared against it)"""
    L = seqs[0]
    cache = {}

    def get(t, s):
        if (t, s) not in cache:
            cache[(t, s)] = vd.extract(L[t, s], vd.Params())
        return cache[(t, s)]
    return get


def _train_on_frame_0(orb_cache, S, L=5):
    """vocab=: a callable that trains on the loop's context with tb_vocab_train_dev, on frame 0's descriptors of every sequence"""
    docs = [orb_cache(0, s)[1] for s in range(S)]
    pitch = max(len(d) for d in docs) + 3
    D = np.zeros((S, pitch, 32), np.uint8)
    for s, d in enumerate(docs):
        D[s, :len(d)] = d
    cnt = np.array([len(d) for d in docs], np.int32)
    return lambda ctx: ctx.vocab_train_dev(_dev(D), _dev(cnt), k=10, L=L, weighting=0, scoring=0, seed=5)[0]


def _vocab(which, orb_cache, S):
    if which == "synth":
        return synth.vocabulary(1, 10, 5)
    if which == "ragged":
        return synth.vocabulary(2, 10, 5, stop_frac=0.05, ragged=0.3)
    return _train_on_frame_0(orb_cache, S)


def _bow_snapshot(vo):
    (fv, kfv), (bv, kbv) = vo.feature_vector(), vo.bow_vector()
    out = {}
    for pre, d in (("", fv), ("kf_", kfv), ("", bv), ("kf_", kbv)):
        out.update({pre + k: v.cpu().numpy() for k, v in d.items()})
    return out


def _snap(vo):
    g = _snapshot(vo)
    g.update(_bow_snapshot(vo))
    return g


def _bow_of(g, s, pre, n):
    """the vectors of the current frame (pre "") or the keyframe ("kf_") of sequence s as vo_bow_reference keeps them"""
    nf, nb = g[pre + "fv_counts"][s], g[pre + "bv_counts"][s]
    return dict(word_ids=g[pre + "word_ids"][s, :n].copy(), node_ids=g[pre + "node_ids"][s, :n].copy(),
                fv=vb.fv_from_keys(g[pre + "fv_keys"][s, :nf].view(np.uint64)),
                bv=dict(zip(g[pre + "bv_words"][s, :nb].tolist(), g[pre + "bv_values"][s, :nb].tolist())))


def _cpu_bow_state(g, s, t):
    st = _cpu_state(g, s, t)
    if st["kf"] is not None:
        st["kf"]["bow"] = _bow_of(g, s, "kf_", g["kf_cnt"][s])
    return st


def _same_bow(got, exp, where):
    assert np.array_equal(got["word_ids"], exp["word_ids"]) and np.array_equal(got["node_ids"], exp["node_ids"]), where
    assert got["fv"] == exp["fv"] and list(got["fv"]) == sorted(exp["fv"]), where
    assert list(got["bv"]) == list(exp["bv"]), where
    assert np.array_equal(np.array(list(got["bv"].values()), np.float64).view(np.uint64),
                          np.array(list(exp["bv"].values()), np.float64).view(np.uint64)), where


def _check_bow(g, s, exp, where):
    n = len(exp["orb"])
    cur = _bow_of(g, s, "", n)
    _same_bow(cur, exp["bow"], where)
    assert g["fv_counts"][s] == int((exp["bow"]["weights"] > 0).sum()), where
    k = len(exp["kf"]["orb"])
    _same_bow(_bow_of(g, s, "kf_", k), exp["kf"]["bow"], where + " keyframe")


def _step_parity(seqs, orb_cache, vocab, params, tr, nframes, keyframe_every, S=None, seq0=0):
    L, R, G = seqs
    S = L.shape[1] if S is None else S
    sl = slice(seq0, seq0 + S)
    P = vd.Params(keyframe_every=keyframe_every)
    vo = StereoVO(S, keyframe_every=keyframe_every, tracker="bow", vocab=vocab, **params)
    tracked, matched, stopped = 0, 0, 0
    try:
        voc = vo.ctx.vocab_export(vo.vocab)
        vo.reset(G[0, sl])
        prev = None
        for t in range(nframes):
            kf = t % keyframe_every == 0
            vo.step(_dev(L[t, sl]), _dev(R[t, sl]) if kf else None)
            g = _snap(vo)
            for s in range(S):
                cpu_in = vd.initial_state(G[0, seq0 + s]) if t == 0 else _cpu_bow_state(prev, s, t)
                exp, info = vb.step(cpu_in, L[t, seq0 + s], R[t, seq0 + s], P, tr, voc, spawn_Tcw=g["Tcw"][s], orb=orb_cache(t, seq0 + s))
                where = "bow frame %d seq %d" % (t, seq0 + s)
                _check_step(g, s, exp, info, where, P.K, cpu_in["Tcw"])
                _check_bow(g, s, exp, where)
                q = info["matches"]["queryIdx"]
                assert len(np.unique(q)) == len(q), where
                tracked += t > 0 and len(info["obs"]) > 3
                matched += len(q)
                stopped += int((exp["bow"]["weights"] == 0).sum())
            prev = g
    finally:
        vo.close()
    return voc, tracked, matched, stopped


@pytest.mark.parametrize("pset", list(SETS))
@pytest.mark.parametrize("which", ["synth", "ragged", "trained"])
def test_step_parity_21_frames(seqs, orb_cache, which, pset):
    params, tr = SETS[pset]
    S = seqs[0].shape[1]
    voc, tracked, matched, stopped = _step_parity(seqs, orb_cache, _vocab(which, orb_cache, S), params, tr, T, 10)
    print("%s / %s: %d nodes, %d matches over the run, %d steps tracked, %d stopped features" % (which, pset, voc.nnodes, matched, tracked, stopped))
    assert matched > 0
    if which == "ragged":
        assert stopped > 0
        leaves = np.flatnonzero(np.diff(voc.child_start) == 0)
        assert len(leaves) < 10 ** 5       # some branches end above level L


def test_step_parity_keyframe_every_3(seqs, orb_cache):
    params, tr = SETS["test_kitti"]
    _, tracked, matched, _ = _step_parity(seqs, orb_cache, _vocab("ragged", orb_cache, 4), params, tr, 10, 3)
    assert matched > 0


def test_root_node_one_group_of_all_keys(seqs, orb_cache):
    """L = 4 with levelsup 4: the FeatureVector's node is the root, so searchByBow compares every key with every keyframe key
    (about 2000 x 2000 descriptor pairs per sequence). S = 1."""
    params, tr = SETS["test_kitti"]
    voc, tracked, matched, _ = _step_parity(seqs, orb_cache, synth.vocabulary(4, 10, 4), params, tr, 3, 10, S=1)
    assert voc.L == 4 and matched > 0


def _run_all(vo, L, R, G, nframes, every):
    vo.reset(G[0])
    out = []
    for t in range(nframes):
        vo.step(_dev(L[t]), _dev(R[t]) if t % every == 0 else None)
        out.append(_snap(vo))
    return out


def test_batch_independence(seqs):
    """a sequence gives the same bits alone and in a batch"""
    L, R, G = seqs
    S, n, every = L.shape[1], 7, 3
    voc = synth.vocabulary(2, 10, 5, stop_frac=0.05, ragged=0.3)
    vo = StereoVO(S, keyframe_every=every, tracker="bow", vocab=voc)
    try:
        together = _run_all(vo, L, R, G, n, every)
    finally:
        vo.close()
    rows = dict(xy="kc", mp="kc", mv="kc", orb="ocnt", desc="ocnt", mt="mc", obs="oc", outl="oc", kf_orb="kf_cnt", kf_desc="kf_cnt",
                kf_mp="kf_cnt", kf_mv="kf_cnt", word_ids="ocnt", node_ids="ocnt", fv_keys="fv_counts", bv_words="bv_counts",
                bv_values="bv_counts", kf_word_ids="kf_cnt", kf_node_ids="kf_cnt", kf_fv_keys="kf_fv_counts", kf_bv_words="kf_bv_counts",
                kf_bv_values="kf_bv_counts")
    for s in range(S):
        one = StereoVO(1, keyframe_every=every, tracker="bow", vocab=voc)
        try:
            alone = _run_all(one, L[:, s:s + 1], R[:, s:s + 1], G[:, s:s + 1], n, every)
        finally:
            one.close()
        for t in range(n):
            a, b = together[t], alone[t]
            assert a["kf_frame"] == b["kf_frame"], (s, t)
            for key in ("Tcw", "kc", "oc", "ninl", "ocnt", "mc", "fl", "kf_cnt", "fv_counts", "bv_counts", "kf_fv_counts", "kf_bv_counts"):
                assert np.array_equal(a[key][s:s + 1].view(np.uint8), b[key][0:1].view(np.uint8)), (key, s, t)
            for key, cnt in rows.items():
                k = a[cnt][s]
                x, y = a[key][s, :k], b[key][0, :k]
                if key in ("mp", "kf_mp"):   # entries without a map point are not part of the state
                    v = a["mv" if key == "mp" else "kf_mv"][s, :k] > 0
                    x, y = x[v], y[v]
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (key, s, t)


def test_free_run_matches_cpu(seqs, orb_cache):
    L, R, G = seqs
    S = L.shape[1]
    params, tr = SETS["test_kitti"]
    voc = synth.vocabulary(1, 10, 5)
    vo = StereoVO(S, tracker="bow", vocab=voc)
    try:
        vo.reset(G[0])
        traj = []
        for t in range(T):
            vo.step(_dev(L[t]), _dev(R[t]) if t % 10 == 0 else None)
            traj.append(vo.Tcw().cpu().numpy())
    finally:
        vo.close()
    P = vd.Params()
    for s in range(S):
        st = vd.initial_state(G[0, s])
        for t in range(T):
            st, _ = vb.step(st, L[t, s], R[t, s], P, tr, voc, orb=orb_cache(t, s))
            assert _pose_close(traj[t][s], st["Tcw"], 1e-4), (s, t)


def test_argument_checks_and_ownership(seqs):
    L, R, G = seqs
    voc = synth.vocabulary(1, 10, 5)

    def code(**kw):
        with pytest.raises(capi.TBError) as e:
            StereoVO(2, tracker="bow", vocab=voc, **kw)
        return e.value.code

    for bad in (dict(histo_len=0), dict(histo_len=1025), dict(levelsup=-1), dict(th_low=-1)):
        assert code(**bad) == capi.TB_EINVAL, bad
    with pytest.raises(ValueError):
        StereoVO(2, tracker="bow")                                   # no vocabulary
    with pytest.raises(TypeError):
        StereoVO(2, tracker="violence", vocab=voc)
    with pytest.raises(TypeError):
        StereoVO(2, tracker="bow", vocab=voc, radius=5.0)
    for kw in (dict(histo_len=1), dict(histo_len=1024, levelsup=0, th_low=0)):
        StereoVO(2, tracker="bow", vocab=voc, **kw).close()
    # a handle is borrowed and belongs to the context= it was made on; a null or foreign vocabulary is refused
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    other = capi.Context(0)
    try:
        h = ctx.vocab_create(voc)
        with pytest.raises(ValueError):
            StereoVO(2, tracker="bow", vocab=h)
        vo = StereoVO(2, tracker="bow", vocab=h, context=ctx)
        prm, bow = vo.params, capi.VOBow(4, 1, 50, 6.0, 30, 1)
        out = C.c_void_p()
        lib = capi.lib()
        assert lib.tb_vo_create_bow(ctx._h, C.byref(prm), C.byref(bow), None, 2, C.byref(out)) == capi.TB_EINVAL and not out.value
        assert lib.tb_vo_create_bow(other._h, C.byref(prm), C.byref(bow), h, 2, C.byref(out)) == capi.TB_EINVAL and not out.value
        assert lib.tb_vo_create_bow(ctx._h, C.byref(prm), C.byref(capi.VOBow()), h, 2, C.byref(out)) == capi.TB_EINVAL and not out.value
        tr = capi.VOTracker()
        tr.kind, tr.histo_len, tr.th_low, tr.nratio = capi.TB_VO_BOW, 30, 50, 6.0
        assert lib.tb_vo_create_ex(ctx._h, C.byref(prm), C.byref(tr), 2, C.byref(out)) == capi.TB_EINVAL and not out.value
        try:
            assert vo.keyframe()["frame"] == -1
            assert vo.step_rc(_dev(L[0, :2])) == capi.TB_ESTATE          # before reset
            vo.reset(G[0, :2])
            assert vo.step_rc(_dev(L[0, :2]), None) == capi.TB_EINVAL    # frame 0 is a keyframe
            assert vo.step_rc(_dev(L[0, :2]), _dev(R[0, :2])) == 0
            assert vo.step_rc(_dev(L[1, :2]), None) == 0
            assert vo.keyframe()["frame"] == 0
            fv, kfv = vo.feature_vector()
            assert (fv["fv_counts"] > 1000).all() and (kfv["fv_counts"] > 1000).all()
            assert int(vo.matches()[1].sum()) > 0
        finally:
            vo.close()
        # the context and the handle are still the caller's
        wid, _, _ = ctx.bow_transform(h, np.zeros((3, 32), np.uint8), 4)
        assert len(wid) == 3
        ctx.vocab_destroy(h)
        # the other trackers have no BoW state
        v2 = StereoVO(2, tracker="violence")
        try:
            with pytest.raises(capi.TBError) as e:
                v2.feature_vector()
            assert e.value.code == capi.TB_ESTATE
        finally:
            v2.close()
    finally:
        ctx.close()
        other.close()
