"""GPU tests of the depth filter (trackingbench_slam_amd.depth_filter.DepthFilter, tb_depth_filter_*, kernels k_df_update / k_df_add /
k_df_copy / k_df_points) against its definition, tests/depth_filter_reference.py.

After every update the definition is run from the GPU's own previous seed state: the trace's flag, n, winning sample and score
compare exactly, the aligned pixel, z, tau, mu, sigma2, a, b and the points at 1e-6 relative. Where the convergence test
sqrt(sigma2) < z_range / conv_div is within 1e-6 of its threshold the flag (UPDATED or CONVERGED) and the state may differ; such
entries are listed by the test (none on these fixtures so far).

Fixtures: 320 x 96 renders of three sequences, S = 3, ref_slots = 2. "scaled" is KITTI's camera scaled by 320 / 1241: its renders
alias, nearly every search ends at the score gate under the default zmssd_max, and it runs with a loose gate (100000) so that
the alignment and the update are reached; its second sequence offers no key. "crop" is a 320 x 96 window of the full-resolution
camera under the default parameters, where seeds are updated and converge.
"""
import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.depth_filter import DepthFilter
from trackingbench_slam_amd.vo import _DevArray

import depth_filter_cases as dc
import depth_filter_reference as dfr

pytestmark = pytest.mark.gpu

W, H = dc.SMALL_W, dc.SMALL_H
SEEDS = (0, 1, 2)
T = 7
FIXTURES = {"scaled": (dc.SMALL_K, dict(zmssd_max=100000)), "crop": (dc.CROP_K, {})}


@pytest.fixture(scope="module")
def renders():
    out = {}
    for name, (K, _) in FIXTURES.items():
        seqs = [dc.small_sequence(s, T, K) for s in SEEDS]
        P = max(len(q[2]) for q in seqs)
        keys = np.zeros((len(SEEDS), P, 2), np.float32)
        for s, q in enumerate(seqs):
            keys[s, :len(q[2])] = q[2]
        out[name] = dict(L=np.stack([q[0] for q in seqs], 1), G=np.stack([q[1] for q in seqs], 1), keys=keys,
                         counts=np.array([len(q[2]) for q in seqs], np.int32))
    return out


@pytest.fixture(scope="module")
def shared():
    """one context and stream for every filter of this module"""
    host = DepthFilter(1, W, H, dc.CROP_K, pitch=1)
    yield host
    host.close()


class Mirror:
    """The host's copy of a filter's ring images (the poses are read back), kept by the rule of the definition"""

    def __init__(self, df):
        self.df = df
        self.img = np.zeros((df.S, df.ref_slots, H, W), np.uint8)
        self.newest = np.full(df.S, -1, np.int64)

    def add(self, images, active=None):
        for s in range(self.df.S):
            if active is None or active[s]:
                self.newest[s] = (self.newest[s] + 1) % self.df.ref_slots
                self.img[s, self.newest[s]] = images[s]
        Tcw, newest = self.df.slots()
        assert np.array_equal(newest, self.newest)
        return Tcw


def _prm(df_kwargs, ref_slots=2):
    return dfr.Params(ref_slots=ref_slots, **df_kwargs)


def _close(a, b, atol=1e-12):
    return np.allclose(a, b, rtol=1e-6, atol=atol, equal_nan=True)


def check_update(df, mirror, prev, images, Tcw, K, prm, where):
    """The GPU's seeds and traces after an update against the definition run from `prev`, the GPU's seeds before it. Returns the
    entries whose convergence test is within 1e-6 of its threshold."""
    g_seeds, g_tr = df.seeds(), df.trace()
    ring_Tcw, _ = df.slots()
    near = []
    for s in range(df.S):
        exp, tr = dfr.update_all(prev[s], mirror.img[s], ring_Tcw[s], images[s], Tcw[s], K, prm)
        edge = np.array([tr["flag"][e] in (dfr.UPDATED, dfr.CONVERGED) and dfr.convergence_margin(exp[e], prm) < 1e-6
                         for e in range(df.pitch)])
        near += [(where, s, int(e)) for e in np.nonzero(edge)[0]]
        ok = ~edge
        g, gt = g_seeds[s], g_tr[s]
        assert np.array_equal(gt["flag"][ok], tr["flag"][ok]), (where, s, gt["flag"].tolist(), tr["flag"].tolist())
        both = np.isin(gt["flag"], (dfr.UPDATED, dfr.CONVERGED)) & np.isin(tr["flag"], (dfr.UPDATED, dfr.CONVERGED))
        assert both[edge].all(), (where, s)
        for k in ("n", "win", "score"):
            assert np.array_equal(gt[k], tr[k]), (where, s, k)
        assert _close(gt["px"], tr["px"], 1e-6) and _close(gt["py"], tr["py"], 1e-6), (where, s)
        for k in ("z", "tau"):
            assert _close(gt[k], tr[k]), (where, s, k)
        for k in ("mu", "sigma2", "a", "b"):
            assert _close(g[k], exp[k]), (where, s, k)
        for k in ("z_range", "u", "v", "slot", "updates", "reserved"):
            assert np.array_equal(g[k], exp[k]), (where, s, k)
        assert np.array_equal(g["state"][ok], exp["state"][ok]), (where, s)
        # an entry the definition leaves alone keeps every byte
        same = np.array([exp[e].tobytes() == prev[s][e].tobytes() for e in range(df.pitch)])
        assert all(g[e].tobytes() == prev[s][e].tobytes() for e in np.nonzero(same)[0]), (where, s)
    return near


def check_points(df, K, release=False):
    seeds = df.seeds()
    ring_Tcw, _ = df.slots()
    xyz, ok = df.points(release=release)
    xyz, ok = xyz.cpu().numpy(), ok.cpu().numpy()
    for s in range(df.S):
        pts, flags = dfr.points(seeds[s].copy(), ring_Tcw[s], K, False)
        assert np.array_equal(ok[s], flags)
        assert np.allclose(xyz[s], pts, rtol=1e-6, atol=1e-6)
        assert not xyz[s][flags == 0].any()
    after = df.seeds()
    exp = seeds.copy()
    if release:
        exp["state"][ok != 0] = dfr.FREE
    assert after.tobytes() == exp.tobytes()
    return int(ok.sum())


def check_add(df, before, keys, counts, skip, slot, prm, left, active=None):
    """the seeds after an add against the definition's, byte for byte"""
    after = df.seeds()
    left = left.cpu().numpy()
    for s in range(df.S):
        exp = before[s].copy()
        if active is None or active[s]:
            _, na = dfr.add_keyframe(exp, np.zeros((prm.ref_slots, 1, 1), np.uint8), np.zeros((prm.ref_slots, 4, 4), np.float32), slot[s] - 1,
                                     np.zeros((1, 1), np.uint8), np.eye(4), keys[s], counts[s], None if skip is None else skip[s], prm)
            assert left[s] == na, s
        assert after[s].tobytes() == exp.tobytes(), s


@pytest.mark.parametrize("fixture,pitch", [("scaled", 1), ("scaled", 5), ("scaled", 64), ("scaled", 67), ("crop", 67)])
def test_six_updates_against_the_definition(renders, shared, fixture, pitch):
    """pitch 1: a lone seed; 5: a partly filled workgroup; 64: full ones; 67: a tail"""
    K, kw = FIXTURES[fixture]
    R = renders[fixture]
    L, G, keys = R["L"], R["G"], R["keys"]
    counts = R["counts"].copy()
    if fixture == "scaled":
        counts[1] = 0                      # a sequence with 0 keys
    prm = _prm(kw)
    df = DepthFilter(len(SEEDS), W, H, K, pitch=pitch, context=shared, ref_slots=2, **kw)
    try:
        mirror = Mirror(df)
        before = df.seeds()
        assert not before.tobytes().strip(b"\0")
        left = df.add_keyframe(L[0], G[0], keys, counts)
        ring_Tcw = mirror.add(L[0])
        assert np.array_equal(ring_Tcw[:, 0], G[0])
        check_add(df, before, keys, counts, None, mirror.newest, prm, left)
        assert np.array_equal(left.cpu().numpy(), np.maximum(counts - pitch, 0))
        near, flags = [], []
        for t in range(1, T):
            prev = df.seeds()
            df.update(torch.from_numpy(L[t]).cuda(), G[t])
            near += check_update(df, mirror, prev, L[t], G[t], K, prm, "update %d" % t)
            flags += df.trace()["flag"].reshape(-1).tolist()
        print("%s pitch %d: flags %s, near the convergence threshold: %s" % (fixture, pitch, np.bincount(np.array(flags) + 1).tolist(), near))
        if pitch >= 64:                     # the run is about something: seeds are updated, refused and left alone
            assert flags.count(dfr.UPDATED) >= 20 and flags.count(dfr.NO_MATCH) >= 20 and flags.count(dfr.IDLE) >= 1
        if fixture == "crop":
            assert flags.count(dfr.CONVERGED) >= 1 and flags.count(dfr.OUTSIDE) >= 1
        nconv = check_points(df, K)
        assert nconv == flags.count(dfr.CONVERGED) or near
    finally:
        df.close()


def _poke(df, seeds):
    """overwrite the filter's entries (a test's back door: the C ABI lends the pointer read-only)"""
    raw = torch.from_numpy(np.ascontiguousarray(seeds).view(np.uint8).reshape(df.S, df.pitch, dfr.DF_SEED.itemsize).copy())
    with torch.cuda.stream(df.stream):
        dst = torch.as_tensor(_DevArray(df.df.state_dev()["seeds"], raw.shape, "|u1"), device=df.dev)
        dst.copy_(raw.to(df.dev))
    df.stream.synchronize()


@pytest.mark.parametrize("name", ("updated", "converged", "behind", "outside", "warp", "degenerate", "no_line", "max_steps", "line_leaves",
                                  "nonfinite"))
def test_hand_built_seeds(shared, name):
    """max_steps = 8 (NO_MATCH), identical poses (DEGENERATE), a 6 m jump (WARP), a seed at the 5 px margin (OUTSIDE), a line that
    leaves the image, and the other flags: entry 1 of 3 holds the case, entries 0 and 2 stay free"""
    c = dc.hand_cases()[name]
    p = c["prm"]
    kw = dict(max_steps=p.max_steps, zmssd_max=p.zmssd_max, align_iters=p.align_iters)
    df = DepthFilter(1, W, H, dc.CROP_K, pitch=3, context=shared, ref_slots=2, **kw)
    try:
        df.add_keyframe(c["ref"][0][None], c["ref"][1][None], np.zeros((1, 1, 2), np.float32), [0])
        seeds = df.seeds()
        seeds[0, 1] = c["seed"]
        _poke(df, seeds)
        assert df.seeds().tobytes() == seeds.tobytes()
        df.update(c["cur"][0][None], c["cur"][1][None])
        exp, tr = dc.run_case(c)
        g, gt = df.seeds()[0], df.trace()[0]
        assert gt["flag"].tolist() == [dfr.IDLE, c["flag"], dfr.IDLE], gt["flag"]
        for k in ("n", "win", "score"):
            assert gt[k][1] == tr[k], k
        for k in ("px", "py", "z", "tau"):
            assert _close(gt[k][1], tr[k], 1e-6), k
        if c["flag"] in dfr.UNCHANGED or c["flag"] == dfr.NO_MATCH:
            assert g[1].tobytes() == np.array(exp, dfr.DF_SEED).tobytes()      # unchanged, or b + 1 alone: byte for byte
        else:
            for k in ("mu", "sigma2", "a", "b"):
                assert _close(g[k][1], exp[k]), k
            assert g["state"][1] == exp["state"] and g["updates"][1] == exp["updates"]
        assert g[0].tobytes() == seeds[0, 0].tobytes() and g[2].tobytes() == seeds[0, 2].tobytes()
    finally:
        df.close()


def _run(shared, R, K, which, S, at, pitch=40, first_dummy=False, updates=4):
    """sequence `which` of the fixture as sequence `at` of a batch of S -> (seeds, traces) of that sequence after every update"""
    L, G, keys, counts = R["L"], R["G"], R["keys"], R["counts"]
    order = [(which + j - at) % len(SEEDS) for j in range(S)]
    df = DepthFilter(S, W, H, K, pitch=pitch, context=shared, ref_slots=2)
    out = []
    try:
        if first_dummy:      # a keyframe without keys first: the real one lands in slot 1
            df.add_keyframe(L[1][order], G[1][order], keys[order], np.zeros(S, np.int32))
        df.add_keyframe(L[0][order], G[0][order], keys[order], counts[order])
        for t in range(1, 1 + updates):
            df.update(L[t][order], G[t][order])
            out.append((df.seeds()[at].copy(), df.trace()[at].copy()))
    finally:
        df.close()
    return out


def test_a_sequence_gives_the_same_bits_alone_in_a_batch_in_another_slot_and_again(renders, shared):
    K = dc.CROP_K
    R = renders["crop"]
    alone = _run(shared, R, K, 2, 1, 0)
    again = _run(shared, R, K, 2, 1, 0)
    batch = _run(shared, R, K, 2, 3, 1)
    other = _run(shared, R, K, 2, 1, 0, first_dummy=True)
    assert any((tr["flag"] == dfr.UPDATED).any() for _, tr in alone)
    for (s0, t0), (s1, t1), (s2, t2), (s3, t3) in zip(alone, again, batch, other):
        assert s0.tobytes() == s1.tobytes() == s2.tobytes() and t0.tobytes() == t1.tobytes() == t2.tobytes()
        assert (s3["slot"] == 1)[s3["state"] != 0].all() and (s0["slot"] == 0).all()
        s3 = s3.copy()
        s3["slot"] = s0["slot"]
        assert s3.tobytes() == s0.tobytes() and t3.tobytes() == t0.tobytes()


def test_an_inactive_sequence_keeps_every_byte(renders, shared):
    K = dc.CROP_K
    R = renders["crop"]
    L, G, keys, counts = R["L"], R["G"], R["keys"], R["counts"]
    prm = _prm({})
    df = DepthFilter(3, W, H, K, pitch=24, context=shared, ref_slots=2)
    try:
        mirror = Mirror(df)
        df.add_keyframe(L[0], G[0], keys, counts)
        mirror.add(L[0])
        df.update(L[1], G[1])
        for active in ([True, False, True], [False, False, True], [False, True, False], [False, False, False]):
            prev, prev_tr = df.seeds(), df.trace()
            # the inactive sequences' image and pose are rubbish: they must not be read into anything
            img, pose = L[2].copy(), G[2].copy()
            for s in range(3):
                if not active[s]:
                    img[s] = 255 - img[s]
                    pose[s] = np.eye(4)
            df.update(img, pose, active=active)
            g, gt = df.seeds(), df.trace()
            ring_Tcw, _ = df.slots()
            for s in range(3):
                if not active[s]:
                    assert g[s].tobytes() == prev[s].tobytes() and gt[s].tobytes() == prev_tr[s].tobytes(), (active, s)
                else:
                    exp, tr = dfr.update_all(prev[s], mirror.img[s], ring_Tcw[s], L[2, s], G[2, s], K, prm)
                    assert np.array_equal(gt[s]["flag"], tr["flag"]) and np.array_equal(gt[s]["score"], tr["score"]), (active, s)
                    assert _close(g[s]["mu"], exp["mu"]), (active, s)
        # a keyframe for sequence 1 alone: the others keep seeds, ring slot, pose and newest slot
        prev = df.seeds()
        T0, n0 = df.slots()
        left = df.add_keyframe(L[3], G[3], keys, np.minimum(counts, 5), active=[False, True, False])
        T1, n1 = df.slots()
        g = df.seeds()
        assert n1.tolist() == [0, 1, 0] and np.array_equal(T1[[0, 2]], T0[[0, 2]]) and np.array_equal(T1[1, 1], G[3, 1])
        assert g[0].tobytes() == prev[0].tobytes() and g[2].tobytes() == prev[2].tobytes()
        assert (g[1]["slot"] == 1).sum() == min(5, 24 - (prev[1]["state"] != 0).sum()) and left.cpu().numpy()[[0, 2]].tolist() == [0, 0]
        # and its new seeds are matched in the image it was given, the others' in theirs
        mirror.add(L[3], active=[False, True, False])
        prev = df.seeds()
        df.update(L[4], G[4])
        check_update(df, mirror, prev, L[4], G[4], K, prm, "after the masked keyframe")
    finally:
        df.close()


def test_three_keyframes_on_two_slots_and_release(renders, shared):
    """the third keyframe retires the first one's seeds; points(release=True) frees exactly the converged entries, and the next
    keyframe fills them in ascending order"""
    K = dc.CROP_K
    R = renders["crop"]
    L, G, keys, counts = R["L"], R["G"], R["keys"], R["counts"]
    prm = _prm({})
    pitch = 48
    df = DepthFilter(3, W, H, K, pitch=pitch, context=shared, ref_slots=2)
    try:
        mirror = Mirror(df)
        n_first = np.minimum(counts, 30)
        skip = np.zeros(keys.shape[:2], np.uint8)
        skip[:, 3] = 1
        skip[0, 7:11] = 1
        for t, (kk, cc, sk) in enumerate(((keys, n_first, skip), (keys[:, 30:], np.minimum(counts - 30, 12), None),
                                          (keys[:, 10:], np.full(3, 20, np.int32), None))):
            before = df.seeds()
            left = df.add_keyframe(L[2 * t], G[2 * t], kk, cc, skip=sk)
            mirror.add(L[2 * t])
            check_add(df, before, kk, cc, sk, mirror.newest, prm, left)
            g = df.seeds()
            if t == 2:     # the wrap: nothing of the first keyframe is left, the second one's seeds stay
                was_first = (before["state"] != 0) & (before["slot"] == 0)
                kept = (before["state"] != 0) & (before["slot"] == 1)
                assert was_first.any() and kept.any()
                assert all(g[was_first][i].tobytes() != before[was_first][i].tobytes() for i in range(was_first.sum()))
                assert g[kept].tobytes() == before[kept].tobytes()
                assert (g["state"][was_first] != 2).all()
            for dt in (1, 2):
                prev = df.seeds()
                df.update(L[2 * t + dt], G[2 * t + dt])
                check_update(df, mirror, prev, L[2 * t + dt], G[2 * t + dt], K, prm, "keyframe %d + %d" % (t, dt))
        # make sure something is converged, then release it
        seeds = df.seeds()
        for s in range(3):
            act = np.nonzero(seeds[s]["state"] == dfr.ACTIVE)[0][:3]
            seeds["state"][s, act] = dfr.DONE
        _poke(df, seeds)
        nconv = check_points(df, K, release=True)
        assert nconv >= 9
        before = df.seeds()
        assert ((seeds["state"] == dfr.DONE) == ((before["state"] == dfr.FREE) & (seeds["state"] != dfr.FREE))).all()
        left = df.add_keyframe(L[6], G[6], keys, np.full(3, 2, np.int32))
        mirror.add(L[6])
        check_add(df, before, keys, np.full(3, 2, np.int32), None, mirror.newest, prm, left)
    finally:
        df.close()


def test_refusals(shared):
    ctx = shared.ctx
    K = dc.CROP_K

    def rc(**kw):
        a = dict(nseq=1, pitch=4, ref_slots=2, width=W, height=H, params=capi.depth_filter_params())
        a.update(kw)
        try:
            capi.DepthFilter(ctx, a["nseq"], a["pitch"], a["ref_slots"], a["width"], a["height"], K, a["params"]).close()
        except capi.TBError as e:
            return e.code
        return 0

    assert rc() == 0
    for kw in (dict(pitch=0), dict(ref_slots=0), dict(ref_slots=17), dict(params=capi.depth_filter_params(depth_min=0.0)),
               dict(params=capi.depth_filter_params(depth_mean=1.0, depth_min=2.0)), dict(params=capi.depth_filter_params(max_steps=0)),
               dict(params=capi.depth_filter_params(align_iters=-1)), dict(params=capi.depth_filter_params(align_iters=100))):
        assert rc(**kw) == capi.TB_EINVAL, kw
    assert rc(width=15) == capi.TB_EUNSUPPORTED and rc(height=15) == capi.TB_EUNSUPPORTED
    df = capi.DepthFilter(ctx, 1, 4, 2, W, H, K)
    try:
        img = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
        T = torch.eye(4, device="cuda").reshape(1, 16).contiguous()
        torch.cuda.synchronize()
        assert df.update_dev(0, W, W * H, T.data_ptr()) == capi.TB_EINVAL
        assert df.update_dev(img.data_ptr(), W, W * H, 0) == capi.TB_EINVAL
        assert df.update_dev(img.data_ptr(), W - 1, W * H, T.data_ptr()) == capi.TB_EINVAL
        assert df.add_keyframe_dev(0, W, W * H, T.data_ptr(), T.data_ptr(), T.data_ptr(), 1) == capi.TB_EINVAL
        assert df.update_dev(img.data_ptr(), W, W * H, T.data_ptr()) == 0
        torch.cuda.synchronize()
    finally:
        df.close()
