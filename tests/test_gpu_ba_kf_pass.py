"""Local BA, the keyframe pass (k_ba.hip, ba_kf_pass): a workgroup owns a contiguous run of a free keyframe's 512-edge chunks
(BA_KFBLK = 1: all of them), its threads carry their 27 sums over the whole run, 512 edges per round with the next rounds'
loads in flight, the workgroup reduces once and writes the total to the run's first chunk slot and zeros to the others.

Windows of 2 fixed + 2 or 3 free keyframes in which free keyframe 2 has exactly n edges, n on both sides of every boundary of
that walk: 1, 255 | 256 | 257 (a thread's second edge of a round), 511 | 512 | 513 (a second round, a second chunk slot),
1024 | 1025 (a third), 1537 (four slots, a one-edge tail round). One more window has a free keyframe that sees a single point. Every window against the FP64 CPU solver (oracle.local_ba) at the bound of tests/test_gpu_ba.py
(1e-6 relative on poses, points and the final chi2, 1e-9 on the initial chi2, equal iteration counts); and bit for bit: a second
run, direct launches against the replayed graph, and a batch (11 windows in the graph, 35 launched directly: neither a multiple
of the 8 windows the pass deals to the XCDs at a time) against the same windows one at a time.

The seeds are chosen on the CPU: the CPU solver accepts every step on these windows (test_windows_hold_the_required_cases), so
a change in the last bits of a sum cannot flip a trial count."""
import functools

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi, synth

K = (718.856, 718.856, 607.1928, 185.2157)
ITERS = 5
NPT = 1600
NFIXED = 2
EDGES = [1, 255, 256, 257, 511, 512, 513, 1024, 1025, 1537]
SINGLE = -1   # the window whose last free keyframe sees one point (keyframe 2 has 700 edges)
# (n, nkf, seed)
WINDOWS = [(1, 4, 1), (255, 5, 2), (256, 4, 3), (257, 5, 4), (511, 4, 5), (512, 5, 6), (513, 4, 7), (1024, 5, 8), (1025, 4, 9),
           (1537, 5, 10), (SINGLE, 5, 11)]
# the batches hold one shape: every n again with 3 free keyframes
BATCH = [(n, 5, 20 + i) for i, n in enumerate(EDGES)] + [(SINGLE, 5, 11)]


@functools.lru_cache(maxsize=None)
def _window(n, nkf, seed):
    """NPT points, every one seen by both fixed keyframes; free keyframe 2 sees n of them (chosen at random), the other free
    keyframes about half each -- the last one a single point in the SINGLE window. Poses, points and their start values are
    synth.ba_problem's; the pixels are the true projections with +-0.5 px of uniform noise."""
    Pt, Pi, Xt, Xi, _ = synth.ba_problem(seed, nkf, NPT, K, obs_per_pt=1)
    rng = np.random.default_rng(5000 + seed)
    sees = np.zeros((nkf, NPT), bool)
    sees[:NFIXED] = True
    sees[2, rng.permutation(NPT)[:(700 if n == SINGLE else n)]] = True
    for k in range(3, nkf):
        sees[k] = rng.random(NPT) < 0.5
    if n == SINGLE:
        sees[nkf - 1] = False
        sees[nkf - 1, int(rng.integers(NPT))] = True
    pt, kf = np.nonzero(sees.T)   # by point, then keyframe
    obs = np.zeros(len(pt), capi.BA_OBS)
    pc = np.einsum("nij,nj->ni", Pt[kf, :3, :3].astype(np.float64), Xt[pt].astype(np.float64)) + Pt[kf, :3, 3]
    assert pc[:, 2].min() > 0.5
    noise = rng.uniform(-0.5, 0.5, (len(pt), 2))
    obs["kf"], obs["pt"], obs["inv_sigma2"] = kf, pt, 1.0
    obs["u"] = pc[:, 0] / pc[:, 2] * K[0] + K[2] + noise[:, 0]
    obs["v"] = pc[:, 1] / pc[:, 2] * K[1] + K[3] + noise[:, 1]
    return Pi, Xi, obs


@functools.lru_cache(maxsize=None)
def _oracle(n, nkf, seed):
    Pi, Xi, obs = _window(n, nkf, seed)
    return oracle.local_ba(K, Pi, NFIXED, Xi, obs, ITERS)


def _close(a, b, tol=1e-6):
    assert np.allclose(a, b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max()))), float(np.abs(a - b).max())


def _check(got, case):
    it, P, X, st = got
    io, Po, Xo, so = _oracle(*case)
    assert it == io
    _close(np.asarray(P).reshape(-1, 4, 4), Po)
    _close(X, Xo)
    assert np.isclose(st[2], so[2], rtol=1e-6, atol=1e-9) and np.isclose(st[1], so[1], rtol=1e-9)


def test_windows_hold_the_required_cases():
    """no GPU: the edge counts are what the GPU tests are about, and the CPU solver accepts every step (stats[4]: trials)"""
    assert [n for n, _, _ in WINDOWS[:-1]] == EDGES and [n for n, _, _ in BATCH[:-1]] == EDGES
    assert {nkf for _, nkf, _ in WINDOWS} == {4, 5}
    for n, nkf, seed in WINDOWS + BATCH:
        Pi, Xi, obs = _window(n, nkf, seed)
        assert len(Xi) == NPT and np.all(np.diff(obs["pt"]) >= 0)
        per_kf = np.bincount(obs["kf"], minlength=nkf)
        assert per_kf[2] == (700 if n == SINGLE else n)
        if n == SINGLE:
            assert per_kf[nkf - 1] == 1
        io, Po, Xo, so = _oracle(n, nkf, seed)
        assert io == ITERS and so[4] == io and so[2] < so[1], (n, nkf, seed, io, so[4])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _direct(ctx, run):
    """run() with the per-kernel timing on: the driver launches directly instead of replaying its graph"""
    ctx.profile_enable(True)
    try:
        return run()
    finally:
        ctx.profile_enable(False)


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _single(ctx, case):
    """one window on its own, through the replayed graph: shared by the tests below"""
    Pi, Xi, obs = _window(*case)
    return ctx.local_ba(K, Pi, NFIXED, Xi, obs, ITERS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "n%d-kf%d" % (c[0], c[1]))
def test_single_window(ctx, case):
    Pi, Xi, obs = _window(*case)
    got = _single(ctx, case)
    _check(got, case)
    assert _same(got, ctx.local_ba(K, Pi, NFIXED, Xi, obs, ITERS)), "second run"
    assert _same(got, _direct(ctx, lambda: ctx.local_ba(K, Pi, NFIXED, Xi, obs, ITERS))), "direct launches against the graph"


def _batch(ctx, W):
    """W windows cycling through BATCH"""
    import torch
    from trackingbench_slam_amd.ba import BatchedLocalBA
    dev = torch.device("cuda", 0)
    ba = BatchedLocalBA(ctx, W, nkf=5, npt=NPT, iters=ITERS, seed=1, device=dev, nfixed=NFIXED, distinct=1)
    wins = [_window(*c) for c in BATCH]
    ba.obs_pitch = max(len(o) for _, _, o in wins)
    obs = np.zeros((W, ba.obs_pitch), capi.BA_OBS)
    cnt = np.zeros(W, np.int32)
    poses = np.zeros((W, 5, 16), np.float32)
    pts = np.zeros((W, NPT, 3), np.float32)
    for w in range(W):
        Pi, Xi, o = wins[w % len(wins)]
        obs[w, :len(o)] = o
        cnt[w] = len(o)
        poses[w] = Pi.reshape(5, 16)
        pts[w] = Xi
    ba.obs = torch.from_numpy(obs.view(np.uint8).reshape(W, ba.obs_pitch, capi.BA_OBS.itemsize)).to(dev)
    ba.counts = torch.from_numpy(cnt).to(dev)
    ba.poses0 = torch.from_numpy(poses).to(dev)
    ba.pts0 = torch.from_numpy(pts).to(dev)

    def run():
        ba.run()
        torch.cuda.synchronize()
        return ba.poses.cpu().numpy().copy(), ba.pts.cpu().numpy().copy(), ba.stats.cpu().numpy().copy()
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("W", [11, 35])   # k_ba_lin in the replayed graph; separate k_ba_points / k_ba_kf launches
def test_batch(ctx, W):
    run = _batch(ctx, W)
    P, X, st = run()
    assert _same((P, X, st), run()), "second run"
    if W <= 32:
        assert _same((P, X, st), _direct(ctx, run)), "direct launches against the graph"
    for w in range(W):
        case = BATCH[w % len(BATCH)]
        _check((int(st[w, 0]), P[w], X[w], st[w]), case)
        i1, P1, X1, s1 = _single(ctx, case)
        assert np.array_equal(P[w].reshape(-1, 4, 4), P1) and np.array_equal(X[w], X1), "window %d: batched against alone" % w
        assert np.array_equal(st[w], s1)
