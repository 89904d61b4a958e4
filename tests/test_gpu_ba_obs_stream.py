"""Local BA, the lane-interleaved observation stream of the point passes (k_ba.hip, ba_stream_walk).

Windows of up to 8192 points are renumbered by k_ba_prepare, which also writes their observations as 16-byte entries sliced
by wavefront: the 64 consecutive ranks of one wavefront own one range of the stream, all lanes' observation 0 first, then all
observation 1, ... The point passes read that stream; tb_debug_ba_plain_obs sends them back to the array-of-structs walk.
Both walks visit a point's observations in the same order with the same arithmetic, so every result is equal bit for bit.

CPU: the exported position rule (tb_ba_obs_stream_positions) against a numpy model.
GPU: stream against plain (np.array_equal on poses, points, stats) and against the FP64 CPU solver (1e-6, equal iteration
counts), on windows whose degrees inside one 64-rank block range from 0 to nkf."""
import functools

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi, synth

K = (718.856, 718.856, 607.1928, 185.2157)
ITERS = 6
# (seed, npt, nkf, nfixed): every npt of {1, 63, 64, 65, 130, 700}, nkf 3..10, nfixed 0..2
SHAPES = [(1, 1, 3, 2), (2, 63, 4, 1), (3, 64, 10, 2), (4, 65, 5, 0), (5, 130, 7, 1), (6, 700, 10, 2), (7, 700, 8, 0),
          (8, 64, 6, 1), (9, 130, 9, 0)]


def _ranks(obs, npt, nfixed):
    """k_ba_prepare's renumbering: points by ascending mask of the free keyframes that see them, ties in point order."""
    mask = np.zeros(npt, np.int64)
    free = obs["kf"] >= nfixed
    np.bitwise_or.at(mask, obs["pt"][free], np.int64(1) << (obs["kf"][free] - nfixed).astype(np.int64))
    return np.argsort(mask, kind="stable")   # perm[r] = the point that becomes r


@functools.lru_cache(maxsize=None)
def _window(seed, npt, nkf, nfixed):
    """synth.ba_problem with every keyframe a candidate for every point, then observations removed at random with a keep
    rate of its own per point: degrees from 0 to nkf side by side. From 64 points on: point 0 loses every observation (it
    becomes rank 0, the first lane of block 0), point 2 is seen by every keyframe (the largest mask: the last rank -- lane 63
    of block 0 when npt = 64), and with fixed keyframes point 1 keeps only theirs."""
    Pt, Pi, Xt, Xi, obs = synth.ba_problem(seed, nkf, npt, K, obs_per_pt=nkf)
    rng = np.random.default_rng(1000 + seed)
    keep = rng.random(len(obs)) < rng.uniform(0.2, 1.0, npt)[obs["pt"]]
    if npt >= 64:
        keep &= (obs["pt"] != 0) & (obs["pt"] != 2) & ((obs["pt"] != 1) | (nfixed == 0))
    obs = obs[keep]
    if npt >= 64:
        rows = [(k, 2) for k in range(nkf)] + [(k, 1) for k in range(nfixed)]
        extra = np.zeros(len(rows), capi.BA_OBS)
        for i, (k, p) in enumerate(rows):
            pc = Pt[k, :3, :3].astype(np.float64) @ Xt[p].astype(np.float64) + Pt[k, :3, 3]
            extra[i] = (k, p, pc[0] / pc[2] * K[0] + K[2] + 0.25, pc[1] / pc[2] * K[1] + K[3] - 0.25, 1.0)
        obs = np.concatenate([obs, extra])
        obs = obs[np.lexsort((obs["kf"], obs["pt"]))]
    return Pi, Xi, obs


@functools.lru_cache(maxsize=None)
def _oracle(seed, npt, nkf, nfixed, iters=ITERS):
    Pi, Xi, obs = _window(seed, npt, nkf, nfixed)
    return oracle.local_ba(K, Pi, nfixed, Xi, obs, iters)


def _close(a, b, tol=1e-6):
    assert np.allclose(a, b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max()))), float(np.abs(a - b).max())


def _model_positions(pt_start):
    """the stream position of every observation (CSR order), the layout spelt out in numpy"""
    deg = np.diff(pt_start)
    pos = np.full(int(pt_start[-1]), -1, np.int64)
    for b0 in range(0, len(deg), 64):
        d = deg[b0:b0 + 64]
        at = int(pt_start[b0])
        for j in range(int(d.max(initial=0))):
            lanes = np.nonzero(d > j)[0]                       # the lanes that have slot j, in lane order, no padding
            pos[pt_start[b0 + lanes] + j] = at + np.arange(len(lanes))
            at += len(lanes)
    return pos


def test_stream_positions_match_model():
    rng = np.random.default_rng(7)
    cases = [np.zeros(1, np.int64), np.zeros(70, np.int64), np.full(64, 3), np.arange(64), np.arange(64)[::-1], np.r_[0, np.zeros(62, np.int64), 10]]
    for npt in (1, 2, 63, 64, 65, 127, 128, 130, 700, 1000):
        for hi in (1, 4, 10, 64):
            cases.append(rng.integers(0, hi + 1, npt))
    for deg in cases:
        pt_start = np.r_[0, np.cumsum(deg)].astype(np.int32)
        pos = capi.ba_obs_stream_positions(pt_start)
        assert np.array_equal(pos, _model_positions(pt_start))
        for b0 in range(0, len(deg), 64):                      # a permutation of every block's own range
            lo, hi_ = pt_start[b0], pt_start[min(b0 + 64, len(deg))]
            assert np.array_equal(np.sort(pos[lo:hi_]), np.arange(lo, hi_))


def test_windows_hold_the_required_cases():
    """no GPU: the windows the GPU tests run contain what they are meant to (degrees by rank, as the point passes see them)"""
    seen_zero = seen_fixed_only = seen_first0_lastmax = False
    for seed, npt, nkf, nfixed in SHAPES:
        Pi, Xi, obs = _window(seed, npt, nkf, nfixed)
        assert np.all(np.diff(obs["pt"]) >= 0)
        deg = np.bincount(obs["pt"], minlength=npt)[_ranks(obs, npt, nfixed)]
        degfree = np.bincount(obs["pt"][obs["kf"] >= nfixed], minlength=npt)
        seen_zero |= bool((deg == 0).any())
        seen_fixed_only |= bool(((np.bincount(obs["pt"], minlength=npt) > 0) & (degfree == 0)).any())
        for b0 in range(0, npt - 63, 64):
            seen_first0_lastmax |= deg[b0] == 0 and deg[b0 + 63] == nkf
        if npt >= 64:
            assert deg.min() == 0 and deg.max() == nkf
    assert seen_zero and seen_fixed_only and seen_first0_lastmax


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _both(ctx, run):
    """run() on the stream path and on the plain path"""
    ctx.ba_plain_obs(False)
    a = run()
    ctx.ba_plain_obs(True)
    try:
        b = run()
    finally:
        ctx.ba_plain_obs(False)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("seed,npt,nkf,nfixed", SHAPES)
def test_single_window_stream_equals_plain_and_oracle(ctx, seed, npt, nkf, nfixed):
    Pi, Xi, obs = _window(seed, npt, nkf, nfixed)
    (ig, Pg, Xg, sg), (ip, Pp, Xp, sp) = _both(ctx, lambda: ctx.local_ba(K, Pi, nfixed, Xi, obs, ITERS))
    assert np.array_equal(Pg, Pp) and np.array_equal(Xg, Xp) and np.array_equal(sg, sp)
    io, Po, Xo, so = _oracle(seed, npt, nkf, nfixed)
    assert ig == io
    _close(Pg, Po)
    _close(Xg, Xo)
    assert np.isclose(sg[2], so[2], rtol=1e-6, atol=1e-9) and np.isclose(sg[1], so[1], rtol=1e-9)


def _batch(ctx, W, shapes):
    """a BatchedLocalBA of W windows that cycles through the windows of `shapes` (one npt / nkf / nfixed, several seeds)"""
    import torch
    from trackingbench_slam_amd.ba import BatchedLocalBA
    _, npt, nkf, nfixed = shapes[0]
    dev = torch.device("cuda", 0)
    ba = BatchedLocalBA(ctx, W, nkf=nkf, npt=npt, iters=ITERS, seed=1, device=dev, nfixed=nfixed, distinct=1)
    wins = [_window(*s) for s in shapes]
    ba.obs_pitch = max(len(o) for _, _, o in wins)
    obs = np.zeros((W, ba.obs_pitch), capi.BA_OBS)
    cnt = np.zeros(W, np.int32)
    poses = np.zeros((W, nkf, 16), np.float32)
    pts = np.zeros((W, npt, 3), np.float32)
    for w in range(W):
        Pi, Xi, o = wins[w % len(wins)]
        obs[w, :len(o)] = o
        cnt[w] = len(o)
        poses[w] = Pi.reshape(nkf, 16)
        pts[w] = Xi
    ba.obs = torch.from_numpy(obs.view(np.uint8).reshape(W, ba.obs_pitch, capi.BA_OBS.itemsize)).to(dev)
    ba.counts = torch.from_numpy(cnt).to(dev)
    ba.poses0 = torch.from_numpy(poses).to(dev)
    ba.pts0 = torch.from_numpy(pts).to(dev)
    return ba


@pytest.mark.gpu
@pytest.mark.parametrize("W,shapes", [(5, [(20 + i, 130, 7, 1) for i in range(5)]),    # W <= 32: k_ba_lin in the replayed graph
                                      (33, [(30 + i, 65, 5, 2) for i in range(3)])])   # separate k_ba_points / k_ba_kf launches
def test_batch_stream_equals_plain_and_oracle(ctx, W, shapes):
    import torch
    ba = _batch(ctx, W, shapes)

    def run():
        ba.run()
        torch.cuda.synchronize()
        return ba.poses.cpu().numpy().copy(), ba.pts.cpu().numpy().copy(), ba.stats.cpu().numpy().copy()

    (Pg, Xg, sg), (Pp, Xp, sp) = _both(ctx, run)
    assert np.array_equal(Pg, Pp) and np.array_equal(Xg, Xp) and np.array_equal(sg, sp)
    for w in range(W):
        seed, npt, nkf, nfixed = shapes[w % len(shapes)]
        io, Po, Xo, so = _oracle(seed, npt, nkf, nfixed)
        assert int(sg[w, 0]) == io
        _close(Pg[w].reshape(-1, 4, 4), Po)
        _close(Xg[w], Xo)
        assert np.isclose(sg[w, 2], so[2], rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_rejected_steps_on_the_stream(ctx):
    """a far start (the first case of test_local_ba_rejected_steps): after a rejected step the point pass runs again on the
    same state with the new lambda -- on the stream, with the result of the plain walk and of the CPU solver"""
    Pt, Pi, Xt, Xi, obs = synth.ba_problem(50, 3, 40, K, obs_per_pt=3, pose_noise=3.0, pt_noise=12.0)
    io, Po, Xo, so = oracle.local_ba(K, Pi, 1, Xi, obs, 8)
    assert so[4] > io, "the case is meant to contain rejected steps"
    (ig, Pg, Xg, sg), (ip, Pp, Xp, sp) = _both(ctx, lambda: ctx.local_ba(K, Pi, 1, Xi, obs, 8))
    assert np.array_equal(Pg, Pp) and np.array_equal(Xg, Xp) and np.array_equal(sg, sp)
    assert ig == io
    _close(Pg, Po)
    _close(Xg, Xo)
    assert np.isclose(sg[2], so[2], rtol=1e-6, atol=1e-9) and np.isclose(sg[1], so[1], rtol=1e-9)


@pytest.mark.gpu
def test_rejected_input_in_a_window_that_is_not_renumbered(ctx):
    """More than 8192 points: the window keeps the array-of-structs walk and finds its point records through the rank table,
    which nobody writes once k_ba_setup has rejected the observations -- so no pass may load a record before it has seen the
    window's status. A keyframe index out of range is refused, and the same window without it still runs afterwards."""
    Pt, Pi, Xt, Xi, obs = synth.ba_problem(7, 5, 9000, K)
    bad = obs.copy()
    bad["kf"][len(bad) // 2] = 99
    with pytest.raises(capi.TBError):
        ctx.local_ba(K, Pi, 2, Xi, bad, 3)
    ig, Pg, Xg, sg = ctx.local_ba(K, Pi, 2, Xi, obs, 3)
    assert sg[2] < sg[1]
