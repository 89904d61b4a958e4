"""Local BA, the host driver (k_ba.hip: BaPlan, ba_enqueue_head / ba_enqueue_round, ba_graph) and tb_lds_limit.

Zero iterations: no LM trial is queued on either path (replayed graph for up to 32 windows, direct launches above that or
with the per-kernel timing on), so the driver must not read a still-running counter that no trial wrote; the call returns the
input as the set-up stored it (poses through their quaternion form: the oracle's iters = 0 result, within 1.9e-9 of the
input), and the context is fit for ordinary calls afterwards.

Dynamic-LDS limits: k_ba_prepare needs 16 npt + 16 bytes and k_ba_solve_big 8 (np + 1) 33 bytes, above the 64 KB default
from npt = 4100 and from 42 free keyframes on. The limit belongs to the (kernel, device) pair, not to the call: a small
window between two large ones, and a second context in the same process, must leave the large ones working.

Expected values: the FP64 CPU solver (oracle.local_ba), 1e-6 relative, the project's BA bound (tests/test_gpu_ba.py)."""
import functools

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi, synth

pytestmark = pytest.mark.gpu
K = (718.856, 718.856, 607.1928, 185.2157)
# (nkf, nfixed, npt): the small path, and the first size with more than 10 free keyframes (block-pair Schur, panel solve)
ZERO_WINDOWS = [(3, 1, 64), (13, 2, 64)]
BATCH_SEED = 7   # BatchedLocalBA(seed=s, distinct=1) holds synth.ba_problem(100 s, ...) in every window


@functools.lru_cache(maxsize=None)
def _problem(seed, nkf, npt):
    Pt, Pi, Xt, Xi, obs = synth.ba_problem(seed, nkf, npt, K)
    return Pi, Xi, obs


@functools.lru_cache(maxsize=None)
def _oracle(seed, nkf, nfixed, npt, iters):
    Pi, Xi, obs = _problem(seed, nkf, npt)
    return oracle.local_ba(K, Pi, nfixed, Xi, obs, iters)


def _close(a, b, tol=1e-6):
    assert np.allclose(a, b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max()))), float(np.abs(a - b).max())


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _check(got, seed, nkf, nfixed, npt, iters):
    """one window's (iterations, poses, points, stats) against the CPU solver"""
    it, P, X, st = got
    io, Po, Xo, so = _oracle(seed, nkf, nfixed, npt, iters)
    assert st[7] == 0, "rejected-input flag"
    assert it == io and (iters or it == 0)
    _close(np.asarray(P).reshape(-1, 4, 4), Po)
    _close(X, Xo)
    if iters:   # the CPU solver computes chi2 inside its loop: with no round there is none to compare
        assert np.isclose(st[2], so[2], rtol=1e-6, atol=1e-9) and np.isclose(st[1], so[1], rtol=1e-9)


def _single(ctx, seed, nkf, nfixed, npt, iters):
    Pi, Xi, obs = _problem(seed, nkf, npt)
    _check(ctx.local_ba(K, Pi, nfixed, Xi, obs, iters), seed, nkf, nfixed, npt, iters)   # raises unless the call returned OK


@pytest.mark.parametrize("nkf,nfixed,npt", ZERO_WINDOWS)
@pytest.mark.parametrize("prof", [False, True])   # W = 1: the graph path; with the timing on: direct launches
def test_zero_iterations_single_window(ctx, nkf, nfixed, npt, prof):
    seed = 100 * BATCH_SEED
    ctx.profile_enable(prof)
    try:
        _single(ctx, seed, nkf, nfixed, npt, 0)
    finally:
        ctx.profile_enable(False)
    _single(ctx, seed, nkf, nfixed, npt, 5)   # captures
    _single(ctx, seed, nkf, nfixed, npt, 5)   # replays the cached graph


@pytest.mark.parametrize("nkf,nfixed,npt", ZERO_WINDOWS)
def test_zero_iterations_direct_batch(ctx, nkf, nfixed, npt):
    """33 windows, the smallest batch that launches directly, every window the same problem"""
    import torch
    from trackingbench_slam_amd.ba import BatchedLocalBA
    W = 33
    ba = BatchedLocalBA(ctx, W, nkf=nkf, npt=npt, iters=0, seed=BATCH_SEED, device=torch.device("cuda", 0), nfixed=nfixed, distinct=1)
    for iters in (0, 5, 5):
        ba.iters = iters
        ba.run()   # raises unless the call returned OK
        torch.cuda.synchronize()
        P, X, st = ba.poses.cpu().numpy(), ba.pts.cpu().numpy(), ba.stats.cpu().numpy()
        for w in range(W):
            _check((int(st[w, 0]), P[w], X[w], st[w]), 100 * BATCH_SEED, nkf, nfixed, npt, iters)


def test_lds_limits_only_rise(ctx):
    """seed, nkf, nfixed, npt in call order; iters = 2. k_ba_prepare: 16 x 4100 + 16 = 65 616 bytes, the first size above
    64 KB; k_ba_solve_big with 42 free keyframes: 253 x 33 x 8 = 66 792 bytes, the first size above 64 KB."""
    big_pts, small, big_kf, mid_kf = (41, 5, 2, 4100), (42, 5, 2, 64), (43, 44, 2, 400), (44, 13, 2, 400)
    for case in (big_pts, small, big_pts, big_kf, mid_kf, big_kf):
        _single(ctx, *case, 2)
    other = capi.Context(0)
    try:
        _single(other, 45, 5, 2, 8192, 2)   # the largest renumbered window: 131 088 bytes
        _single(ctx, *big_pts, 2)
    finally:
        other.close()
