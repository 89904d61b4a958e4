"""GPU parity tests (pytest -m gpu): Hamming matchers (bit-exact) and pose optimisation (1e-6 relative,
the tolerance BASELINE.json's north_star states for BA pose / reprojection error)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

K = (718.856, 718.856, 607.1928, 185.2157)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _eq_struct(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f


def test_bf_golden(ctx, golden):
    for tag in ("c5", "c8"):
        d1, d2 = golden[f"{tag}_desc_left"], golden[f"{tag}_desc_right"]
        _eq_struct(ctx.bf_match(d1, d2, True), golden[f"{tag}_bf_all"])
        _eq_struct(ctx.search_by_bf(d1, d2, 10, 30), golden[f"{tag}_bf_10_30"])
        _eq_struct(ctx.bf_match(d1, d2, False), oracle.bf_match(d1, d2, False))


def test_bf_ties_empty_ragged(ctx):
    rng = np.random.default_rng(5)
    d1 = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (1300, 32), dtype=np.uint8)
    d2[:300] = d1[100:400]      # exact duplicates: zero distances and index ties
    d2[600:650] = d1[5]         # many trains pointing at one query
    d2[5] ^= 1
    for a, b in ((d1, d2), (d2, d1), (d1[:1], d2), (d1, d2[:1]), (d1[:257], d2[:513])):
        _eq_struct(ctx.bf_match(a, b, True), oracle.bf_match(a, b, True))
        _eq_struct(ctx.bf_match(a, b, False), oracle.bf_match(a, b, False))
        _eq_struct(ctx.search_by_bf(a, b, 10, 30), oracle.search_by_bf(a, b, 10, 30))
        _eq_struct(ctx.search_by_bf(a, b, 1.5, 300), oracle.search_by_bf(a, b, 1.5, 300))
    assert len(ctx.bf_match(d1[:0], d2)) == 0 and len(ctx.bf_match(d1, d2[:0])) == 0


def test_violence_golden_and_params(ctx, golden):
    for tag, nl in (("c5", 5), ("c8", 8)):
        k1, d1 = golden[f"{tag}_kps_left"], golden[f"{tag}_desc_left"]
        k2, d2 = golden[f"{tag}_kps_right"], golden[f"{tag}_desc_right"]
        _eq_struct(ctx.search_by_violence(k1, d1, k2, d2, 1241, 376, 0, nl, 50.0, th_low=30, nratio=5.0, histo_len=30,
                                          check_orientation=True), golden[f"{tag}_violence"])
        for kw in (dict(min_level=0, max_level=1, radius=10.0, th_low=50, nratio=0.9, histo_len=30, check_orientation=False),
                   dict(min_level=1, max_level=3, radius=80.0, th_low=60, nratio=0.8, histo_len=30, check_orientation=True),
                   dict(min_level=0, max_level=-1, radius=25.0, th_low=100, nratio=1.0, histo_len=45, check_orientation=True)):
            _eq_struct(ctx.search_by_violence(k1, d1, k2, d2, 1241, 376, **kw),
                       oracle.search_by_violence(k1, d1, k2, d2, 1241, 376, **kw))
    # HISTO_LENGTH is both the bin count and the divisor (matcher.cpp:315,364): below 19 the reference's
    # assert(bin < HISTO_LENGTH) fires; the C ABI reports it instead of writing out of range
    with pytest.raises(capi.TBError) as e:
        ctx.search_by_violence(k1, d1, k2, d2, 1241, 376, 0, 8, 50.0, th_low=100, nratio=1.0, histo_len=12)
    assert e.value.code == capi.TB_EUNSUPPORTED
    with pytest.raises(oracle.OracleError):
        oracle.search_by_violence(k1, d1, k2, d2, 1241, 376, 0, 8, 50.0, th_low=100, nratio=1.0, histo_len=12)
    assert len(ctx.search_by_violence(k1[:0], d1[:0], k2, d2, 1241, 376)) == 0
    assert len(ctx.search_by_violence(k1, d1, k2[:0], d2[:0], 1241, 376)) == 0



def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw_violence(ctx, k1, d1, k2, d2, cap, histo_len=30):
    """tb_search_by_violence through the raw C ABI: (return code, *count, out[:cap])."""
    k1 = np.ascontiguousarray(k1, capi.KEYPOINT); k2 = np.ascontiguousarray(k2, capi.KEYPOINT)
    d1, d2 = np.ascontiguousarray(d1, np.uint8), np.ascontiguousarray(d2, np.uint8)
    out = np.zeros(max(cap, 1), capi.MATCH); n = C.c_int(-7)
    rc = capi.lib().tb_search_by_violence(ctx._h, _ptr(k1), _ptr(d1), len(k1), _ptr(k2), _ptr(d2), len(k2), 1241, 376, 0, 8,
                                          C.c_float(50.0), 100, C.c_float(1.0), histo_len, 1, _ptr(out), cap, C.byref(n))
    return rc, n.value, out[:cap]


def test_violence_capacity_and_bounds(ctx, golden):
    """The host form's capacity contract: cap = count - 1 -> TB_ECAPACITY with the full count, cap = count -> the oracle's
    list; histo_len above the batched kernels' 1024 bins is rejected."""
    k1, d1, k2, d2 = (golden[f"c8_{x}"] for x in ("kps_left", "desc_left", "kps_right", "desc_right"))
    exp = oracle.search_by_violence(k1, d1, k2, d2, 1241, 376, 0, 8, 50.0, th_low=100, nratio=1.0, histo_len=30)
    assert len(exp) > 1
    rc, n, _ = _raw_violence(ctx, k1, d1, k2, d2, len(exp) - 1)
    assert rc == capi.TB_ECAPACITY and n == len(exp)
    rc, n, out = _raw_violence(ctx, k1, d1, k2, d2, len(exp))
    assert rc == capi.TB_OK and n == len(exp)
    _eq_struct(out, exp)
    assert _raw_violence(ctx, k1, d1, k2, d2, len(exp), histo_len=1025)[0] == capi.TB_EINVAL

def _pose_close(a, b):
    assert np.allclose(a, b, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(b).max())))


def test_pose_opt_kat(ctx, golden):
    n, T, outl, st = ctx.pose_opt(K, golden["pose_Tinit"], golden["pose_obs"])
    assert n == int(golden["pose_n"])
    assert np.array_equal(outl, golden["pose_outlier"])
    _pose_close(T, golden["pose_T"])
    assert np.isclose(st[1], golden["pose_stats"][1], rtol=1e-6)  # final robust chi2 (reprojection error)
    # the LM iteration count is NOT compared: at convergence the accept/reject sign of rho is rounding
    # noise (tree vs sequential summation), which changes how many no-op iterations run, not the pose


@pytest.mark.parametrize("seed,n,frac", [(1, 300, 0.15), (2, 2000, 0.05), (3, 50, 0.3), (4, 9, 0.0), (5, 3, 0.0), (6, 700, 0.5)])
def test_pose_opt_vs_oracle(ctx, seed, n, frac):
    Tt, Ti, obs = synth.pose_problem(seed, n, K, noise_px=0.4, outlier_frac=frac)
    no, To, oo, so = oracle.pose_opt(K, Ti, obs)
    ng, Tg, og, sg = ctx.pose_opt(K, Ti, obs)
    assert ng == no and np.array_equal(og, oo)
    _pose_close(Tg, To)
    assert np.isclose(sg[1], so[1], rtol=1e-6, atol=1e-9)
    # pre-set outlier flags are an input (Frame::GetOutlier)
    pre = (np.arange(n) % 7 == 0).astype(np.uint8)
    no, To, oo, _ = oracle.pose_opt(K, Ti, obs, pre)
    ng, Tg, og, _ = ctx.pose_opt(K, Ti, obs, pre)
    assert ng == no and np.array_equal(og, oo)
    _pose_close(Tg, To)


def test_pose_opt_too_few(ctx):
    Tt, Ti, obs = synth.pose_problem(9, 2, K)
    n, T, outl, st = ctx.pose_opt(K, Ti, obs)
    assert n == 0 and np.array_equal(T, Ti)
    n, T, outl, st = ctx.pose_opt(K, Ti, obs[:0])
    assert n == 0 and np.array_equal(T, Ti)


def _bow_case(seed, n1=1500, n2=1400, nnodes=180, overlap=0.75):
    """Two frames with descriptors, angles and DBoW2-style feature vectors (node id -> feature indices): a share of F2's
    features are noisy copies of F1 features filed under the same node, some nodes exist in one frame only."""
    rng = np.random.default_rng(seed)
    k1 = np.zeros(n1, capi.KEYPOINT); k2 = np.zeros(n2, capi.KEYPOINT)
    k1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    node1 = rng.integers(0, nnodes, n1) * 7 + 3
    src = rng.integers(0, n1, n2)
    same = rng.uniform(size=n2) < overlap
    node2 = np.where(same, node1[src], rng.integers(0, nnodes + 40, n2) * 7 + 3)
    for i in np.nonzero(same)[0]:
        d2[i] = d1[src[i]]
        flips = rng.integers(0, 256, rng.integers(0, 40))
        for b in flips:
            d2[i, b >> 3] ^= np.uint8(1 << (b & 7))
    rot = np.where(rng.uniform(size=n2) < 0.7, 20.0, rng.uniform(0, 360, n2))
    k2["angle"] = ((k1["angle"][src] - rot + rng.uniform(-4, 4, n2)) % 360).astype(np.float32)
    fv1, fv2 = {}, {}
    for i in rng.permutation(n1):
        fv1.setdefault(int(node1[i]), []).append(int(i))
    for i in rng.permutation(n2):
        fv2.setdefault(int(node2[i]), []).append(int(i))
    has_mp2 = (rng.uniform(size=n2) < 0.6).astype(np.uint8)
    return k1, d1, fv1, k2, d2, fv2, has_mp2


@pytest.mark.parametrize("seed,kw", [(1, dict(th_low=50, nratio=0.9, histo_len=30, check_orientation=True)),
                                     (2, dict(th_low=80, nratio=0.7, histo_len=30, check_orientation=False)),
                                     (3, dict(th_low=100, nratio=1.0, histo_len=45, check_orientation=True, map_point_only=True)),
                                     (4, dict(th_low=257, nratio=2.0, histo_len=30, check_orientation=True))])
def test_search_by_bow_vs_oracle(ctx, seed, kw):
    """Matcher::searchByBow (matcher.cpp:619-721) with the frames' feature vectors as inputs."""
    k1, d1, fv1, k2, d2, fv2, has_mp2 = _bow_case(seed)
    exp = oracle.search_by_bow(k1, d1, fv1, k2, d2, fv2, has_mp2=has_mp2, **kw)
    got = ctx.search_by_bow(k1, d1, fv1, k2, d2, fv2, has_mp2=has_mp2, **kw)
    _eq_struct(got, exp)
    assert len(exp) > 100


def test_search_by_bow_edges(ctx):
    k1, d1, fv1, k2, d2, fv2, has_mp2 = _bow_case(5, n1=200, n2=150, nnodes=20)
    kw = dict(th_low=60, nratio=0.9, histo_len=30, check_orientation=True)
    assert len(ctx.search_by_bow(k1, d1, {}, k2, d2, fv2, **kw)) == 0          # an empty feature vector
    assert len(ctx.search_by_bow(k1, d1, fv1, k2, d2, {}, **kw)) == 0
    disjoint = {k + 100000: v for k, v in fv2.items()}                          # no shared node
    assert len(ctx.search_by_bow(k1, d1, fv1, k2, d2, disjoint, **kw)) == 0
    none = np.zeros(len(k2), np.uint8)                                          # MapPointOnly without any map point
    assert len(ctx.search_by_bow(k1, d1, fv1, k2, d2, fv2, has_mp2=none, map_point_only=True, **kw)) == 0
    with pytest.raises(capi.TBError):                                           # a feature index outside the frame
        bad = dict(fv1); bad[next(iter(bad))] = [10 ** 6]
        ctx.search_by_bow(k1, d1, bad, k2, d2, fv2, **kw)



def _raw_bow(ctx, k1, d1, csr1, k2, d2, csr2, cap, has_mp2=None, map_point_only=False, th_low=80, nratio=0.95, histo_len=30):
    """tb_search_by_bow through the raw C ABI on CSR feature vectors (nodes, start, items): (return code, *count, out[:cap])."""
    k1 = np.ascontiguousarray(k1, capi.KEYPOINT); k2 = np.ascontiguousarray(k2, capi.KEYPOINT)
    d1, d2 = np.ascontiguousarray(d1, np.uint8), np.ascontiguousarray(d2, np.uint8)
    (n1, s1, i1), (n2, s2, i2) = csr1, csr2
    out = np.zeros(max(cap, 1), capi.MATCH); n = C.c_int(-7)
    rc = capi.lib().tb_search_by_bow(ctx._h, _ptr(k1), _ptr(d1), len(k1), _ptr(n1), _ptr(s1), _ptr(i1), len(n1), _ptr(k2), _ptr(d2),
                                     len(k2), _ptr(has_mp2), _ptr(n2), _ptr(s2), _ptr(i2), len(n2), int(map_point_only), th_low,
                                     C.c_float(nratio), histo_len, 1, _ptr(out), cap, C.byref(n))
    return rc, n.value, out[:cap]


def test_search_by_bow_capacity_and_bounds(ctx):
    """cap = count - 1 -> TB_ECAPACITY with the full count, cap = count -> the oracle's list; node ids out of order and
    histo_len above 1024 are rejected."""
    k1, d1, fv1, k2, d2, fv2, has_mp2 = _bow_case(6)
    csr1, csr2 = capi.Context._fv(fv1), capi.Context._fv(fv2)
    exp = oracle.search_by_bow(k1, d1, fv1, k2, d2, fv2, has_mp2=has_mp2, map_point_only=True, th_low=80, nratio=0.95, histo_len=30)
    assert len(exp) > 1
    rc, n, _ = _raw_bow(ctx, k1, d1, csr1, k2, d2, csr2, len(exp) - 1, has_mp2, True)
    assert rc == capi.TB_ECAPACITY and n == len(exp)
    rc, n, out = _raw_bow(ctx, k1, d1, csr1, k2, d2, csr2, len(exp), has_mp2, True)
    assert rc == capi.TB_OK and n == len(exp)
    _eq_struct(out, exp)
    for side in (0, 1):
        nodes = [csr1[0].copy(), csr2[0].copy()]
        nodes[side][[0, 1]] = nodes[side][[1, 0]]                                   # two node ids swapped
        bad = [(nodes[0],) + csr1[1:], (nodes[1],) + csr2[1:]]
        assert _raw_bow(ctx, k1, d1, bad[0], k2, d2, bad[1], len(exp))[0] == capi.TB_EINVAL
    assert _raw_bow(ctx, k1, d1, csr1, k2, d2, csr2, len(exp), histo_len=1025)[0] == capi.TB_EINVAL

def test_pose_from_stereo_tracks_finds_the_baseline(ctx):
    """tb_stereo_tracks_to_obs_batch_dev + PoseOptimization from the identity, the composition bench.py times: keys of a left
    frame with known depths, their right-frame images one baseline along x (plus pixel noise and a few gross mismatches), a
    match per key -> observation rows == oracle bit for bit, ragged counts, dropped zero-disparity rows, and the pose found
    from them is the right camera's (t = -baseline along x)."""
    import torch
    from trackingbench_slam_amd.pipeline import KITTI_BF, KITTI_K
    dev = torch.device("cuda", 0)
    fx, fy, cx, cy = KITTI_K
    F, cap = 3, 700
    isig2 = oracle.scale_factors(8, 0.8)[3]
    rng = np.random.default_rng(17)
    KL = np.zeros((F, cap), capi.KEYPOINT); KR = np.zeros((F, cap), capi.KEYPOINT)
    M = np.zeros((F, cap), capi.MATCH); MC = np.zeros(F, np.int32)
    for f, n in enumerate((600, 257, 2)):
        depth = rng.uniform(6.0, 60.0, n).astype(np.float32)
        KL[f, :n]["x"] = rng.uniform(100, 1100, n); KL[f, :n]["y"] = rng.uniform(40, 340, n)
        KL[f, :n]["octave"] = rng.integers(0, 8, n)
        KR[f, :n] = KL[f, :n]
        KR[f, :n]["x"] = KL[f, :n]["x"] - np.float32(KITTI_BF) / depth + rng.normal(0, 0.3, n).astype(np.float32)
        KR[f, :n]["y"] = KL[f, :n]["y"] + rng.normal(0, 0.3, n).astype(np.float32)
        bad = rng.permutation(n)[:n // 12]
        KR["y"][f, bad] += 40.0                                   # gross mismatches: pose-opt must flag them
        perm = rng.permutation(n)                                 # matches in an order of their own, right keys shuffled
        inv = np.argsort(perm)
        KR[f, :n] = KR[f, :n][perm]
        M[f, :n]["queryIdx"] = np.arange(n); M[f, :n]["trainIdx"] = inv; M[f, :n]["imgIdx"] = -1
        if n > 10:
            KR[f, inv[5]]["x"] = KL[f, 5]["x"]                    # no disparity: the row is dropped
        MC[f] = n
    t = lambda a, dt: torch.from_numpy(a.view(dt).reshape(F, cap, -1)).to(dev)
    dKL, dKR, dM = t(KL, np.float32), t(KR, np.float32), t(M, np.int32)
    dMC = torch.from_numpy(MC).to(dev)
    obs = torch.zeros((F, cap, 6), dtype=torch.float32, device=dev)
    oc = torch.zeros(F, dtype=torch.int32, device=dev)
    Kf = np.ascontiguousarray(KITTI_K, np.float32)
    L = capi.lib()
    ctx.check(L.tb_stereo_tracks_to_obs_batch_dev(ctx._h, F, C.c_void_p(dKL.data_ptr()), C.c_void_p(dKR.data_ptr()), cap,
                                                  C.c_void_p(dM.data_ptr()), C.c_void_p(dMC.data_ptr()), cap,
                                                  Kf.ctypes.data_as(C.c_void_p), C.c_float(KITTI_BF), isig2.ctypes.data_as(C.c_void_p), 8,
                                                  C.c_void_p(obs.data_ptr()), cap, C.c_void_p(oc.data_ptr())))
    ctx.synchronize()
    for f in range(F):
        n = int(MC[f])
        exp = oracle.stereo_tracks_to_obs(KL[f], KR[f], M[f, :n], KITTI_K, KITTI_BF, isig2)
        assert int(oc[f].item()) == len(exp) == (n - 1 if n > 10 else n)
        got = obs[f, :len(exp)].cpu().numpy().reshape(-1).view(capi.OBS)
        assert np.array_equal(got, exp)
        ninl, T, outl, _ = ctx.pose_opt(KITTI_K, np.eye(4, dtype=np.float32), got)
        no, To, oo, _ = oracle.pose_opt(KITTI_K, np.eye(4, dtype=np.float32), exp)
        assert ninl == no and np.array_equal(outl, oo) and np.allclose(T, To, rtol=1e-6, atol=1e-6)
        if n > 10:
            assert abs(T[0, 3] + KITTI_BF / fx) < 0.02 and np.abs(T[:3, :3] - np.eye(3)).max() < 5e-3
            assert n // 12 <= outl.sum() < n // 6


def test_stereo_tracks_ordered_compaction_edges(ctx):
    """tb_stereo_tracks_to_obs_batch_dev's ordered compaction at wave (64) and workgroup (256) boundaries: one batch whose frames
    hold 0 .. 600 matches, every third of them without disparity (dropped); each frame == the oracle, rows in match order."""
    import torch
    from trackingbench_slam_amd.pipeline import KITTI_BF, KITTI_K
    dev = torch.device("cuda", 0)
    counts = (0, 1, 63, 64, 65, 255, 256, 257, 600)
    F, cap = len(counts), 600
    isig2 = oracle.scale_factors(8, 0.8)[3]
    rng = np.random.default_rng(23)
    KL = np.zeros((F, cap), capi.KEYPOINT); KR = np.zeros((F, cap), capi.KEYPOINT)
    M = np.zeros((F, cap), capi.MATCH); MC = np.array(counts, np.int32)
    for f, n in enumerate(counts):
        KL[f, :n]["x"] = rng.uniform(100, 1100, n); KL[f, :n]["y"] = rng.uniform(40, 340, n)
        KL[f, :n]["octave"] = rng.integers(0, 8, n)
        perm = rng.permutation(n)                                 # match i: left key i <-> right key perm[i]
        KR[f, perm] = KL[f, :n]
        disp = rng.uniform(5.0, 60.0, n).astype(np.float32)
        disp[np.arange(n) % 3 == 0] = 0.0                         # every third match: no disparity
        KR["x"][f, perm] = KL["x"][f, :n] - disp
        M[f, :n]["queryIdx"] = np.arange(n); M[f, :n]["trainIdx"] = perm; M[f, :n]["imgIdx"] = -1
    t = lambda a, dt: torch.from_numpy(a.view(dt).reshape(F, cap, -1)).to(dev)
    dKL, dKR, dM = t(KL, np.float32), t(KR, np.float32), t(M, np.int32)
    dMC = torch.from_numpy(MC).to(dev)
    obs = torch.full((F, cap, 6), -1.0, dtype=torch.float32, device=dev)
    oc = torch.full((F,), -1, dtype=torch.int32, device=dev)
    Kf = np.ascontiguousarray(KITTI_K, np.float32)
    ctx.check(capi.lib().tb_stereo_tracks_to_obs_batch_dev(ctx._h, F, C.c_void_p(dKL.data_ptr()), C.c_void_p(dKR.data_ptr()), cap,
                                                           C.c_void_p(dM.data_ptr()), C.c_void_p(dMC.data_ptr()), cap,
                                                           Kf.ctypes.data_as(C.c_void_p), C.c_float(KITTI_BF),
                                                           isig2.ctypes.data_as(C.c_void_p), 8, C.c_void_p(obs.data_ptr()), cap,
                                                           C.c_void_p(oc.data_ptr())))
    ctx.synchronize()
    got_all, got_n = obs.cpu().numpy(), oc.cpu().numpy()
    for f, n in enumerate(counts):
        exp = oracle.stereo_tracks_to_obs(KL[f], KR[f], M[f, :n], KITTI_K, KITTI_BF, isig2)
        assert int(got_n[f]) == len(exp) == n - (n + 2) // 3
        assert np.array_equal(got_all[f, :len(exp)].reshape(-1).view(capi.OBS), exp)
        assert (got_all[f, len(exp):] == -1.0).all()              # nothing written past the list
