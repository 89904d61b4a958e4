"""GPU tests (pytest -m gpu) of the keyframe store's Sim(3) query (tb_kf_store_sim3_dev, include/tb_capi.h) against
tests/reloc_sim3_reference.py, on a store filled as tests/test_gpu_kf_store_pnp.py fills its own: 200 keys, pitch 256, S = 2
sequences, capacity 2, slot 0 a keyframe 70 % of whose stored map points are displaced by metres, slot 1 one with five map
points. The query frame carries a map of its own: the true scene points moved by a known similarity D (s = 1.1, 0.1 rad, 1 m) --
a drifted map -- for nine keys in ten. X1 = Tq D X and X2 = Tst X, so the transform sought is S12 = Tq D Tst^-1.

Rows, row counts, per-candidate outputs and the selection are exact (the RANSAC's inputs are the same bits).

The recovered transform against S12: the noise-free bounds of tests/test_sim3_reference.py (1e-6 relative in scale, 1e-6 rad, 1e-5 m)
loosened by what the float32 storage costs. The coordinates lie below 64 m, where half a float32 ulp is 1.9e-6 m. A row's X1 is
rounded twice (the query's world point, then the camera point), its X2 once more than the stored point, which is exact: each side
is off by at most sqrt(3) * 2 * 1.9e-6 = 6.6e-6 m, the two sides together by d = 1.3e-5 m in the worst case of aligned errors.
The consensus rows spread r = 7 m (RMS) about a centroid c = 19 m from the cameras. A least-squares similarity then moves by at
most d / r = 1.9e-6 in scale and in rotation (rad), and by d + c d / r = 4.9e-5 m in translation. The float32 poses Tq and Tst are
orthonormal to 6e-8 only, which the fit sees as 6e-8 of scale and rotation and 6e-8 * c = 1.1e-6 m. With the noise-free bounds
that is 3e-6, 3e-6 rad and 6e-5 m, rounded up to 7e-5 m."""
import numpy as np
import pytest
import torch

import pnp_cases as pc
import reloc_reference as rr
import reloc_sim3_reference as rs
import sim3_cases as sc
import sim3_reference as sr
import test_gpu_kf_store_pnp as kp
from test_gpu_kf_store import K, NLEVELS, SCALE, TR, _pack_frames, _view, voc  # noqa: F401 (fixtures)
from test_gpu_vo_desc import _same_bits
from trackingbench_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

S, CAP, PITCH, N = kp.S, kp.CAP, kp.PITCH, kp.N
CANDS = kp.CANDS                      # [[0, -1], [1, 0]]
PRM = dict(hypotheses=256, fixed_scale=False, chi2_max=sr.CHI2_MAX, seed=3)
MIN_CONS = 20
BOUNDS = (3e-6, 3e-6, 7e-5)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def drift():
    """D: X -> s R X + t in world coordinates"""
    return 1.1, sc.rodrigues((0.3, 1.0, -0.2), 0.1), np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74])


def build_case(voc):
    """test_gpu_kf_store_pnp.build_case's construction with the query's point ids kept: adds[a][s] = (keyframe, Tcw, kf_id),
    queries[s] = (kps, desc, bow), q_mp [s] float32 [N][3] = D applied to the true points, q_valid[s], q_Tcw[s], truth[s] = (s, R, t)
    of S12 = Tq D Tst^-1"""
    rng = np.random.default_rng(77)
    sD, RD, tD = drift()
    adds = [[None] * S for _ in range(CAP)]
    out = dict(adds=adds, queries=[], q_mp=[], q_valid=[], q_Tcw=[], truth=[])
    for s in range(S):
        scene = (np.stack([rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(8, 30, N)], -1).astype(np.float32),
                 synth.descriptors_near_words(500 + s, voc, N, flips=12), rng.uniform(0, 360, N), rng.integers(0, NLEVELS, N))
        Tst = pc.pose(0.1 * (s + 1), -0.05, (0.4, -0.2, 0.5)).astype(np.float32)
        Tq = pc.moved(Tst.astype(np.float64), 0.2, 3.0)
        kps, desc, bow, ids = _view(rng, voc, scene, Tq, N, 2, 0.5)
        out["queries"].append((kps, desc, bow))
        out["q_mp"].append((sD * scene[0][ids].astype(np.float64) @ RD.T + tD).astype(np.float32))
        out["q_Tcw"].append(Tq.astype(np.float32))
        for a in range(CAP):
            kkps, kdesc, kbow, kids = _view(rng, voc, scene, Tst, N, 2, 0.5)
            mp = scene[0][kids].copy()
            valid = np.ones(N, bool)
            if a == 0:
                bad = rng.permutation(N)[:int(0.7 * N)]
                mp[bad] += (rng.uniform(2, 5, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))).astype(np.float32)
            else:
                valid[:] = False
                valid[rng.permutation(N)[:5]] = True
            adds[a][s] = (dict(orb=kkps, desc=kdesc, mp=mp.astype(np.float32), valid=valid, frame=10 * a, bow=kbow), Tst, 10 * a)
        # X1 = Rq (s RD X + tD) + tq and X = Rst' (X2 - tst)
        Rq, tq = Tq[:3, :3].astype(np.float64), Tq[:3, 3].astype(np.float64)
        Rs, ts = Tst[:3, :3].astype(np.float64), Tst[:3, 3].astype(np.float64)
        R12 = Rq @ RD @ Rs.T
        out["truth"].append((sD, R12, Rq @ tD + tq - sD * R12 @ ts))
    vrng = np.random.default_rng(78)
    out["q_valid"] = [vrng.uniform(0, 1, N) < 0.9 for _ in range(S)]
    return out


@pytest.fixture(scope="module")
def case():
    return build_case(synth.vocabulary(1, 10, 5))


def _query_map(case):
    rng = np.random.default_rng(56)
    mp = rng.uniform(-5, 5, (S, PITCH, 3)).astype(np.float32)
    valid = rng.integers(0, 2, (S, PITCH)).astype(np.uint8)        # what lies beyond the counts is garbage
    for s in range(S):
        mp[s, :N] = case["q_mp"][s]
        valid[s, :N] = case["q_valid"][s]
    return torch.from_numpy(mp).cuda(), torch.from_numpy(valid).cuda(), torch.from_numpy(np.stack(case["q_Tcw"])).cuda()


def _snapshot(ctx, st, reloc):
    ctx.synchronize()
    snap = {"state_" + k: (v.cpu().numpy().tobytes() if hasattr(v, "cpu") else v) for k, v in st.state("cuda").items()}
    snap.update({"work_" + k: v.cpu().numpy().tobytes() for k, v in st.work("cuda", 2).items()})
    snap.update({"out_" + k: v.cpu().numpy().tobytes() for k, v in reloc.items()})
    return snap


@pytest.fixture(scope="module")
def ran(ctx, case):
    """relocalize, then sim3: the GPU's outputs, the snapshots around the query, and the composition's"""
    st, rings = kp._fill(ctx, case)
    try:
        q = _pack_frames(case["queries"], PITCH, 55)
        cands = torch.from_numpy(CANDS).cuda()
        mp, valid, Tq = _query_map(case)
        rc_early, _ = st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, min_consensus=MIN_CONS, **PRM)
        with pytest.raises(capi.TBError) as early_state:
            st.sim3_state("cuda", 2)
        reloc = st.relocalize(K, NLEVELS, SCALE, *q, cands, map_point_only=TR.map_point_only, th_low=TR.th_low, nratio=TR.nratio,
                              histo_len=TR.histo_len, check_orientation=TR.check_orientation, min_inliers=kp.MIN_INL)
        before = _snapshot(ctx, st, reloc)
        def go(min_consensus=MIN_CONS, **kw):
            o = st.sim3(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, min_consensus=min_consensus, **dict(PRM, **kw))
            ctx.synchronize()               # the query runs on the context's stream
            return {k: v.cpu().numpy() for k, v in o.items()}

        g = go()
        after = _snapshot(ctx, st, reloc)
        g.update({k: v.cpu().numpy() for k, v in st.sim3_state("cuda", 2).items()})
        again = go()                        # a second query: the same bytes
        fixed = go(fixed_scale=True)
        high = go(min_consensus=100000)
        errs = [st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, **dict(PRM, **bad))[0] for bad in
                (dict(hypotheses=0), dict(hypotheses=1025), dict(fixed_scale=2), dict(chi2_max=float("nan")), dict(chi2_max=-1.0))]
        errs += [st.sim3_rc(K, 0, SCALE, q[0], q[2], mp, valid, Tq, cands, **PRM)[0], st.sim3_rc(K, 17, SCALE, q[0], q[2], mp, valid, Tq, cands, **PRM)[0],
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, ncand=3, **PRM)[0],
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, ncand=0, **PRM)[0],
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, ncand=1, **PRM)[0],      # not the verification's ncand
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, q_pitch=PITCH + 1, **PRM)[0],
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, q_pitch=0, **PRM)[0],
                 st.sim3_rc(K, NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, min_consensus=-1, **PRM)[0],
                 st.sim3_rc((0.0, 360.0, 320.0, 120.0), NLEVELS, SCALE, q[0], q[2], mp, valid, Tq, cands, **PRM)[0]]
        ctx.synchronize()
    finally:
        st.close()
    exp = [rs.sim3(*case["queries"][s], case["q_mp"][s], case["q_valid"][s], case["q_Tcw"][s], rings[s], CANDS[s], TR, K, NLEVELS, SCALE,
                   MIN_CONS, **PRM) for s in range(S)]
    return dict(g=g, again=again, fixed=fixed, high=high, before=before, after=after, exp=exp, rc_early=rc_early,
                early_state=early_state.value.code, errs=errs)


def test_rows_candidates_and_selection_equal_the_composition(ran):
    g, exp = ran["g"], ran["exp"]
    for s, e in enumerate(exp):
        for r, c in enumerate(e["cands"]):
            p, w, n = 2 * s + r, (s, r), len(c["rows"])
            assert c["margin"] > 1e-9, w
            assert g["cand_rows"][s, r] == n == g["row_counts"][p], w
            assert _same_bits(g["rows"][p, :n], c["rows"].view(np.float32).reshape(-1, 8)), w
            assert g["cand_consensus"][s, r] == c["consensus"] and g["cand_flags"][s, r] == c["flags"], w
            assert np.array_equal(g["cand_S12"][s, r].view(np.uint32), c["S12"].view(np.uint32)), w
            assert np.array_equal(g["cand_srt"][s, r].view(np.uint64), c["srt"].view(np.uint64)), w
            assert np.array_equal(g["inlier"][p, :n], c["inlier"]) and not g["inlier"][p, n:].any(), w
        assert g["best_rank"][s] == e["best_rank"] and g["best_kf"][s] == e["best_kf"], s
        assert np.array_equal(g["best_S12"][s].view(np.uint32), e["best_S12"].view(np.uint32)), s
        assert np.array_equal(g["best_srt"][s].view(np.uint64), e["best_srt"].view(np.uint64)), s
    # what the case is there for: the drifted map is tied to the far keyframe's good rows (at most 60, nine in ten with a point)
    assert g["best_rank"].tolist() == [0, 1] and g["best_kf"].tolist() == [0, 0]
    for c in (exp[0]["cands"][0], exp[1]["cands"][1]):
        assert len(c["rows"]) >= 120 and 35 <= c["consensus"] <= 60 and c["winner"][1] == 1
    few = exp[1]["cands"][0]
    assert len(few["rows"]) <= 5 and few["consensus"] < MIN_CONS       # the keyframe with five map points


def test_an_absent_candidate_has_no_rows_and_never_wins(ran):
    g, exp = ran["g"], ran["exp"]
    assert exp[0]["cands"][1]["kf"] == -1
    assert g["cand_rows"][0, 1] == 0 and g["row_counts"][1] == 0 and g["cand_consensus"][0, 1] == 0 and g["cand_flags"][0, 1] == 1
    assert np.array_equal(g["cand_S12"][0, 1], np.eye(4, dtype=np.float32)) and np.array_equal(g["cand_srt"][0, 1], rs.SRT_EYE)
    h = ran["high"]      # a consensus nobody reaches: no answer, the identity and scale 1
    assert h["best_rank"].tolist() == [-1, -1] and h["best_kf"].tolist() == [-1, -1]
    assert all(np.array_equal(h["best_S12"][s], np.eye(4, dtype=np.float32)) and np.array_equal(h["best_srt"][s], rs.SRT_EYE) for s in range(S))


def test_the_recovered_transform_is_the_drift(ran, case):
    g = ran["g"]
    for s in range(S):
        es, er, et = sc.errors(dict(srt=g["best_srt"][s]), case["truth"][s])
        print("sequence %d: scale %.2e  rotation %.2e rad  translation %.2e m" % (s, es, er, et))
        assert es < BOUNDS[0] and er < BOUNDS[1] and et < BOUNDS[2]
    # with the scale fixed at 1 the transform of a map that is 10 % too large finds little
    f = ran["fixed"]
    assert (f["cand_srt"][..., 7] == 1.0).all() and (f["cand_consensus"] < ran["g"]["cand_consensus"].max()).all()


def test_the_query_changes_nothing_else_and_repeats(ran):
    assert ran["before"].keys() == ran["after"].keys()
    for k in ran["before"]:
        assert ran["before"][k] == ran["after"][k], k
    for k, v in ran["again"].items():
        assert v.tobytes() == ran["g"][k].tobytes(), k


def test_state_and_argument_errors(ran):
    assert ran["rc_early"] == capi.TB_ESTATE and ran["early_state"] == capi.TB_ESTATE
    assert ran["errs"] == [capi.TB_EINVAL] * len(ran["errs"])
