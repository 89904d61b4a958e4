"""tb_pose_graph_sim3 / tb_pose_graph_sim3_batch_dev (k_pgo_sim3.hip) against tests/pose_graph_sim3_reference.py, the numpy float64 solver.

Bounds: nodes and chi2 within 1e-6 relative (the project's bar for k_pgo and the BA), iteration and trial counts and the malformed
flag exact, skipped and flagged graphs byte-identical to their input. The counts can be exact because every case stops, by its
`iters`, before LM reaches the rounding floor of chi2; every trial of the reference's trace is asserted to change chi2 by more than
1e-9 of itself.

Sizes sit on each side of the kernel's internal boundaries, N = D (nnodes - nfixed) unknowns, D = 7 with the scale free, 6 held:
  PG3_PANEL = 7 columns per panel     nnodes 2: N = 7 one full panel (6: a part); nnodes 3: N = 14 two panels (12: one and a part)
  PG3_TILE = 16 trailing-update tile  nnodes 3: below one tile; nnodes 4: N = 21 (18), a tile and a part
  PG3_T = 256 threads, one per row    N + 1 = 253 and 260 rows (nnodes 37, 38 free; 253 and 259 at nnodes 43, 44 held)
and at the caps: 64 nodes, edge_pitch 256 with 250 edges."""
import functools

import numpy as np
import pytest
import torch

import pose_graph_sim3_reference as s3
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dense_chords(n, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) > 1:
            out.append((a, b))
    return out


# name -> (chain_graph arguments, nfixed, iters, fixed_scale)
CASES = {
    "n2": (dict(seed=1, nnodes=2, chords=[]), 1, 2, False),
    "n2_held": (dict(seed=1, nnodes=2, chords=[]), 1, 2, True),
    "n3_chord": (dict(seed=2, nnodes=3, chords=[(0, 2)]), 1, 3, False),
    "n3_chord_held": (dict(seed=2, nnodes=3, chords=[(0, 2)]), 1, 3, True),
    "n4_chord": (dict(seed=2, nnodes=4, chords=[(0, 3)]), 1, 3, False),
    "n4_chord_held": (dict(seed=2, nnodes=4, chords=[(0, 3)]), 1, 3, True),
    "n7_fan_repeat_reversed": (dict(seed=3, nnodes=7, chords=[(0, 6), (2, 6), (2, 6), (5, 1)], reverse=(1, 7)), 1, 3, False),
    "n7_fan_repeat_reversed_held": (dict(seed=3, nnodes=7, chords=[(0, 6), (2, 6), (2, 6), (5, 1)], reverse=(1, 7)), 1, 3, True),
    "n7_nfixed2_weights": (dict(seed=3, nnodes=7, chords=[(0, 6), (2, 6)], w=(4.0, 0.5, 2.0)), 2, 3, False),
    "n7_nfixed2_weights_held": (dict(seed=3, nnodes=7, chords=[(0, 6), (2, 6)], w=(4.0, 0.5, 2.0)), 2, 3, True),
    "n6_far_scales": (dict(seed=4, nnodes=6, chords=[(0, 5), (1, 4)], step_scale={2: 0.5, 4: 2.0, 5: 2.0}), 1, 3, False),
    "n6_far_scales_held": (dict(seed=4, nnodes=6, chords=[(0, 5), (1, 4)], step_scale={2: 0.5, 4: 2.0, 5: 2.0}), 1, 3, True),
    "n37": (dict(seed=5, nnodes=37, chords=[(0, 36), (7, 30)]), 1, 3, False),            # 253 rows
    "n38": (dict(seed=5, nnodes=38, chords=[(0, 37), (7, 30)]), 1, 3, False),            # 260 rows
    "n43_held": (dict(seed=5, nnodes=43, chords=[(0, 42), (7, 30)]), 1, 3, True),        # 253 rows
    "n44_held": (dict(seed=5, nnodes=44, chords=[(0, 43), (7, 30)]), 1, 3, True),        # 259 rows
    "n64_pitch_full": (dict(seed=9, nnodes=64, chords=_dense_chords(64, 250 - 63, 4)), 1, 3, False),
    "iters0": (dict(seed=3, nnodes=7, chords=[(0, 6)]), 1, 0, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(nodes0, edges, nfixed, iters, fixed_scale, reference nodes, reference stats), computed once"""
    if name.startswith("rejecting"):
        nodes0, edges, nfixed, iters = s3.rejecting_case()
        fixed_scale = name.endswith("_held")
    else:
        args, nfixed, iters, fixed_scale = CASES[name]
        nodes0, edges = s3.chain_graph(**args)
    trace = []
    ref, st = s3.solve(nodes0, nfixed, edges, iters, fixed_scale, trace=trace)
    assert all(abs(t[4] - t[5]) > 1e-9 * t[4] for t in trace), "a trial of this case is decided by rounding"
    for a in (nodes0, edges, ref, st):
        a.setflags(write=False)
    return nodes0, edges, nfixed, iters, fixed_scale, ref, st


def _close(got, ref, st, rst):
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(ref).max()))), float(np.abs(got - ref).max())
    assert st[0] == rst[0] and st[4] == rst[4] and st[7] == rst[7] == 0, (st, rst)
    assert np.isclose(st[1], rst[1], rtol=1e-6, atol=1e-12) and np.isclose(st[2], rst[2], rtol=1e-6, atol=1e-12), (st, rst)
    assert np.isclose(st[3], rst[3], rtol=1e-6), (st, rst)


def _batch(ctx, nodes, nfixed, edges, counts, iters, fixed_scale):
    """tb_pose_graph_sim3_batch_dev on host arrays [G, n, 8], [G, pitch], [G] -> (nodes, stats)"""
    G, n = nodes.shape[:2]
    dn = torch.from_numpy(np.array(nodes, np.float64)).cuda()      # a copy: the cases' arrays are read-only
    de = torch.from_numpy(np.ascontiguousarray(edges).view(np.uint8).reshape(G, -1)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    ds = torch.full((G, 8), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.pose_graph_sim3_dev(G, n, nfixed, dn.data_ptr(), de.data_ptr(), dc.data_ptr(), edges.shape[1], iters, ds.data_ptr(),
                                      fixed_scale=fixed_scale))
    ctx.synchronize()
    return dn.cpu().numpy(), ds.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES) + ["rejecting"])
def test_single_graph_matches_the_reference(ctx, name):
    nodes0, edges, nfixed, iters, fixed_scale, ref, rst = _case(name)
    if name.startswith("rejecting"):
        assert rst[4] > rst[0]
    if name.startswith("n6_far_scales"):
        assert 0.4 < nodes0[2, 7] < 0.6 and np.any(edges["srt"][:, 7] > 1.7) and np.any(edges["srt"][:, 7] < 0.6)
    if name == "n64_pitch_full":     # the host form would run it at pitch 250: a 256-wide edge array, 250 counted, through the device form
        assert len(edges) == 250
        wide = np.zeros((1, 256), s3.EDGE)
        wide[0, :len(edges)] = edges
        gotb, stb = _batch(ctx, nodes0[None], nfixed, wide, [len(edges)], iters, fixed_scale)
        got, st = gotb[0], stb[0]
    else:
        got, st = ctx.pose_graph_sim3(nodes0, nfixed, edges, iters, fixed_scale)
        # the host form equals the device form, bit for bit
        gotb, stb = _batch(ctx, nodes0[None], nfixed, edges[None], [len(edges)], iters, fixed_scale)
        assert gotb[0].tobytes() == got.tobytes() and stb[0].tobytes() == st.tobytes()
    _close(got, ref, st, rst)
    assert got[:nfixed].tobytes() == nodes0[:nfixed].tobytes()
    if fixed_scale:
        assert got[:, 7].tobytes() == nodes0[:, 7].tobytes()
    elif iters:
        assert not np.array_equal(got[nfixed:, 7], nodes0[nfixed:, 7])
    if iters == 0:
        assert got.tobytes() == nodes0.tobytes() and st[1] == st[2] > 0


def _mixed_batch():
    """five graphs of 7 nodes at pitch 12: a good one, one with no edge, the first again, a malformed one, another good one"""
    n0, e0 = _case("n7_fan_repeat_reversed")[:2]
    n1, e1 = s3.chain_graph(seed=13, nnodes=7, chords=[(1, 5), (0, 6)])
    pitch = 12
    nodes = np.stack([n0, n1, n0, n1, n1])
    edges = np.zeros((5, pitch), s3.EDGE)
    counts = np.array([len(e0), 0, len(e0), len(e1), len(e1)], np.int32)
    edges[0, :len(e0)] = e0
    edges[1, :len(e1)] = e1          # present but not counted
    edges[2, :len(e0)] = e0
    edges[3, :len(e1)] = e1
    edges[3, 4]["b"] = 7             # out of range
    edges[4, :len(e1)] = e1
    return nodes, edges, counts


@pytest.mark.parametrize("fixed_scale", [False, True])
def test_batch_with_an_empty_and_a_malformed_graph_and_bitwise_repeatability(ctx, fixed_scale):
    nodes, edges, counts = _mixed_batch()
    ref, rst = s3.solve_batch(nodes, 1, edges, counts, 3, fixed_scale)
    got, st = _batch(ctx, nodes, 1, edges, counts, 3, fixed_scale)
    for g in (0, 2, 4):
        _close(got[g], ref[g], st[g], rst[g])
    assert got[1].tobytes() == nodes[1].tobytes() and not st[1].any()
    assert got[3].tobytes() == nodes[3].tobytes() and st[3, 7] == -1 and not st[3, :7].any()
    assert got[0].tobytes() == got[2].tobytes() and st[0].tobytes() == st[2].tobytes()
    # the same call twice, and graph 0 alone (another pitch offset, another scratch slice): bit for bit
    got2, st2 = _batch(ctx, nodes, 1, edges, counts, 3, fixed_scale)
    assert got2.tobytes() == got.tobytes() and st2.tobytes() == st.tobytes()
    alone, sta = _batch(ctx, nodes[:1], 1, edges[:1], counts[:1], 3, fixed_scale)
    assert alone[0].tobytes() == got[0].tobytes() and sta[0].tobytes() == st[0].tobytes()


MALFORMED = ["count_above_pitch", "negative_count", "a_equals_b", "nan_weight", "negative_weight", "inf_translation", "zero_quaternion",
             "negative_index", "index_too_large", "edge_scale_zero", "edge_scale_negative", "edge_scale_nan", "edge_scale_inf",
             "node_scale_zero", "node_scale_negative", "node_scale_nan", "node_zero_quaternion", "node_inf_translation",
             "w_scale_negative", "w_scale_nan", "w_scale_inf"]


@pytest.mark.parametrize("how", MALFORMED)
def test_malformed_graphs_are_flagged_and_untouched(ctx, how):
    n0, e = _case("n3_chord")[:2]
    nodes = n0.copy()
    edges = np.zeros((1, 4), s3.EDGE)
    edges[0, :len(e)] = e
    counts = np.array([len(e)], np.int32)
    if how == "count_above_pitch":
        counts[0] = 5
    elif how == "negative_count":
        counts[0] = -1
    elif how == "a_equals_b":
        edges[0, 1]["a"] = edges[0, 1]["b"]
    elif how == "nan_weight":
        edges[0, 2]["w_rot"] = np.nan
    elif how == "negative_weight":
        edges[0, 2]["w_trans"] = -1.0
    elif how == "inf_translation":
        edges[0, 0]["srt"][5] = np.inf
    elif how == "zero_quaternion":
        edges[0, 0]["srt"][:4] = 0
    elif how == "negative_index":
        edges[0, 2]["a"] = -1
    elif how == "index_too_large":
        edges[0, 2]["b"] = 3
    elif how.startswith("edge_scale_"):
        edges[0, 1]["srt"][7] = dict(zero=0.0, negative=-1.0, nan=np.nan, inf=np.inf)[how[11:]]
    elif how.startswith("node_scale_"):
        nodes[2, 7] = dict(zero=0.0, negative=-0.5, nan=np.nan)[how[11:]]
    elif how == "node_zero_quaternion":
        nodes[0, :4] = 0
    elif how == "node_inf_translation":
        nodes[1, 4] = -np.inf
    else:
        edges[0, 0]["w_scale"] = dict(negative=-1e-3, nan=np.nan, inf=np.inf)[how[8:]]
    rn, rst = s3.solve_batch(nodes[None], 1, edges, counts, 3)
    assert rst[0, 7] == -1 and rn[0].tobytes() == nodes.tobytes()
    for fixed_scale in (False, True):
        got, st = _batch(ctx, nodes[None], 1, edges, counts, 3, fixed_scale)
        assert st[0, 7] == -1 and not st[0, :7].any() and got[0].tobytes() == nodes.tobytes()
    if how not in ("count_above_pitch", "negative_count"):
        with pytest.raises(capi.TBError) as ei:
            ctx.pose_graph_sim3(nodes, 1, edges[0, :3], 3)
        assert ei.value.code == capi.TB_EINVAL


def test_argument_errors(ctx):
    nodes0, edges = _case("n3_chord")[:2]
    dn = torch.from_numpy(nodes0.copy()).cuda()
    de = torch.from_numpy(edges.copy().view(np.uint8)).cuda()
    dc = torch.tensor([len(edges)], dtype=torch.int32, device="cuda")
    call = lambda G, n, nf, pitch, it, p=None, e=None, c=None, fs=0: ctx.pose_graph_sim3_dev(
        G, n, nf, dn.data_ptr() if p is None else p, de.data_ptr() if e is None else e, dc.data_ptr() if c is None else c, pitch, it,
        fixed_scale=fs)
    assert call(1, 3, 1, 3, 3) == capi.TB_OK and call(1, 3, 1, 3, 3, fs=1) == capi.TB_OK
    assert call(0, 3, 1, 3, 3) == capi.TB_OK
    for bad in ((1, 3, 0, 3, 3), (1, 3, 3, 3, 3), (1, 1, 1, 3, 3), (1, 3, 1, 0, 3), (1, 3, 1, 3, -1), (-1, 3, 1, 3, 3)):
        assert call(*bad) == capi.TB_EINVAL, bad
    assert call(1, 3, 1, 3, 3, fs=2) == capi.TB_EINVAL and call(1, 3, 1, 3, 3, fs=-1) == capi.TB_EINVAL
    assert call(1, 3, 1, 3, 3, p=0) == capi.TB_EINVAL and call(1, 3, 1, 3, 3, e=0) == capi.TB_EINVAL and call(1, 3, 1, 3, 3, c=0) == capi.TB_EINVAL
    for unsupported in ((1, 65, 1, 3, 3), (1, 3, 1, 257, 3), (1, 3, 1, 3, 100)):
        assert call(*unsupported) == capi.TB_EUNSUPPORTED, unsupported
    ctx.synchronize()
    # the planning call: the same checks, and a shape planned ahead runs
    assert ctx.pose_graph_sim3_plan(3, 64, 1, 256) == capi.TB_OK and ctx.pose_graph_sim3_plan(0, 3, 1, 3) == capi.TB_OK
    assert ctx.pose_graph_sim3_plan(1, 3, 0, 3) == capi.TB_EINVAL and ctx.pose_graph_sim3_plan(1, 3, 3, 3) == capi.TB_EINVAL
    assert ctx.pose_graph_sim3_plan(1, 65, 1, 3) == capi.TB_EUNSUPPORTED and ctx.pose_graph_sim3_plan(1, 3, 1, 257) == capi.TB_EUNSUPPORTED
    assert call(1, 3, 1, 3, 3) == capi.TB_OK
    ctx.synchronize()
    with pytest.raises(capi.TBError) as ei:
        ctx.pose_graph_sim3(np.tile(nodes0[:1], (65, 1)), 1, edges, 3)
    assert ei.value.code == capi.TB_EUNSUPPORTED
    with pytest.raises(capi.TBError) as ei:
        ctx.pose_graph_sim3(nodes0, 1, np.zeros(257, s3.EDGE), 3)
    assert ei.value.code == capi.TB_EUNSUPPORTED
    got, st = ctx.pose_graph_sim3(nodes0, 1, edges[:0], 3)       # no edge: nothing to do, nothing flagged
    assert not st.any() and got.tobytes() == nodes0.tobytes()
