"""CPU tests: the library declares, binds and exports the Sim(3) pose-graph optimiser and its two graph queries, their kernels are
in the built code object, and the Python helpers agree with tests/pose_graph_sim3_reference.py."""
import os
import re
import subprocess

import numpy as np

import pose_graph_sim3_reference as s3
from trackingbench_slam_amd import capi

NEW = ("tb_pose_graph_sim3", "tb_pose_graph_sim3_batch_dev", "tb_pose_graph_sim3_plan", "tb_kf_store_sim3_graph_dev", "tb_vo_loop_sim3_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_points_and_holds_the_kernels():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    assert capi.EXPORTS[-len(NEW):] == list(NEW)                      # appended
    blob = open(libpath, "rb").read()
    assert b"k_pgo_sim3" in blob and b"k_sim3_graph" in blob


def test_header_declares_them_and_the_records():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert "tests/pose_graph_sim3_reference.py" in text and "tests/sim3_graph_reference.py" in text
    types = open(os.path.join(ROOT, "include", "tb_types.h")).read()
    assert re.search(r"typedef struct tb_pg_sim3_edge \{", types) and re.search(r"typedef struct tb_sim3_graph_out \{", types)
    for field in (r"int32_t a, b;", r"double srt\[8\];", r"double w_rot, w_trans, w_scale;"):
        assert re.search(field, types), field


def test_bindings_exist_and_the_edge_layout_is_the_reference_one():
    for m in ("pose_graph_sim3", "pose_graph_sim3_dev", "pose_graph_sim3_plan"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(capi.KeyframeStore.sim3_graph) and callable(capi.KeyframeStore.sim3_graph_rc)
    from trackingbench_slam_amd.vo import StereoVO
    assert callable(StereoVO.loop_sim3)
    assert capi.PG_SIM3_EDGE == s3.EDGE and capi.PG_SIM3_EDGE.itemsize == 96
    assert [capi.PG_SIM3_EDGE.fields[f][1] for f in ("a", "b", "srt", "w_rot", "w_trans", "w_scale")] == [0, 4, 8, 72, 80, 88]
    assert capi.C.sizeof(capi.Sim3GraphOut) == 8 * 8 and capi.Sim3GraphOut.nnodes.offset == 8


def _elements(rng, n):
    S = [s3.exp(np.concatenate([rng.normal(0, 1.5, 3), rng.normal(0, 3, 3), rng.normal(0, 0.5, 1)])) for _ in range(n)]
    return S + [s3.make(2.0, np.diag([1.0, -1.0, -1.0]), (1, 2, 3)), s3.make(0.5, np.diag([-1.0, 1.0, -1.0]), (0, 0, 0))]   # w = 0: the other branches


def test_matrix_converters_agree_with_the_reference():
    rng = np.random.default_rng(2)
    S = np.stack(_elements(rng, 12))
    srt = capi.sim3_from_matrix(S)
    assert srt.shape == (14, 8) and np.all(srt[:, 0] >= 0)
    for i in range(len(S)):
        assert srt[i].tobytes() == s3.srt_from_matrix(S[i]).tobytes()            # one rule, the kernel's
        assert np.abs(capi.sim3_to_matrix(srt[i]) - s3.srt_to_matrix(srt[i])).max() < 1e-15
        assert np.abs(capi.sim3_to_matrix(srt[i]) - S[i]).max() < 1e-14 * max(1.0, np.abs(S[i]).max())
    assert capi.sim3_from_matrix(S[0]).shape == (8,) and capi.sim3_to_matrix(srt).shape == (14, 4, 4)
    flipped = srt[3].copy()
    flipped[:4] *= -2.5          # neither unit nor w >= 0: normalised as the kernel normalises
    assert np.abs(capi.sim3_to_matrix(flipped) - capi.sim3_to_matrix(srt[3])).max() < 1e-15


def test_edge_builder_agrees_with_the_reference():
    rng = np.random.default_rng(3)
    Z = np.stack(_elements(rng, 6))
    pairs = [(i, i + 1) for i in range(len(Z))]
    e = capi.pose_graph_sim3_edges(pairs, Z, 2.0, 0.5, 3.0)
    for i in range(len(Z)):
        r = s3.make_edge(i, i + 1, Z[i], 2.0, 0.5, 3.0)
        assert e[i].tobytes() == np.asarray(r).tobytes()
    srt = capi.sim3_from_matrix(Z)
    srt[0, :4] *= -1.0           # records are copied as they are: a solver's best_srt stays byte for byte
    e2 = capi.pose_graph_sim3_edges(pairs, srt, w_scale=np.arange(len(Z), dtype=np.float64))
    assert e2["srt"].tobytes() == srt.tobytes() and e2["w_scale"].tolist() == list(range(len(Z))) and np.all(e2["w_rot"] == 1.0)
