"""CPU tests: the library declares, binds and exports loop correction in the VO loop, and its kernels are in the built code object."""
import os
import re
import subprocess

import pytest

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import LOOP_DEFAULTS, StereoVO

NEW = ("tb_vo_loop_enable", "tb_vo_loop_state_dev", "tb_pose_graph_plan")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_loop_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_vo_loop_graph", b"k_vo_loop_adopt", b"k_pgo"):
        assert k in blob, k


def test_header_declares_them_and_no_longer_lists_loop_correction_as_missing():
    text = open(HEADER).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_vo_loop \{", text)
    for field in ("topk", "exclude_newest", "min_inliers", "iters"):
        assert re.search(r"\bint %s;" % field, text), field
    assert re.search(r"\bdouble w_rot, w_trans;", text)
    assert "tests/vo_loop_reference.py" in text
    assert "Loop correction and ORB-SLAM's second stage" not in text


def test_bindings_exist():
    for m in ("loop_enable", "loop_state_dev"):
        assert callable(getattr(capi.VO, m)), m
    assert callable(StereoVO.loop) and callable(capi.Context.pose_graph_plan)
    assert [f[0] for f in capi.VOLoop._fields_] == ["topk", "exclude_newest", "min_inliers", "iters", "w_rot", "w_trans"]
    assert LOOP_DEFAULTS == dict(topk=4, exclude_newest=1, min_inliers=50, iters=10, w_rot=1.0, w_trans=1.0)


def test_loop_close_needs_relocalize_and_excludes_recover():
    """checked before anything touches a device"""
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), keyframe_db=4, loop_close=True)
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), keyframe_db=4, relocalize=2, loop_close=dict(inliers=3))
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), keyframe_db=4, relocalize=2, recover=True, loop_close=True)
