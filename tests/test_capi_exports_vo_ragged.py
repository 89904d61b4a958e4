"""CPU tests: the library declares, binds and exports the ragged-batch entry points of the VO loop, and their kernels are in the
built code object."""
import inspect
import os
import re
import subprocess

import pytest

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import StereoVO

NEW = ("tb_vo_reset_seq_dev", "tb_vo_step_ragged_dev", "tb_vo_frames")
KERNELS = (b"k_vo_hold", b"k_vo_kf_snapshot", b"k_vo_kf_gather", b"k_vo_reset_seq")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_ragged_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in KERNELS:
        assert k in blob, k


def test_header_declares_them_and_says_what_is_unsupported():
    text = open(HEADER).read()
    for s in NEW:
        assert re.search(r"\bint %s\(tb_vo\* vo" % s, text), s
    assert re.search(r"tb_vo_step_ragged_dev\([^;]*const uint8_t\* active,\s*const uint8_t\* force_keyframe\);", text)
    for word in ("TB_VO_PROJECTION_MAP", "tb_vo_bow_db_enable", "TB_EUNSUPPORTED", "one host ->\n * device copy"):
        assert word in text[text.index("ragged batches"):text.index("int tb_vo_frames(")], word


def test_bindings_exist():
    for m in ("reset_seq_dev", "step_ragged_dev", "frames"):
        assert callable(getattr(capi.VO, m)), m
    assert callable(StereoVO.frames)
    assert "which" in inspect.signature(StereoVO.reset).parameters
    for p in ("active", "keyframe"):
        assert p in inspect.signature(StereoVO.step).parameters, p


def test_masks_are_checked_before_anything_touches_a_device():
    vo = StereoVO.__new__(StereoVO)
    vo.S = 3
    assert vo._mask(None, "active") is None
    assert vo._mask([2, 0], "active").tolist() == [True, False, True]
    assert vo._mask([True, False, False], "which").tolist() == [True, False, False]
    assert vo._mask([], "keyframe").tolist() == [False] * 3
    for bad in ([3], [-1], [True, False]):
        with pytest.raises(ValueError):
            vo._mask(bad, "active")
    vo.tracker, vo.db = "projection_map", None
    with pytest.raises(TypeError):
        vo._ragged_ok()
    vo.tracker, vo.db = "bow", object()
    with pytest.raises(TypeError):
        vo._ragged_ok()
    vo.vo = None   # nothing to close
