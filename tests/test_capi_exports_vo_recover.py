"""CPU tests: the library declares, binds and exports recovery in the VO loop, and its kernels are in the built code object."""
import os
import re
import subprocess

import pytest

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import RECOVER_DEFAULTS, StereoVO

NEW = ("tb_vo_recover_enable", "tb_vo_recover_state_dev")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_recovery_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_vo_recover_adopt", b"k_vo_recover_switch", b"k_vo_recover_mask", b"k_vo_recover_ring_add"):
        assert k in blob, k


def test_header_declares_them_and_no_longer_lists_adoption_as_missing():
    text = open(HEADER).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_vo_recover \{", text)
    for field in ("lost_inliers", "topk", "exclude_newest", "min_inliers"):
        assert re.search(r"\bint %s;" % field, text), field
    assert "tests/vo_recover_reference.py" in text
    assert "Adopting the pose after a loss" not in text


def test_bindings_exist():
    for m in ("recover_enable", "recover_state_dev"):
        assert callable(getattr(capi.VO, m)), m
    for m in ("recovery", "recovery_rings"):
        assert callable(getattr(StereoVO, m)), m
    assert [f[0] for f in capi.VORecover._fields_] == ["lost_inliers", "topk", "exclude_newest", "min_inliers"]
    assert RECOVER_DEFAULTS == dict(lost_inliers=30, topk=4, exclude_newest=1, min_inliers=50)


def test_recover_needs_relocalize():
    """checked before anything touches a device"""
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), keyframe_db=4, recover=True)
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), keyframe_db=4, relocalize=2, recover=dict(inliers=3))
