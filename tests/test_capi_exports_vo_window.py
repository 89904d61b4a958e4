"""CPU tests: the library declares, binds and exports the window BA of the optical-flow VO loop, its kernels are in the built code
object, and StereoVO checks its arguments before anything touches a device."""
import inspect
import os
import re
import subprocess

import pytest

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import WINDOW_BA_DEFAULTS, StereoVO

NEW = ("tb_vo_window_ba_enable", "tb_vo_window_state_dev")
KERNELS = (b"k_vo_seg_log", b"k_vo_seg_window", b"k_vo_seg_adopt", b"k_vo_seg_start")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_window_ba_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in KERNELS:
        assert k in blob, k


def test_header_declares_them_and_states_the_rules():
    text = open(HEADER).read()
    for s in NEW:
        assert re.search(r"\bint %s\(tb_vo\* vo" % s, text), s
    assert re.search(r"typedef struct tb_vo_window_ba \{", text)
    for field in ("iters", "fixed", "min_obs", "min_points"):
        assert re.search(r"\bint %s;" % field, text), field
    assert "tests/vo_window_reference.py" in text
    assert "Local BA is not part of the loop unless" in text
    doc = text[text.index("Window BA in a TB_VO_OPFLOW loop"):text.index("int tb_vo_window_state_dev(")]
    for word in ("TB_ESTATE", "TB_EINVAL", "TB_EUNSUPPORTED", "synchronises the stream once", "Tracking steps stay free of host synchronisation"):
        assert word in doc, word
    # the ragged entry points refuse an enabled loop, and the header says so next to the other ragged rules
    assert "tb_vo_window_ba_enable" in text[text.index("ragged batches"):text.index("int tb_vo_frames(")]


def test_bindings_exist():
    for m in ("window_ba_enable", "window_state_dev"):
        assert callable(getattr(capi.VO, m)), m
    assert callable(StereoVO.window)
    assert "window_ba" in inspect.signature(StereoVO.__init__).parameters
    assert [f[0] for f in capi.VOWindowBA._fields_] == ["iters", "fixed", "min_obs", "min_points"]
    assert WINDOW_BA_DEFAULTS == dict(iters=10, fixed=1, min_obs=2, min_points=3)


def test_arguments_are_checked_before_anything_touches_a_device():
    for kind in ("bf", "violence", "projection", "projection_map"):
        with pytest.raises(TypeError):
            StereoVO(1, tracker=kind, window_ba=True)
    with pytest.raises(TypeError):
        StereoVO(1, tracker="bow", vocab=object(), window_ba=True)
    with pytest.raises(TypeError):
        StereoVO(1, window_ba=dict(iterations=3))
    # which= / active= / keyframe= on an enabled loop
    vo = StereoVO.__new__(StereoVO)
    vo.S, vo.tracker, vo.db, vo.window_ba = 3, "opflow", None, dict(WINDOW_BA_DEFAULTS)
    with pytest.raises(TypeError):
        vo._ragged_ok()
    with pytest.raises(TypeError):
        vo.reset(None, which=[0])
    vo.window_ba = None
    vo._ragged_ok()
    vo.vo = None   # nothing to close
