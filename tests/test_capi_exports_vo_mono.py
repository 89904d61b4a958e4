"""CPU tests: the library declares, binds and exports the linear triangulation and the mono mode of the optical-flow VO loop,
their kernels are in the built code object, the structs have the sizes the header gives them, and StereoVO checks mono='s
arguments before anything touches a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from trackingbench_slam_amd import capi
from trackingbench_slam_amd.vo import MONO_DEFAULTS, StereoVO

NEW = ("tb_linear_triangle", "tb_linear_triangle_batch_dev", "tb_vo_mono_enable", "tb_vo_mono_state_dev")
KERNELS = (b"k_linear_triangle", b"k_vo_kf_merge", b"k_vo_mono_alive")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_entry_points():
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
    for s in NEW[:2]:
        assert re.search(r"\bint %s\(tb_ctx\* ctx" % s, text), s
    for s in NEW[2:]:
        assert re.search(r"\bint %s\(tb_vo\* vo" % s, text), s
    assert re.search(r"typedef struct tb_triangulate_params \{", text) and re.search(r"typedef struct tb_vo_mono \{", text)
    assert "tests/triangulate_reference.py" in text and "tests/vo_mono_reference.py" in text
    doc = text[text.index("Monocular map growth in a TB_VO_OPFLOW loop"):text.index("int tb_vo_mono_state_dev(")]
    for word in ("TB_ESTATE", "TB_EINVAL", "TB_EUNSUPPORTED", "no host synchronisation", "tb_vo_step_ragged_dev", "tb_vo_window_ba_enable"):
        assert word in doc, word
    tri = text[text.index("LocalBA::LinearTriangle, LocalBA.cpp:24-43"):text.index("int tb_linear_triangle_batch_dev(")]
    for word in ("DEVIATION", "6 cyclic Jacobi sweeps", "WRITTEN ONLY WHERE ACCEPTED", "cos_parallax_max", "chi2_max"):
        assert word in tri, word


def test_struct_sizes():
    """tb_triangulate_params: two doubles; tb_vo_mono: two doubles and an int, padded to the doubles' alignment"""
    assert C.sizeof(capi.TriangulateParams) == 16
    assert [f[0] for f in capi.TriangulateParams._fields_] == ["cos_parallax_max", "chi2_max"]
    assert C.sizeof(capi.VOMono) == 24 and capi.VOMono.cell.offset == 16
    assert [f[0] for f in capi.VOMono._fields_] == ["cos_parallax_max", "chi2_max", "cell"]


def test_bindings_exist():
    for m in ("mono_enable", "mono_state_dev"):
        assert callable(getattr(capi.VO, m)), m
    for m in ("linear_triangle", "linear_triangle_batch_dev"):
        assert callable(getattr(capi.Context, m)), m
    assert callable(StereoVO.mono)
    assert "mono" in inspect.signature(StereoVO.__init__).parameters
    assert MONO_DEFAULTS == dict(cos_parallax_max=0.9998, chi2_max=5.991, cell=8)


def test_arguments_are_checked_before_anything_touches_a_device():
    with pytest.raises(TypeError):
        StereoVO(1, mono=dict(cells=4))
    vo = StereoVO.__new__(StereoVO)
    vo.mono_params = None
    with pytest.raises(capi.TBError) as e:
        vo.mono()
    assert e.value.code == capi.TB_ESTATE
    # which= / active= / keyframe= on a mono loop
    vo.S, vo.tracker, vo.db, vo.window_ba, vo.mono_params = 3, "opflow", None, None, dict(MONO_DEFAULTS)
    with pytest.raises(TypeError):
        vo._ragged_ok()
    with pytest.raises(TypeError):
        vo.reset(None, which=[0])
    vo.mono_params = None
    vo._ragged_ok()
    vo.vo = None   # nothing to close
