"""CPU tests: the library exports the projection trackers' entry points and the bindings fill the reference's arguments
(test/test_projection.cpp:512-517)."""
import ctypes as C
import subprocess

import pytest

from trackingbench_slam_amd import capi, vo


def test_library_exports_the_map_accessors():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("tb_vo_map_state_dev", "tb_vo_mp_desc_dev"):
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_tracker_kinds_and_struct_layout():
    assert (capi.TB_VO_OPFLOW, capi.TB_VO_BF, capi.TB_VO_VIOLENCE) == (0, 1, 2)     # unchanged
    assert (capi.TB_VO_PROJECTION, capi.TB_VO_PROJECTION_MAP) == (3, 4)
    names = [f[0] for f in capi.VOTracker._fields_]
    # the new fields are appended: the existing ones keep their offsets
    assert names[:10] == ["kind", "bf_ratio", "bf_min_th", "min_level", "max_level", "radius", "th_low", "nratio", "histo_len",
                          "check_orientation"]
    assert names[10:] == ["th_high", "radio", "map_keyframes"]
    assert C.sizeof(capi.VOTracker) == 13 * 4


def test_reference_defaults():
    t = vo._tracker("projection_map", 5, {})
    assert t.kind == capi.TB_VO_PROJECTION_MAP
    assert (t.nratio, t.th_high, t.map_keyframes) == (20.0, 50, 4)
    assert t.radio == pytest.approx(0.6, rel=1e-7)    # the float nearest 0.6
    t = vo._tracker("projection", 5, {})
    assert t.kind == capi.TB_VO_PROJECTION
    assert (t.nratio, t.th_high, t.histo_len, t.check_orientation) == (30.0, 50, 30, 1)
    t = vo._tracker("projection_map", 5, dict(map_keyframes=2, radio=0.8))
    assert t.map_keyframes == 2 and t.radio == pytest.approx(0.8, rel=1e-7)
    with pytest.raises(TypeError):
        vo._tracker("projection", 5, dict(map_keyframes=2))     # the keyframe tracker has no map
    with pytest.raises(TypeError):
        vo._tracker("projection_map", 5, dict(radius=5.0))
    # the existing trackers' defaults are what they were
    t = vo._tracker("violence", 5, {})
    assert (t.kind, t.max_level, t.radius, t.th_low, t.nratio, t.histo_len, t.check_orientation) == (capi.TB_VO_VIOLENCE, 5, 50.0, 50, 6.0, 30, 1)
    assert (t.th_high, t.radio, t.map_keyframes) == (0, 0.0, 0)
