"""CPU tests: the library exports the searchByBow loop's entry points and the BowVector kernel, the existing tracker struct keeps
its layout, and the bindings fill the reference's arguments (test/test_vo.cpp:706-711, :207-212)."""
import ctypes as C
import subprocess

import pytest

from trackingbench_slam_amd import capi, vo


def test_library_exports_the_bow_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("tb_bow_vector_batch_dev", "tb_vo_create_bow", "tb_vo_bow_state_dev"):
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    assert b"k_bow_vector" in open(libpath, "rb").read()


def test_tracker_kind_and_struct_layouts():
    assert capi.TB_VO_BOW == 5
    assert (capi.TB_VO_OPFLOW, capi.TB_VO_BF, capi.TB_VO_VIOLENCE, capi.TB_VO_PROJECTION, capi.TB_VO_PROJECTION_MAP) == (0, 1, 2, 3, 4)
    assert C.sizeof(capi.VOTracker) == 13 * 4                 # tb_vo_tracker is unchanged
    assert [f[0] for f in capi.VOBow._fields_] == ["levelsup", "map_point_only", "th_low", "nratio", "histo_len", "check_orientation"]
    assert C.sizeof(capi.VOBow) == 6 * 4


def _create(bow, params=None):
    prm = params or capi.VOParams(1241, 376, 5, 0.8, 2000, 80.0, 30.0, (C.c_double * 4)(718.856, 718.856, 607.1928, 185.2157), 386.1448, 10)
    h = C.c_void_p()
    rc = capi.lib().tb_vo_create_bow(None, C.byref(prm), C.byref(bow) if bow is not None else None, None, 1, C.byref(h))
    assert not h.value
    return rc


def test_a_zeroed_tb_vo_bow_is_refused():
    """the arguments are checked before anything touches a device: a zero-initialised struct (histo_len 0), a null struct and the
    out-of-range fields are TB_EINVAL"""
    assert _create(capi.VOBow()) == capi.TB_EINVAL
    assert _create(None) == capi.TB_EINVAL
    good = dict(levelsup=4, map_point_only=1, th_low=50, nratio=6.0, histo_len=30, check_orientation=1)
    for bad in (dict(histo_len=0), dict(histo_len=1025), dict(levelsup=-1), dict(th_low=-1)):
        assert _create(capi.VOBow(**dict(good, **bad))) == capi.TB_EINVAL, bad
    assert _create(capi.VOBow(**good)) == capi.TB_EINVAL       # no context, no vocabulary


def test_reference_defaults():
    t = vo._tracker("bow", 5, {})
    assert isinstance(t, capi.VOBow)
    assert (t.levelsup, t.map_point_only, t.th_low, t.nratio, t.histo_len, t.check_orientation) == (4, 1, 50, 6.0, 30, 1)
    t = vo._tracker("bow", 5, vo.BOW_TEST_VO_1)
    assert (t.levelsup, t.map_point_only, t.th_low, t.nratio, t.histo_len, t.check_orientation) == (4, 0, 30, 5.0, 30, 1)
    with pytest.raises(TypeError):
        vo._tracker("bow", 5, dict(radius=5.0))
    with pytest.raises(ValueError) as e:
        vo._tracker("nn", 5, {})
    assert "'bow'" in str(e.value)
    # the other trackers' defaults are what they were
    t = vo._tracker("violence", 5, {})
    assert (t.kind, t.max_level, t.radius, t.th_low, t.nratio, t.histo_len, t.check_orientation) == (capi.TB_VO_VIOLENCE, 5, 50.0, 50, 6.0, 30, 1)
