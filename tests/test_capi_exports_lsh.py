"""CPU tests: the library exports the searchByNN matcher's entry points and kernel, the header declares them, the bindings list
them, the tracker struct keeps its layout, and the "lsh" tracker fills the reference's arguments (test/test_vo.cpp:213,
matcher.cpp:17-18)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from trackingbench_slam_amd import capi, vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("tb_lsh_draw_bits", "tb_lsh_create", "tb_lsh_destroy", "tb_lsh_info", "tb_match_lsh", "tb_search_by_nn",
        "tb_search_by_nn_batch_dev", "tb_vo_create_lsh")


def test_library_exports_the_lsh_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    hdr = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tb_[a-z0-9_]+)\s*\(", hdr))
    for s in SYMS:
        assert s in syms and s in declared and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    data = open(libpath, "rb").read()
    assert b"k_lsh_nn" in data and b"gfx950" in data
    for name in ("lsh", "match_lsh", "search_by_nn", "search_by_nn_batch_dev"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(capi.lsh_draw_bits)


def test_the_header_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for words in ("Matcher::searchByNN", "LshIndexParams(20, 10, 2)", "UNPINNED", "Fisher-Yates", "0x9E3779B97F4A7C15", "popcount(key_t",
                  "TB_VO_NN = 6"):
        assert words in hdr, words
    shim = open(os.path.join(ROOT, "include", "matchers", "matcher.h")).read()
    assert "searchByNN" in shim and "NN(LSH)" not in shim


def test_tracker_kind_and_struct_layouts():
    assert capi.TB_VO_NN == 6 and capi.TB_VO_BOW == 5
    assert C.sizeof(capi.VOTracker) == 13 * 4                 # tb_vo_tracker is unchanged
    assert [f[0] for f in capi.VOLsh._fields_] == ["ratio", "min_th", "min_level", "max_level", "tables", "key_size", "multi_probe_level",
                                                    "seed", "bits"]
    assert C.sizeof(capi.VOLsh) == 48 and capi.VOLsh.seed.offset == 32 and capi.VOLsh.bits.offset == 40


def test_reference_defaults():
    t = vo._tracker("lsh", 5, {})
    assert isinstance(t, capi.VOLsh)
    assert (t.ratio, t.min_th, t.min_level, t.max_level, t.tables, t.key_size, t.multi_probe_level, t.seed) == (10.0, 30.0, 0, 5, 20, 10, 2, 0)
    assert not t.bits
    assert vo._tracker("lsh", 8, {}).max_level == 8
    bits = capi.lsh_draw_bits(4, 16, 3)
    t = vo._tracker("lsh", 5, dict(tables=4, key_size=16, multi_probe_level=1, seed=9, bits=bits, ratio=3.0, min_th=64.0, max_level=4))
    assert (t.ratio, t.min_th, t.max_level, t.tables, t.key_size, t.multi_probe_level, t.seed) == (3.0, 64.0, 4, 4, 16, 1, 9)
    assert t.bits == t._bits.ctypes.data and np.array_equal(t._bits, bits)
    with pytest.raises(ValueError):
        vo._tracker("lsh", 5, dict(bits=bits))                  # a [4, 16] table for (20, 10)
    with pytest.raises(TypeError):
        vo._tracker("lsh", 5, dict(radius=5.0))
    with pytest.raises(TypeError):
        vo._tracker("bf", 5, dict(tables=20))
    with pytest.raises(ValueError) as e:                          # the tracker is called "lsh": "nn" stays unknown
        vo._tracker("nn", 5, {})
    assert "'bow'" in str(e.value) and "'lsh'" in str(e.value)
    # the other trackers' defaults are what they were
    t = vo._tracker("bf", 5, {})
    assert (t.kind, t.bf_ratio, t.bf_min_th, t.min_level, t.max_level) == (capi.TB_VO_BF, 10.0, 30.0, 0, 5)


def _prm():
    return capi.VOParams(1241, 376, 5, 0.8, 2000, 80.0, 30.0, (C.c_double * 4)(718.856, 718.856, 607.1928, 185.2157), 386.1448, 10)


def test_null_arguments_are_refused_before_any_device_call():
    L = capi.lib()
    h = C.c_void_p()
    prm, lsh = _prm(), vo._tracker("lsh", 5, {})
    assert L.tb_vo_create_lsh(None, C.byref(prm), C.byref(lsh), 1, C.byref(h)) == capi.TB_EINVAL and not h.value
    assert L.tb_lsh_create(None, 20, 10, 2, C.c_uint64(0), None, C.byref(h)) == capi.TB_EINVAL and not h.value
    assert L.tb_lsh_info(None, None, None, None, None) == capi.TB_EINVAL
    n = C.c_int(5)
    assert L.tb_match_lsh(None, None, None, 0, None, 0, None, 0, C.byref(n)) == capi.TB_EINVAL
    assert L.tb_search_by_nn(None, None, None, 0, None, 0, C.c_float(10), C.c_float(30), None, 0, C.byref(n)) == capi.TB_EINVAL
    assert L.tb_search_by_nn_batch_dev(None, None, 0, None, None, None, None, C.c_size_t(64), C.c_float(10), C.c_float(30), None, 1, None) == capi.TB_EINVAL
    L.tb_lsh_destroy(None)
    tr = capi.VOTracker()
    tr.kind = capi.TB_VO_NN                                       # tb_vo_create_ex without a context: refused as any call is
    assert L.tb_vo_create_ex(None, C.byref(prm), C.byref(tr), 1, C.byref(h)) == capi.TB_EINVAL and not h.value
