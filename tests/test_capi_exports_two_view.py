"""CPU tests: the library declares, binds and exports the two-view solver, the kernel is in the built code object, and the
argument checks that need no device answer."""
import ctypes as C
import os
import re
import subprocess

from trackingbench_slam_amd import capi

NEW = ("tb_two_view", "tb_two_view_batch_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_two_view_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    assert b"k_two_view" in open(libpath, "rb").read()
    assert "k_two_view.hip" in open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "Makefile")).read()


def test_header_declares_them_and_states_the_rules():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_two_view_params \{", text)
    for words in ("tests/two_view_reference.py", "(16 h + k + 1) * 0x9E3779B97F4A7C15", "ReconstructF", "ties to the lower candidate",
                  "WRITTEN ONLY", "TB_TWO_VIEW_MAX_PITCH 4096"):
        assert words in text, words


def test_bindings_exist_and_the_params_layout():
    for m in ("two_view", "two_view_dev"):
        assert callable(getattr(capi.Context, m)), m
    # int, pad, double, int, pad, two doubles, two doubles, int, pad, double, uint64
    assert C.sizeof(capi.TwoViewParams) == 80
    assert [(f[0], getattr(capi.TwoViewParams, f[0]).offset) for f in capi.TwoViewParams._fields_] == [
        ("hypotheses", 0), ("chi2_epi", 8), ("refit", 16), ("tri", 24), ("min_good_ratio", 40), ("ambiguity_ratio", 48),
        ("min_points", 56), ("baseline", 64), ("seed", 72)]
    d = capi.two_view_params()
    assert (d.hypotheses, d.chi2_epi, d.refit, d.tri.cos_parallax_max, d.tri.chi2_max, d.min_good_ratio, d.ambiguity_ratio, d.min_points,
            d.baseline) == (256, 3.841, 1, 0.9998, 5.991, 0.9, 0.7, 50, 1.0)


def test_a_call_without_a_context_is_refused():
    prm = capi.two_view_params()
    L = capi.lib()
    none = [None] * 9
    assert L.tb_two_view_batch_dev(None, 1, None, None, None, 4, None, None, None, None, None, C.byref(prm), *none) == capi.TB_EINVAL
    assert L.tb_two_view(None, None, None, 0, None, None, None, None, None, C.byref(prm), *([None] * 9)) == capi.TB_EINVAL
