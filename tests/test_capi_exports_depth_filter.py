"""CPU tests: the library declares, binds and exports the depth filter, its kernels are in the built code object, the record
layouts are what the C compiler sees, and the header states the rules."""
import ctypes as C
import os
import re
import subprocess

from trackingbench_slam_amd import capi

NEW = ("tb_depth_filter_create", "tb_depth_filter_destroy", "tb_depth_filter_clear", "tb_depth_filter_add_keyframe_dev",
       "tb_depth_filter_update_dev", "tb_depth_filter_points_dev", "tb_depth_filter_state_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_filter():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_df_update", b"k_df_add", b"k_df_copy", b"k_df_points"):
        assert k in blob, k
    assert "k_depth_filter.hip" in open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "k_depth_filter.hip")).read()
    # the integer stage is wave sums of integers, the compaction the shared one, every launch the library's one path, no atomics
    assert "tb_wave_sum(" in src and "tb_block_ordered_slot(" in src and "tb_launch(" in src
    assert "hipLaunchKernelGGL" not in src and not re.search(r"atomic[A-Z_(]", src)


def test_header_declares_it_and_states_the_rules():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_depth_filter_params \{", text) and "typedef struct tb_depth_filter tb_depth_filter;" in text
    for words in ("tests/depth_filter_reference.py", "matcher.cpp:1518-1592", "matcher.cpp:1247-1364",
                  "mu = 1 / depth_mean, z_range = 1 / depth_min, sigma2 = z_range^2 / 36, a = b = 10",
                  "d_max = 1 / max(mu - sqrt(sigma2), 1e-8)", "BEHIND", "OUTSIDE", "a margin of 5 px", "outside (1/3, 3)",
                  "floor of the bilinear sample, 0 outside", "n = max(1, floor(epi_len / 0.7))", "n > max_steps is NO_MATCH",
                  "floor(p + 0.5)", "closer than 4 to the border", "64 (sum AA - 2 sum AB + sum BB) -", "the first minimum wins",
                  "a best score >= 64 zmssd_max", "p[t] = p[t] + p[t ^ d]", "the 0.03 px stop", "|det A'A| < 1e-6 is DEGENERATE",
                  "px_error_angle = 2 atan(px_noise /", "tau_inv = 0.5 (1 / max(1e-7, z - tau) - 1 / (z + tau))", "NONFINITE",
                  "NO_MATCH is b += 1 and nothing else", "sqrt(sigma2) < z_range / conv_div", "Tcw_ref^-1 (f / mu)",
                  "takes the slot after the newest one", "in ascending entry order", "their count is returned",
                  "an inactive sequence keeps every byte", "ref_slots outside 1..16", "align_iters outside 0..99",
                  "an image under 16 px in either dimension", "A filter that is never created changes nothing in any other call",
                  "no host synchronisation, no copy"):
        assert words in text, words
    types = open(os.path.join(ROOT, "include", "tb_types.h")).read()
    assert re.search(r"typedef struct tb_df_seed \{", types) and re.search(r"typedef struct tb_df_trace \{", types)


def test_bindings_exist_and_the_layouts():
    for m in ("clear", "add_keyframe_dev", "update_dev", "points_dev", "state_dev", "close"):
        assert callable(getattr(capi.DepthFilter, m)), m
    assert capi.DF_SEED.itemsize == 64 and capi.DF_TRACE.itemsize == 56
    assert capi.DF_SEED.names == ("mu", "sigma2", "a", "b", "z_range", "u", "v", "slot", "state", "updates", "reserved")
    assert capi.DF_TRACE.names == ("score", "px", "py", "z", "tau", "flag", "n", "win", "reserved")
    assert C.sizeof(capi.DepthFilterParams) == 48
    assert [(f[0], getattr(capi.DepthFilterParams, f[0]).offset) for f in capi.DepthFilterParams._fields_] == \
        [("depth_mean", 0), ("depth_min", 8), ("conv_div", 16), ("px_noise", 24), ("max_steps", 32), ("zmssd_max", 36),
         ("align_iters", 40), ("reserved", 44)]
    p = capi.depth_filter_params()
    assert (p.depth_mean, p.depth_min, p.conv_div, p.px_noise, p.max_steps, p.zmssd_max, p.align_iters) == (15.0, 2.0, 200.0, 1.0, 1000, 2000, 10)
    # the definition states the same layouts
    import depth_filter_reference as dfr
    assert dfr.DF_SEED == capi.DF_SEED and dfr.DF_TRACE == capi.DF_TRACE
    src = open(os.path.join(ROOT, "trackingbench_slam_amd", "depth_filter.py")).read()
    for m in ("def add_keyframe(self, images, Tcw, keys, counts, skip=None, active=None)", "def update(self, images, Tcw, active=None)",
              "def seeds(self)", "def trace(self)", "def points(self, release=False)"):
        assert m in src, m


def test_sizeof_the_records_in_c(tmp_path):
    """the layouts as the compiler that builds the shim sees the headers"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include "tb_capi.h"\n'
                   "static_assert(sizeof(tb_df_seed) == 64 && offsetof(tb_df_seed, z_range) == 32 && offsetof(tb_df_seed, u) == 40 && "
                   "offsetof(tb_df_seed, slot) == 48 && offsetof(tb_df_seed, state) == 52 && offsetof(tb_df_seed, updates) == 56, \"seed\");\n"
                   "static_assert(sizeof(tb_df_trace) == 56 && offsetof(tb_df_trace, score) == 0 && offsetof(tb_df_trace, px) == 8 && "
                   "offsetof(tb_df_trace, tau) == 32 && offsetof(tb_df_trace, flag) == 40 && offsetof(tb_df_trace, win) == 48, \"trace\");\n"
                   "static_assert(sizeof(tb_depth_filter_params) == 48 && offsetof(tb_depth_filter_params, px_noise) == 24 && "
                   "offsetof(tb_depth_filter_params, max_steps) == 32 && offsetof(tb_depth_filter_params, align_iters) == 40, \"params\");\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
