"""CPU tests: the library declares, binds and exports the Sim(3) optimiser, the keyframe store's refinement query and the VO loop's,
and their kernels are in the built code object."""
import ctypes as C
import os
import re
import subprocess

from trackingbench_slam_amd import capi

NEW = ("tb_sim3_optimize", "tb_sim3_optimize_batch_dev", "tb_kf_store_sim3_refine_dev", "tb_kf_store_sim3_refine_state_dev",
       "tb_vo_refine_sim3_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_optimiser():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_sim3_opt", b"k_sim3_refine_prep", b"k_sim3_refine_select", b"k_sim3_rowsI15tb_sim3_obs_row", b"k_sim3_rowsI11tb_sim3_row"):
        assert k in blob, k
    assert "k_sim3_opt.hip" in open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "Makefile")).read()
    # the kernel includes the shared Exp; it does not restate it
    src = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "k_sim3_opt.hip")).read()
    assert '#include "tb_sim3.h"' in src and "s3_exp(" in src and not re.search(r"PoSim3\s+s3_exp\s*\(", src)
    # the row rule is stated once: one kernel template, instantiated for both row types
    rows = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "k_sim3.hip")).read()
    assert len(re.findall(r"^k_sim3_rows\(", rows, re.M)) == 1 and "template <typename Row>" in rows and rows.count("atomicMax(&win[q], k)") == 1


def test_header_declares_it_and_states_the_rules():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_sim3_opt_params \{", text) and re.search(r"typedef struct tb_sim3_refine_out \{", text)
    for words in ("tests/reloc_sim3_opt_reference.py", "row i of a pair is row i of the store's tb_sim3_row list", "a consensus below 3, is skipped",
                  "stats[7] = 2", "the store's own copy of best_srt takes the refined srt", "ORB-SLAM asks for 20",
                  "a store that never calls it launches and holds what it did before", "every step and reset invalidates it"):
        assert words in text, words
    for words in ("tests/sim3_opt_reference.py", "Optimizer::OptimizeSim3", "e12 = (u1, v1) - proj(Q1)", "e21 = (u2, v2) - proj(Q2)",
                  "delta = sqrt(th2)", "dQ1 / ddelta = [-[Q1]x | I | Q1]", "dQ2 / ddelta = -(1 / s) R12' [-[X1]x | I | X1]",
                  "S <- Exp(delta) S", "lambda0 = 1e-5 max |diag H|", "at most 10 trials", "p[t] = p[t] + p[t ^ d]",
                  "either of its two edges", "srt_out is srt_in byte for byte", "stats[7] = 1", "stats[7] = -1",
                  "iters_bad", "iters_clean", "chi2 = +inf", "s keeps its bytes", "an iteration count outside 0..99", "min_keep < 0"):
        assert words in text, words
    types = open(os.path.join(ROOT, "include", "tb_types.h")).read()
    assert re.search(r"typedef struct tb_sim3_obs_row \{", types)


def test_bindings_exist_and_the_layouts():
    for m in ("sim3_optimize", "sim3_optimize_dev"):
        assert callable(getattr(capi.Context, m)), m
    for m in ("sim3_refine", "sim3_refine_rc", "sim3_refine_state"):
        assert callable(getattr(capi.KeyframeStore, m)), m
    assert callable(capi.VO.refine_sim3_dev)
    from trackingbench_slam_amd import vo
    assert callable(vo.StereoVO.refine_sim3)
    assert C.sizeof(capi.Sim3RefineOut) == 8 * C.sizeof(C.c_void_p)
    # tb_sim3_obs_row: twelve floats, a tb_sim3_row with the four pixel fields before the weights
    assert capi.SIM3_OBS_ROW.itemsize == 48
    assert capi.SIM3_OBS_ROW.names == ("X1", "Y1", "Z1", "X2", "Y2", "Z2", "u1", "v1", "u2", "v2", "inv_sigma2_1", "inv_sigma2_2")
    assert set(capi.SIM3_ROW.names) <= set(capi.SIM3_OBS_ROW.names)
    assert C.sizeof(capi.Sim3OptParams) == 32
    assert [(f[0], getattr(capi.Sim3OptParams, f[0]).offset) for f in capi.Sim3OptParams._fields_] == \
        [("th2", 0), ("iters_first", 8), ("iters_bad", 12), ("iters_clean", 16), ("min_keep", 20), ("fixed_scale", 24)]
    p = capi.sim3_opt_params()
    assert (p.th2, p.iters_first, p.iters_bad, p.iters_clean, p.min_keep, p.fixed_scale) == (10.0, 5, 10, 5, 10, 0)


def test_sizeof_the_row_in_c(tmp_path):
    """sizeof(tb_sim3_obs_row) == 48 and the parameter block's layout, as the compiler that builds the shim sees the headers"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include "tb_capi.h"\n'
                   "static_assert(sizeof(tb_sim3_obs_row) == 48 && offsetof(tb_sim3_obs_row, u1) == 24 && "
                   "offsetof(tb_sim3_obs_row, inv_sigma2_1) == 40, \"row\");\n"
                   "static_assert(sizeof(tb_sim3_opt_params) == 32 && offsetof(tb_sim3_opt_params, th2) == 0 && "
                   "offsetof(tb_sim3_opt_params, iters_first) == 8 && offsetof(tb_sim3_opt_params, iters_bad) == 12 && "
                   "offsetof(tb_sim3_opt_params, iters_clean) == 16 && offsetof(tb_sim3_opt_params, min_keep) == 20 && "
                   "offsetof(tb_sim3_opt_params, fixed_scale) == 24, \"params\");\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
