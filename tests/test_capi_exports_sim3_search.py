"""CPU tests: the library declares, binds and exports SearchBySim3 -- the operator, the keyframe store's query and the VO loop's -- and
its kernels are in the built code object."""
import ctypes as C
import os
import re
import subprocess

from trackingbench_slam_amd import capi

NEW = ("tb_search_by_sim3_batch_dev", "tb_kf_store_sim3_search_dev", "tb_vo_search_sim3_dev")
STATE = "tb_kf_store_sim3_search_state_dev"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_search():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW + (STATE,):
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_sim3_search", b"k_sim3_search_agree", b"k_sim3_search_prep", b"k_sim3_search_merge", b"k_sim3_search_select"):
        assert k in blob, k
    assert "k_sim3_search.hip" in open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "k_sim3_search.hip")).read()
    # the best candidate is a packed (distance, index) minimum, and no atomic decides anything
    assert "<< 32" in src and "atomic" not in src.replace("no atomic", "")
    assert "tb_block_ordered_slot" in src and "tb_launch" in src and "hipLaunchKernelGGL" not in src
    # the row rule is still stated once: the store's prep walks it through the same device function
    rows = open(os.path.join(ROOT, "trackingbench_slam_amd", "csrc", "k_sim3.hip")).read()
    assert rows.count("atomicMax(&win[q], k)") == 1 and rows.count("s3_row_winners(win, n, M, nm, nk, V1, V2)") == 2


def test_header_declares_it_and_states_the_rules():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    for s in NEW + (STATE,):
        assert re.search(r"\b%s\(" % s, text), s
    assert re.search(r"typedef struct tb_sim3_search_out \{", text)
    text = re.sub(r"\s*\n \*\s*", " ", text)      # a comment's line breaks are not part of what it says
    for words in ("tests/sim3_search_reference.py", "ORBmatcher::SearchBySim3", "P = R' (X1c[i] - t) / s", "skipped unless P.z > 0",
                  "0.8 minD <= d <= 1.2 maxD", "the smallest l with g[l] d >= maxD", "r = th g[L]", "octave L - 1 or L",
                  "a tie goes to the lowest j", "match1[i] = j and match2[j] = i", "new pairs are listed in ascending i",
                  "the key's own descriptor stands for the map point's", "the two coincide at s = 1", "the list is truncated at cap, the count is not",
                  "No atomic on any path that decides an output", "tests/reloc_sim3_search_reference.py", "a consensus below 3",
                  "in ascending query key, one entry a key", "starts with every one of those rows active", "drops the widened lists",
                  "a store that never calls it launches and holds what it did before", "a loop that never calls it ends in the same bytes"):
        assert words in text, words


def test_bindings_exist_and_the_layouts():
    for m in ("search_by_sim3", "search_by_sim3_dev"):
        assert callable(getattr(capi.Context, m)), m
    for m in ("sim3_search", "sim3_search_rc", "sim3_search_state"):
        assert callable(getattr(capi.KeyframeStore, m)), m
    assert callable(capi.VO.search_sim3_dev)
    from trackingbench_slam_amd import vo
    assert callable(vo.StereoVO.search_sim3)
    assert C.sizeof(capi.Sim3SearchOut) == 5 * C.sizeof(C.c_void_p)


def test_sizeof_the_out_block_in_c(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include "tb_capi.h"\n'
                   "static_assert(sizeof(tb_sim3_search_out) == 5 * sizeof(void*) && offsetof(tb_sim3_search_out, best_new) == 3 * sizeof(void*), "
                   "\"out\");\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
