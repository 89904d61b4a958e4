"""CPU tests: the library declares, binds and exports the BowVector scoring entry points, the keyframe database and its hooks in
the VO loop, and the scoring kernels are in the built code object."""
import os
import re
import subprocess

from trackingbench_slam_amd import capi

NEW = ("tb_bow_score", "tb_bow_score_batch_dev", "tb_bow_db_create", "tb_bow_db_destroy", "tb_bow_db_clear", "tb_bow_db_add_dev",
       "tb_bow_db_query_dev", "tb_bow_db_state_dev", "tb_vo_bow_db_enable", "tb_vo_bow_db_get")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tb_capi.h")


def test_library_exports_the_scoring_and_database_entry_points():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    blob = open(libpath, "rb").read()
    for k in (b"k_bow_score", b"k_bow_db_add", b"k_bow_db_rank"):
        assert k in blob, k


def test_header_declares_them_and_cites_the_reference():
    text = open(HEADER).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, text), s
    assert "ScoringObject.cpp:23-311" in text and "TemplatedVocabulary.h:156-162" in text
    assert "stays outside this library" not in text
    assert (capi.TB_SCORE_PAIRWISE, capi.TB_SCORE_ALL_PAIRS) == (0, 1)
    assert re.search(r"TB_SCORE_PAIRWISE = 0, TB_SCORE_ALL_PAIRS = 1", text)


def test_bindings_exist():
    for m in ("bow_score", "bow_score_batch_dev"):
        assert callable(getattr(capi.Context, m))
    for m in ("add", "query", "clear", "state", "close"):
        assert callable(getattr(capi.BowDatabase, m))
    for m in ("bow_db_enable", "bow_db"):
        assert callable(getattr(capi.VO, m))
    assert capi.bow_score(5, [1, 2], [0.5, 2.0], [2, 3], [4.0, 1.0]) == 8.0
