"""CPU tests: the C-ABI library builds for gfx950, loads, and exports every symbol include/tb_capi.h
declares; host-only entry points (no GPU needed) agree with the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    return capi.build()


def test_header_and_binding_list_the_same_symbols():
    hdr = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tb_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS), declared ^ set(capi.EXPORTS)


def test_library_exports_every_declared_symbol(libpath):
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    missing = [s for s in capi.EXPORTS if s not in syms]
    assert not missing, missing
    L = capi.lib()
    for s in capi.EXPORTS:
        assert hasattr(L, s)
    assert b"gfx950" in L.tb_version()


def test_library_contains_gfx950_code_object(libpath):
    data = open(libpath, "rb").read()
    assert b"gfx950" in data
    assert b"k_fast_cells" in data and b"k_octree" in data and b"k_describe" in data


def test_product_does_not_reference_the_oracle():
    pkg = os.path.join(ROOT, "trackingbench_slam_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in txt and "liboracle" not in txt and "oracle/" not in txt, f


def test_host_only_entry_points_match_oracle(libpath):
    for n, s in ((5, 0.8), (8, 0.8), (4, 0.5), (5, 0.6), (1, 0.8)):
        got = capi.scale_factors(n, s)
        exp = oracle.scale_factors(n, s)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        if n >= 2:
            for target in (1000, 2000, 8000, 37):
                assert np.array_equal(capi.orb_quotas(got[0], target), oracle.orb_quotas(exp[0], target))
        for w, h in ((1241, 376), (1280, 720), (640, 480), (3840, 2160)):
            assert all(np.array_equal(a, b) for a, b in zip(capi.pyramid_sizes(w, h, got[0]), oracle.pyramid_sizes(w, h, exp[0])))
    with pytest.raises(capi.TBError):
        capi.orb_quotas(np.ones(1, np.float32), 100)
    rng = np.random.default_rng(0)
    for _ in range(50):
        a = rng.integers(0, 256, 32, dtype=np.uint8); b = rng.integers(0, 256, 32, dtype=np.uint8)
        assert capi.descriptor_distance(a, b) == oracle.descriptor_distance(a, b)
    # the second row: ties (first index wins), a second / third bin at and just below a tenth of the first, lengths 1 and 1024
    for sizes in ([0, 5, 9, 2, 7], [100, 5, 9], [100, 50, 9], [0, 0, 0], list(rng.integers(0, 50, 30)),
                  [7, 7, 7], [0, 3, 3, 3], [10, 1, 1], [11, 1, 0], [10, 5, 0], [4], list(rng.integers(0, 50, 1024))):
        assert capi.three_maxima(sizes) == oracle.three_maxima(sizes)


def test_no_gpu_means_loud_failure(libpath):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.TBError):
        capi.Context(0)
