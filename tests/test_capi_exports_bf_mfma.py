"""CPU tests: the library declares, binds and exports the searchByBF test hook, and the matrix-core nearest-neighbour kernel is
in the built gfx950 code object."""
import os
import re
import subprocess

from trackingbench_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_hook_and_carries_the_kernel():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    s = "tb_debug_bf_scalar"
    assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s)
    blob = open(libpath, "rb").read()
    assert b"k_bf_nn_mfma" in blob and b"gfx950" in blob
    # the scalar kernel stays: fallback and yardstick
    assert re.search(rb"_Z7k_bf_nnPK", blob)


def test_header_declares_it_beside_the_other_hooks():
    text = open(os.path.join(ROOT, "include", "tb_capi.h")).read()
    assert re.search(r"\bint tb_debug_bf_scalar\(tb_ctx\* ctx, int on\);", text)
    assert text.index("tb_debug_force_dense_fast(") < text.index("tb_debug_bf_scalar(") < text.index("tb_profile_report(")


def test_binding_and_null_context():
    assert callable(capi.Context.bf_scalar)
    assert capi.lib().tb_debug_bf_scalar(None, 1) == capi.TB_EINVAL
    assert capi.lib().tb_debug_bf_scalar(None, 0) == capi.TB_EINVAL
