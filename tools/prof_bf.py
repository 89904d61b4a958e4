#!/usr/bin/env python3
"""searchByBF alone on the GPU: `reps` calls of tb_search_by_bf_batch_dev on S pairs of n x n random descriptors at key pitch P,
then the per-kernel split (tb_profile_*). The subject of the counter passes of tools/rocprof_pmc.sh on the matcher.

    python tools/prof_bf.py [S=512] [reps=4] [n=2000] [P=2241] [scalar=0]

scalar=1 runs the scalar nearest-neighbour kernel (tb_debug_bf_scalar)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from trackingbench_slam_amd import capi
    a = [int(x) for x in sys.argv[1:]]
    S, reps, n, P, scalar = (a + [512, 4, 2000, 2241, 0][len(a):])[:5]
    ctx = capi.Context(0)
    lib = capi.lib()
    if scalar:
        ctx.bf_scalar(True)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    D1 = torch.randint(0, 256, (S, P, 32), dtype=torch.uint8, device="cuda", generator=g)
    D2 = torch.randint(0, 256, (S, P, 32), dtype=torch.uint8, device="cuda", generator=g)
    c1 = torch.full((S,), n, dtype=torch.int32, device="cuda")
    c2 = c1.clone()
    mo = torch.zeros((S, P, 4), dtype=torch.int32, device="cuda")
    mc = torch.zeros(S, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def bf():
        ctx.check(lib.tb_search_by_bf_batch_dev(ctx._h, S, p(D1), p(c1), p(D2), p(c2), C.c_size_t(P * 32), C.c_float(10.0),
                                                C.c_float(30.0), p(mo), P, p(mc)))

    bf()
    ctx.synchronize()
    ctx.profile_enable(True)
    for _ in range(reps):
        bf()
    ctx.synchronize()
    for k, (c, m) in sorted(ctx.profile_report().items()):
        print("%-16s %4d launches %10.4f ms / launch" % (k, c, m / c))
    print("%d pairs of %d x %d at pitch %d, matches kept per pair %.1f" % (S, n, n, P, float(mc.float().mean().item())))
    ctx.close()


if __name__ == "__main__":
    main()
