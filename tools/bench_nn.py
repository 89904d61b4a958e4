#!/usr/bin/env python3
"""Measurement of the batched searchByNN matcher (tb_search_by_nn_batch_dev: k_lsh_nn, k_bf_finalize) at the reference's
LshIndexParams(20, 10, 2): S = 16 / 64 / 256 pairs of consecutive synth_seq frames at KITTI geometry (1241 x 376), 2000 ORB keys
each from the device extractor; the current frame is the query set, the frame before it the train set. --distinct different pairs
are rendered and repeated to fill a batch.

The yardstick is tb_search_by_bf_batch_dev on the same buffers in the same session (k_bf_nn: one exhaustive pass, every train
row's nearest query; k_bf_cross: the cross-check as a reduction over those; k_bf_finalize).
The two calls alternate, `--reps` times each after a warm-up, HIP events around every call; a process reports the median per
call. The tool starts --procs fresh processes one after the other and reports the median of their figures (and all of them).
Each process also reports, on the distinct pairs: the candidate fraction (numpy, tests/lsh_reference.py), the share of queries
whose LSH neighbour differs from the exhaustive one (tb_match_lsh against tb_match_bf without cross-check), the matches both
matchers keep after the filter (ratio 10, minTh 30), and the per-kernel split (tb_profile_*, a pass of its own).

    python tools/bench_nn.py [--sizes 16 64 256] [--distinct 8] [--reps 20] [--procs 3] [--out profiles/nn_bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from trackingbench_slam_amd import synth_seq  # noqa: E402

W, H, KEYS = 1241, 376, 2000
T, KS, PROBE, RATIO, MIN_TH = 20, 10, 2, 10.0, 30.0


def child(args):
    import torch
    import lsh_reference as lr
    from trackingbench_slam_amd import capi
    images = np.load(args.frames)["images"]            # [2 * distinct, H, W]: pair i = frames 2 i (train), 2 i + 1 (query)
    F = len(images)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)             # the context runs on a torch stream, so torch events can time its calls
    _STREAM["s"] = stream
    ctx = capi.Context(0, stream=stream.cuda_stream)
    lib = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    exr = capi.Extractor(ctx, W, H, 5, 0.8, F, KEYS)
    P = exr.results_dev()[3]
    kps = torch.zeros((F, P, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((F, P, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    n = exr.set_images_host(images)
    exr.build_pyramid(n)
    exr.orb(n, KEYS, 80.0, 30.0)
    exr.copy_results_dev(n, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), P)
    ctx.synchronize()
    exr.close()
    h = ctx.lsh(T, KS, PROBE, seed=args.seed)
    bits = h.info()[3]
    hd, hc = desc.cpu().numpy(), counts.cpu().numpy()
    D = F // 2
    # what the matcher does on the distinct pairs
    cand, differ, raw_n, nq = [], 0, 0, 0
    for i in range(D):
        d1, d2 = hd[2 * i + 1, :hc[2 * i + 1]], hd[2 * i, :hc[2 * i]]
        if i < args.cand_pairs:
            cand.append(float(lr.candidates(d1, d2, bits, PROBE).mean()))
        raw = ctx.match_lsh(h, d1, d2)
        ex = ctx.bf_match(d1, d2, crosscheck=False)
        differ += int((ex["trainIdx"][raw["queryIdx"]] != raw["trainIdx"]).sum()) + (len(d1) - len(raw))
        raw_n += len(raw); nq += len(d1)
    out = dict(keys_per_frame=round(float(hc.mean()), 1), key_pitch=int(P), candidate_fraction=round(float(np.mean(cand)), 4),
               queries=nq, queries_with_a_candidate=raw_n, share_of_queries_whose_neighbour_is_not_the_exhaustive_one=round(differ / nq, 5),
               sizes=[])
    for S in args.sizes:
        idx = torch.arange(S, device=dev) % D
        D1, D2 = desc[2 * idx + 1].contiguous(), desc[2 * idx].contiguous()
        c1, c2 = counts[2 * idx + 1].contiguous(), counts[2 * idx].contiguous()
        mo = [torch.zeros((S, P, 4), dtype=torch.int32, device=dev) for _ in range(2)]
        mc = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def nn():
            ctx.check(lib.tb_search_by_nn_batch_dev(ctx._h, h._h, S, p(D1), p(c1), p(D2), p(c2), C.c_size_t(P * 32), C.c_float(RATIO),
                                                    C.c_float(MIN_TH), p(mo[0]), P, p(mc[0])))

        def bf():
            ctx.check(lib.tb_search_by_bf_batch_dev(ctx._h, S, p(D1), p(c1), p(D2), p(c2), C.c_size_t(P * 32), C.c_float(RATIO),
                                                    C.c_float(MIN_TH), p(mo[1]), P, p(mc[1])))

        for _ in range(3):   # warm-up: code objects, scratch growth
            nn(); bf()
        ctx.synchronize()
        ms = {"nn": [], "bf": []}
        for _ in range(args.reps):
            for name, f in (("nn", nn), ("bf", bf)):
                ctx.synchronize()
                t0 = ctx_event(torch); f(); t1 = ctx_event(torch)
                ctx.synchronize()
                ms[name].append(t0.elapsed_time(t1))
        # the per-kernel split, a pass of its own
        ctx.profile_enable(True)
        for _ in range(5):
            nn(); bf()
        ctx.synchronize()
        rep = ctx.profile_report()
        ctx.profile_enable(False)
        kern = {k: round(m / c, 4) for k, (c, m) in rep.items()}
        a, b = float(np.median(ms["nn"])), float(np.median(ms["bf"]))
        out["sizes"].append(dict(S=S, nn_ms_per_call=round(a, 4), bf_ms_per_call=round(b, 4), nn_over_bf=round(a / b, 3),
                                 nn_ms_min_max=[round(min(ms["nn"]), 4), round(max(ms["nn"]), 4)],
                                 bf_ms_min_max=[round(min(ms["bf"]), 4), round(max(ms["bf"]), 4)],
                                 matches_kept_per_pair=dict(nn=round(float(mc[0].float().mean().item()), 1),
                                                            bf=round(float(mc[1].float().mean().item()), 1)),
                                 kernel_ms_per_launch=kern))
    h.close()
    ctx.close()
    print("BENCH_NN " + json.dumps(out))


_STREAM = {}


def ctx_event(torch):
    """an event recorded on the context's stream (the context was made on a torch stream of this process)"""
    e = torch.cuda.Event(enable_timing=True)
    e.record(_STREAM["s"])
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--distinct", type=int, default=8, help="different frame pairs, repeated to fill a batch")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0, help="seed of the bit table")
    ap.add_argument("--cand-pairs", type=int, default=2, help="pairs the candidate fraction is computed on (numpy, all pairs)")
    ap.add_argument("--speed", type=float, default=0.5, help="metres per frame of the synthetic sequences")
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    ap.add_argument("--frames", default=None, help=argparse.SUPPRESS)   # a child process: the rendered frames
    args = ap.parse_args()
    if args.frames:
        return child(args)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "frames.npz")
        images = np.concatenate([synth_seq.sequence(s, 2, speed=args.speed)[0] for s in range(args.distinct)])
        np.savez(path, images=images)
        runs = []
        for _ in range(args.procs):   # fresh processes, one after the other; this one never opens the GPU
            cmd = [sys.executable, os.path.abspath(__file__), "--frames", path, "--reps", str(args.reps), "--seed", str(args.seed),
                   "--cand-pairs", str(args.cand_pairs), "--sizes"] + [str(s) for s in args.sizes]
            txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
            runs.append(json.loads([l for l in txt.splitlines() if l.startswith("BENCH_NN ")][-1][len("BENCH_NN "):]))
    med = []
    for i, S in enumerate(args.sizes):
        a = float(np.median([r["sizes"][i]["nn_ms_per_call"] for r in runs]))
        b = float(np.median([r["sizes"][i]["bf_ms_per_call"] for r in runs]))
        med.append(dict(S=S, nn_ms_per_call=round(a, 4), bf_ms_per_call=round(b, 4), nn_over_bf=round(a / b, 3)))
    res = dict(tool="bench_nn", width=W, height=H, keys=KEYS, tables=T, key_size=KS, multi_probe_level=PROBE, bits_seed=args.seed,
               ratio=RATIO, min_th=MIN_TH, distinct_pairs=args.distinct, reps=args.reps, median_of_processes=med, processes=runs)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
