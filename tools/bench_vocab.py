#!/usr/bin/env python3
"""Measurement for vocabulary training on the device (tb_vocab_train_dev, TemplatedVocabulary::create): renders synth_seq
frames, extracts ORB on the device, trains on the extractor's output without a host round trip and prints one JSON line per
(k, L) config: descriptors, nodes, words, iters_per_level, wall ms in total and per level, and the kernel split from
tb_profile_report. The per-level wall is the difference between training to depth l and to depth l - 1: the upper levels
of the two trees are the same (the random streams are keyed by level and parent rank).

    python tools/bench_vocab.py [--frames 512] [--keys 2000] [--k 10] [--levels 5 6] [--cpu-desc 64000 --cpu-levels 4]

--cpu-desc N > 0 also times the numpy restatement (tests/vocab_reference.py) on the first N descriptors at --cpu-levels."""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from trackingbench_slam_amd import synth_seq  # noqa: E402

W, H = 1241, 376


def _render(job):
    seed, frames = job
    planes = synth_seq.scene(seed)
    Tcw = synth_seq.trajectory(seed, max(frames) + 1, 0.5)
    return [synth_seq.render(planes, Tcw[f], W, H) for f in frames]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--per-seq", type=int, default=32, help="frames taken from one sequence")
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--cpu-desc", type=int, default=0)
    ap.add_argument("--cpu-levels", type=int, default=4)
    args = ap.parse_args()

    # frames first (worker processes), the GPU after: nothing GPU-side is forked
    jobs = []
    for s in range((args.frames + args.per_seq - 1) // args.per_seq):
        lo = s * args.per_seq
        for a in range(lo, min(lo + args.per_seq, args.frames), 8):
            jobs.append((s, list(range(a - lo, min(a - lo + 8, args.frames - lo, args.per_seq)))))
    t0 = time.perf_counter()
    with concurrent.futures.ProcessPoolExecutor(args.workers) as ex:
        images = np.stack([img for chunk in ex.map(_render, jobs) for img in chunk])
    t_render = time.perf_counter() - t0

    import torch
    from trackingbench_slam_amd import capi
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    F = len(images)
    batch = min(64, F)
    exr = capi.Extractor(ctx, W, H, 5, 0.8, batch, args.keys)
    cap = exr.results_dev()[3]
    kps = torch.zeros((batch, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # the context has its own stream
    t0 = time.perf_counter()
    for b in range(0, F, batch):
        n = exr.set_images_host(images[b:b + batch])
        exr.build_pyramid(n)
        exr.orb(n, args.keys, 40, 10)
        exr.copy_results_dev(n, kps.data_ptr(), desc[b].data_ptr(), counts[b:].data_ptr(), cap)
    ctx.synchronize()
    t_extract = time.perf_counter() - t0
    ndesc = int(counts.sum().item())

    def train(L, profile=False):
        if profile:
            ctx.profile_enable(True)
        t = time.perf_counter()
        h, voc, st = ctx.vocab_train_dev(desc, counts, args.k, L, max_iters=args.max_iters)
        wall = 1e3 * (time.perf_counter() - t)
        prof = ctx.profile_report() if profile else None
        if profile:
            ctx.profile_enable(False)
        ctx.vocab_destroy(h)
        return voc, st, wall, prof

    train(1)   # warm-up: code objects, allocator
    walls = {}
    for L in range(1, max(args.levels) + 1):
        walls[L] = train(L)[2]
    for L in args.levels:
        voc, st, wall, prof = train(L, profile=True)
        out = {"metric": "vocabulary training wall time (tb_vocab_train_dev)", "value": round(wall, 1), "unit": "ms", "higher_is_better": False,
               "n_gpus": 1, "data": "ORB descriptors of %d synth_seq frames (%d sequences, 0.5 m/frame), %d keys/frame" %
               (F, len({j[0] for j in jobs}), args.keys),
               "config": {"k": args.k, "L": L, "weighting": "TF_IDF", "max_iters": args.max_iters, "seed": 0},
               "descriptors": ndesc, "nodes": st["nnodes"], "words": st["nwords"], "iters_per_level": st["iters_per_level"][:L],
               "capped_nodes": st["capped_nodes"], "empty_clusters": st["empty_clusters"],
               "wall_ms_total_unprofiled": round(walls[L], 1),
               "wall_ms_per_level": [round(walls[l] - (walls[l - 1] if l > 1 else 0.0), 1) for l in range(1, L + 1)],
               "wall_ms_per_level_note": "level l = wall(train to depth l) - wall(train to depth l - 1); level 1 holds the fixed costs",
               "kernels_ms": {k: round(v[1], 3) for k, v in sorted(prof.items())},
               "kernel_calls": {k: v[0] for k, v in sorted(prof.items())},
               "render_s": round(t_render, 1), "extract_s": round(t_extract, 2)}
        print(json.dumps(out), flush=True)

    if args.cpu_desc > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import vocab_reference as vr
        hd, hc = desc.cpu().numpy(), counts.cpu().numpy()
        docs, left = [], args.cpu_desc
        for f in range(F):
            m = min(int(hc[f]), left)
            if m <= 0:
                break
            docs.append(hd[f, :m]); left -= m
        t = time.perf_counter()
        ref, rst = vr.train(docs, args.k, args.cpu_levels)
        cpu_s = time.perf_counter() - t
        D = torch.zeros((len(docs), cap, 32), dtype=torch.uint8, device=dev)
        D[:, :, :] = desc[:len(docs)]
        cn = torch.tensor([len(d) for d in docs], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        h, voc, st = ctx.vocab_train_dev(D, cn, args.k, args.cpu_levels)
        gpu_ms = 1e3 * (time.perf_counter() - t)
        ctx.vocab_destroy(h)
        same = bool(np.array_equal(voc.desc, ref.desc) and np.array_equal(voc.child_items, ref.child_items)
                    and np.array_equal(voc.weight.view(np.uint64), ref.weight.view(np.uint64)) and st == rst)
        print(json.dumps({"metric": "numpy restatement (tests/vocab_reference.py) vs device on the same descriptors", "descriptors":
                          sum(len(d) for d in docs), "config": {"k": args.k, "L": args.cpu_levels}, "numpy_restatement_s": round(cpu_s, 2),
                          "device_ms": round(gpu_ms, 1), "nodes": rst["nnodes"], "iters_per_level": rst["iters_per_level"][:args.cpu_levels],
                          "same_bits": same}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
