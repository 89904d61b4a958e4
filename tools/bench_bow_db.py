#!/usr/bin/env python3
"""Measurement for BowVector scoring and the keyframe database on the device (tb_bow_db_query_dev: k_bow_score + k_bow_db_rank;
TemplatedVocabulary::score): S queries, each against the N entries of its own sequence's ring, for S and N in 16 / 64 / 256.

The BowVectors are those of 2000-key ORB frames (synth_seq, extracted on the device) under a vocabulary trained on the device on
those frames (k = 10, L = 5 and 6, TF_IDF, L1_NORM). --frames distinct frames are rendered; ring entry (s, j) and query s cycle
through them, so every pair is a pair of real frames, most of them different. One JSON line per (L, S, N): query wall ms (mean
over --reps after a warm-up, synchronised), pairs/s, the per-kernel split from tb_profile_report, and the yardstick: the host form
tb_bow_score looped on one core over the same pairs (at most --host-pairs of them, evenly spread; the ctypes call is part of what
is timed), whose scores must equal the device's bit for bit.

    python tools/bench_bow_db.py [--frames 64] [--keys 2000] [--levels 5 6] [--sizes 16 64 256] [--reps 20] [--out FILE]"""
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
PER_SEQ = 16


def _render(job):
    seed, frames = job
    planes = synth_seq.scene(seed)
    Tcw = synth_seq.trajectory(seed, max(frames) + 1, 0.5)
    return [synth_seq.render(planes, Tcw[f], W, H) for f in frames]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--topk", type=int, default=4)
    ap.add_argument("--host-pairs", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the lines to this JSON file (a list)")
    args = ap.parse_args()

    # frames first (worker processes), the GPU after: nothing GPU-side is forked
    jobs = [(s, list(range(min(PER_SEQ, args.frames - s * PER_SEQ)))) for s in range((args.frames + PER_SEQ - 1) // PER_SEQ)]
    with concurrent.futures.ProcessPoolExecutor(args.workers) as ex:
        images = np.stack([img for chunk in ex.map(_render, jobs) for img in chunk])

    import ctypes as C
    import torch
    from trackingbench_slam_amd import capi
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    F = len(images)
    batch = min(64, F)
    exr = capi.Extractor(ctx, W, H, 5, 0.8, batch, args.keys)
    P = exr.results_dev()[3]
    kps = torch.zeros((batch, P, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((F, P, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # the context has its own stream
    for b in range(0, F, batch):
        n = exr.set_images_host(images[b:b + batch])
        exr.build_pyramid(n)
        exr.orb(n, args.keys, 40, 10)
        exr.copy_results_dev(n, kps.data_ptr(), desc[b].data_ptr(), counts[b:].data_ptr(), P)
    ctx.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = []
    for L in args.levels:
        h, voc, st = ctx.vocab_train_dev(desc, counts, args.k, L, weighting=0, scoring=0)
        wid = torch.zeros((F, P), dtype=torch.int32, device=dev); wt = torch.zeros((F, P), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.check(capi.lib().tb_bow_transform_batch_dev(ctx._h, h, F, p(desc), p(counts), P, 4, p(wid), None, p(wt), None, None))
        bw, bv, bc = ctx.bow_vector_batch_dev(h, wid, wt, counts)
        ctx.synchronize()
        hw, hv, hc = bw.cpu().numpy(), bv.cpu().numpy(), bc.cpu().numpy()
        for S in args.sizes:
            for N in args.sizes:
                entry = (np.arange(S)[:, None] * 7 + np.arange(N)[None, :]) % F          # frame of ring entry (s, j)
                query = (np.arange(S) * 13 + 5) % F
                db = capi.BowDatabase(ctx, S, N, P, 0)
                for j in range(N):
                    idx = torch.from_numpy(entry[:, j]).to(dev)
                    ew, ev, ec = bw[idx].contiguous(), bv[idx].contiguous(), bc[idx].contiguous()
                    torch.cuda.synchronize()
                    db.add(ew, ev, ec, j)
                    ctx.synchronize()
                qi = torch.from_numpy(query).to(dev)
                qw, qv, qc = bw[qi].contiguous(), bv[qi].contiguous(), bc[qi].contiguous()
                torch.cuda.synchronize()
                for _ in range(3):
                    out = db.query(qw, qv, qc, topk=min(args.topk, N), exclude_newest=0)
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    out = db.query(qw, qv, qc, topk=min(args.topk, N), exclude_newest=0)
                ctx.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / args.reps
                ctx.profile_enable(True)
                for _ in range(args.reps):
                    db.query(qw, qv, qc, topk=min(args.topk, N), exclude_newest=0)
                ctx.synchronize()
                prof = ctx.profile_report()
                ctx.profile_enable(False)
                scores = out["scores"].cpu().numpy()
                # the yardstick: the host form on one core over the same pairs
                pairs = [(s, j) for s in range(S) for j in range(N)]
                pairs = pairs[::max(1, len(pairs) // args.host_pairs)][:args.host_pairs]
                vec = lambda f: (hw[f, :hc[f]], hv[f, :hc[f]])
                ins = [(vec(query[s]), vec(entry[s, j])) for s, j in pairs]
                t0 = time.perf_counter()
                host = [capi.bow_score(0, a[0], a[1], b[0], b[1]) for a, b in ins]
                host_s = time.perf_counter() - t0
                same = all(np.float64(x).view(np.uint64) == scores[s, j].view(np.uint64) for x, (s, j) in zip(host, pairs))
                line = {"metric": "keyframe database query wall time (tb_bow_db_query_dev)", "value": round(ms, 4), "unit": "ms",
                        "higher_is_better": False, "n_gpus": 1,
                        "data": "BowVectors of %d synth_seq frames, %d keys/frame, cycled through the rings" % (F, args.keys),
                        "config": {"k": args.k, "L": L, "weighting": "TF_IDF", "scoring": "L1_NORM", "S": S, "N": N, "pitch": P,
                                   "topk": min(args.topk, N), "reps": args.reps},
                        "vocabulary_words": st["nwords"], "mean_words_per_vector": round(float(hc.mean()), 1),
                        "pairs": S * N, "pairs_per_s": round(S * N / (ms * 1e-3), 1),
                        "kernels_ms_per_query": {k: round(v[1] / args.reps, 4) for k, v in sorted(prof.items())},
                        "host_one_core": {"pairs": len(pairs), "pairs_per_s": round(len(pairs) / host_s, 1), "same_bits_as_device": bool(same)}}
                print(json.dumps(line), flush=True)
                lines.append(line)
                db.close()
        ctx.vocab_destroy(h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
