"""What tb_pose_graph_sim3_batch_dev costs, beside tb_pose_graph_batch_dev on the same graphs in the same session.

The graphs are tools/bench_pose_graph.py's (imported from it): G = 16 / 64 / 256 graphs of 16 / 32 / 64 nodes, a drifted circuit
closed by 1 and by 4 exact chords, every graph of a batch with its own noise. The Sim(3) solver gets them as srt nodes and edges
with s = 1 (capi.sim3_from_matrix of the same float32 poses and float64 motions), once with the scale free (7 unknowns a node)
and once held (6); k_pgo's column is the yardstick, no ratio is promised: both kernels are latency bound by design and neither is
tuned. A call's figure is the median over --reps of HIP events on the context's stream around one call (the nodes are restored
before each call, outside the timed span). Prints one JSON line and writes it to profiles/pose_graph_sim3_bench.json (--out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trackingbench_slam_amd import capi  # noqa: E402
import bench_pose_graph as se3  # noqa: E402


def timed_calls(stream, restore, launch, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(timed):
        with torch.cuda.stream(stream):
            restore()
            if timed:
                a.record(stream)
            launch()
            if timed:
                b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) if timed else 0.0

    call(False)                                   # sizes the context's work buffer
    ms = [call(True) for _ in range(reps)]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def summary(stats, ms):
    st = stats.cpu().numpy()
    return dict(ms_per_call=ms[0], ms_min=ms[1], mean_iterations=round(float(st[:, 0].mean()), 2), mean_trials=round(float(st[:, 4].mean()), 2),
                chi2_before=float(st[:, 1].mean()), chi2_after=float(st[:, 2].mean()), flagged=int((st[:, 7] < 0).sum()))


def run_shape(ctx, stream, G, n, nchords, iters, reps, distinct):
    probs = [se3.graph(1000 * n + 10 * nchords + i, n, nchords) for i in range(min(distinct, G))]
    pitch = len(probs[0][1])
    counts = torch.full((G,), pitch, dtype=torch.int32, device="cuda")
    stats = torch.zeros((G, 8), dtype=torch.float64, device="cuda")
    # SE(3): k_pgo
    poses0 = torch.from_numpy(np.stack([probs[g % len(probs)][0] for g in range(G)])).cuda()
    edges6 = torch.from_numpy(np.stack([probs[g % len(probs)][1] for g in range(G)]).view(np.uint8).reshape(G, -1)).cuda()
    poses = torch.empty_like(poses0)
    out = dict(G=G, nnodes=n, chords=nchords, edges=pitch)
    ms = timed_calls(stream, lambda: poses.copy_(poses0), lambda: ctx.check(ctx.pose_graph_dev(
        G, n, 1, poses.data_ptr(), edges6.data_ptr(), counts.data_ptr(), pitch, iters, stats.data_ptr())), reps)
    out["se3"] = summary(stats, ms)
    # Sim(3): the same graphs, every scale 1
    sim = []
    for p0, e6 in probs:
        e = np.zeros(len(e6), capi.PG_SIM3_EDGE)
        e["a"], e["b"], e["w_rot"], e["w_trans"], e["w_scale"] = e6["a"], e6["b"], e6["w_rot"], e6["w_trans"], 1.0
        e["srt"][:, 0], e["srt"][:, 1:4], e["srt"][:, 4:7], e["srt"][:, 7] = e6["q"][:, 3], e6["q"][:, :3], e6["t"], 1.0
        n0 = capi.sim3_from_matrix(p0.astype(np.float64))
        n0[:, 7] = 1.0      # a float32 rotation's determinant is 1 only to 1e-7
        sim.append((n0, e))
    nodes0 = torch.from_numpy(np.stack([sim[g % len(sim)][0] for g in range(G)])).cuda()
    edges7 = torch.from_numpy(np.stack([sim[g % len(sim)][1] for g in range(G)]).view(np.uint8).reshape(G, -1)).cuda()
    nodes = torch.empty_like(nodes0)
    for name, fs in (("sim3_free", False), ("sim3_held", True)):
        ms = timed_calls(stream, lambda: nodes.copy_(nodes0), lambda: ctx.check(ctx.pose_graph_sim3_dev(
            G, n, 1, nodes.data_ptr(), edges7.data_ptr(), counts.data_ptr(), pitch, iters, stats.data_ptr(), fixed_scale=fs)), reps)
        out[name] = summary(stats, ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="16,64,256")
    ap.add_argument("--nodes", default="16,32,64")
    ap.add_argument("--chords", default="1,4")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="different graphs, repeated to fill a batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_sim3_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_shape(ctx, stream, int(G), int(n), int(c), args.iters, args.reps, args.distinct)
               for n in args.nodes.split(",") for c in args.chords.split(",") for G in args.graphs.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_pose_graph_sim3", device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps,
                           distinct_graphs=args.distinct, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
