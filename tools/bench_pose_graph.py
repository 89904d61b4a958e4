"""What tb_pose_graph_batch_dev costs: G graphs of one shape, a drifted chain closed by chords, `--iters` LM iterations.

For G = 16 / 64 / 256 graphs of 16 / 32 / 64 nodes, chain plus 1 and plus 4 chords: odometry edges with noise, integrated from
node 0 (so the start is the drifted trajectory), exact chords; every graph of a batch has its own noise. A call's figure is the
median over --reps of HIP events on the context's stream around one call (the poses are restored before each call, outside the
timed span); the per-kernel split is the library's own profile of one more call -- the operator is one kernel, k_pgo, so the
difference is launch and event overhead. The mean iterations and trials per graph say how much LM work the time bought. Nothing
exists to compare with: the figures are the record. Prints one JSON line and writes it to profiles/pose_graph_bench.json (--out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trackingbench_slam_amd import capi  # noqa: E402


# The circuit generator needs SE(3)'s exp and inverse on the host; the package has none (its SE(3) arithmetic is device code) and a
# tool cannot import the tests' reference, so the two are restated here. Quaternions come from capi.pose_graph_edges.
def se3_exp(u):
    w, v = np.asarray(u[:3], np.float64), np.asarray(u[3:], np.float64)
    th = float(np.sqrt((w * w).sum()))
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a, b, d = (1.0, 0.5, 1.0 / 6) if th < 1e-5 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Om + b * (Om @ Om)
    T[:3, 3] = (np.eye(3) + b * Om + d * (Om @ Om)) @ v
    return T


def se3_inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def graph(seed, n, nchords):
    """(poses0 float32 [n, 4, 4], edges): a circuit of n cameras, noisy odometry integrated from node 0, exact chords"""
    rng = np.random.default_rng(seed)
    truth = []
    for i in range(n):
        ang = 2 * np.pi * i / n
        Twc = np.eye(4)
        Twc[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
        Twc[:3, 3] = (10 * np.sin(ang), 0.0, 10 * (1 - np.cos(ang)))
        truth.append(se3_inv(Twc))
    pairs, Z, est = [], [], [truth[0]]
    for i in range(n - 1):
        z = se3_exp(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.02, 3)])) @ truth[i + 1] @ se3_inv(truth[i])
        pairs.append((i, i + 1)); Z.append(z); est.append(z @ est[-1])
    for c in range(nchords):
        a, b = (c * (n // 2)) // max(nchords, 1), n - 1 - c
        pairs.append((a, b)); Z.append(truth[b] @ se3_inv(truth[a]))
    poses0 = np.stack(est).astype(np.float32)
    poses0[:, 3] = (0, 0, 0, 1)
    return poses0, capi.pose_graph_edges(pairs, np.stack(Z))


def run_shape(ctx, stream, G, n, nchords, iters, reps, distinct):
    probs = [graph(1000 * n + 10 * nchords + i, n, nchords) for i in range(min(distinct, G))]
    pitch = len(probs[0][1])
    poses0 = torch.from_numpy(np.stack([probs[g % len(probs)][0] for g in range(G)])).cuda()
    edges = torch.from_numpy(np.stack([probs[g % len(probs)][1] for g in range(G)]).view(np.uint8).reshape(G, -1)).cuda()
    counts = torch.full((G,), pitch, dtype=torch.int32, device="cuda")
    poses = torch.empty_like(poses0)
    stats = torch.zeros((G, 8), dtype=torch.float64, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(timed):
        with torch.cuda.stream(stream):
            poses.copy_(poses0)
            if timed:
                a.record(stream)
            ctx.check(ctx.pose_graph_dev(G, n, 1, poses.data_ptr(), edges.data_ptr(), counts.data_ptr(), pitch, iters, stats.data_ptr()))
            if timed:
                b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) if timed else 0.0

    call(False)                                   # sizes the context's work buffer
    ms = [call(True) for _ in range(reps)]
    ctx.profile_enable(True)
    call(False)
    kern = {k: dict(calls=v[0], ms=round(v[1], 4)) for k, v in ctx.profile_report().items()}
    ctx.profile_enable(False)
    st = stats.cpu().numpy()
    return dict(G=G, nnodes=n, chords=nchords, edges=pitch, ms_per_call=round(float(np.median(ms)), 4),
                ms_min=round(float(min(ms)), 4), kernels=kern, mean_iterations=round(float(st[:, 0].mean()), 2),
                mean_trials=round(float(st[:, 4].mean()), 2), chi2_before=float(st[:, 1].mean()), chi2_after=float(st[:, 2].mean()),
                flagged=int((st[:, 7] < 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="16,64,256")
    ap.add_argument("--nodes", default="16,32,64")
    ap.add_argument("--chords", default="1,4")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="different graphs, repeated to fill a batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_shape(ctx, stream, int(G), int(n), int(c), args.iters, args.reps, args.distinct)
               for n in args.nodes.split(",") for c in args.chords.split(",") for G in args.graphs.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_pose_graph", device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps,
                           distinct_graphs=args.distinct, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
