"""What tb_sim3_ransac_batch_dev costs: P problems of 300 rows at 50 % outliers, 256 hypotheses each.

For P = 16 / 64 / 256: points 5-40 m in front of camera 2 (KITTI's K), camera 1 a similarity away (s = 1.3, 0.3 rad, 2 m), noise of
0.05 % of the depth on every coordinate of the good rows, unrelated random points on the others; every problem of a batch has its
own draws. A call's figure is the library's own per-kernel profile (HIP events around k_sim3): after a warm-up call, --reps timed
calls, reported as median, minimum and maximum. Beside it, in the same session, tb_pnp_ransac_batch_dev (k_pnp) on 3D-2D rows of
the same count and outlier share, as tools/bench_pnp.py builds them. Nothing exists to compare with: the figures are the record.
Prints one JSON line and writes it to profiles/sim3_bench.json (--out).
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
import bench_pnp  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)
W, H = 1241, 376


def points(rng, n):
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    z = rng.uniform(5.0, 40.0, n)
    return np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)


def problem(seed, n, outliers):
    """rows float32 [n, 8]: X1 = s R X2 + t on the good rows"""
    rng = np.random.default_rng(seed)
    a = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.3) * Kx + (1 - np.cos(0.3)) * (Kx @ Kx)
    t = 2.0 * np.array([0.6, -0.1, 0.3]) / np.linalg.norm([0.6, -0.1, 0.3])
    X2 = points(rng, n)
    X1 = 1.3 * X2 @ R.T + t
    X1 = X1 + rng.normal(0, 1, (n, 3)) * (0.0005 * X1[:, 2:3])
    X2 = X2 + rng.normal(0, 1, (n, 3)) * (0.0005 * X2[:, 2:3])
    bad = rng.permutation(n)[:int(round(n * outliers))]
    X1[bad] = points(rng, len(bad))
    return np.concatenate([X1, X2, np.ones((n, 2))], 1).astype(np.float32)


def kernel_ms(ctx, stream, name, call, reps):
    """(median, min, max) of the kernel's time over reps calls after one warm-up call"""
    call()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        ctx.profile_enable(True)
        call()
        stream.synchronize()
        ms.append(ctx.profile_report()[name][1])
        ctx.profile_enable(False)
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)


def run_size(ctx, stream, P, n, outliers, hyp, reps):
    rows = torch.from_numpy(np.stack([problem(9000 + p, n, outliers) for p in range(P)])).cuda()
    obs = torch.from_numpy(np.stack([bench_pnp.problem(7000 + p, n, outliers)[0] for p in range(P)])).cuda()
    counts = torch.full((P,), n, dtype=torch.int32, device="cuda")
    S12 = torch.zeros((P, 16), dtype=torch.float32, device="cuda")
    srt = torch.zeros((P, 8), dtype=torch.float64, device="cuda")
    cons = torch.zeros(P, dtype=torch.int32, device="cuda")
    inl = torch.zeros((P, n), dtype=torch.uint8, device="cuda")
    win = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
    flags = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def sim3():
        ctx.check(ctx.sim3_ransac_dev(P, K, rows.data_ptr(), counts.data_ptr(), n, S12.data_ptr(), srt.data_ptr(), cons.data_ptr(),
                                      inl.data_ptr(), win.data_ptr(), flags.data_ptr(), hypotheses=hyp, seed=1))

    def pnp():
        ctx.check(ctx.pnp_ransac_dev(P, bench_pnp.K, obs.data_ptr(), counts.data_ptr(), n, 0, S12.data_ptr(), cons.data_ptr(), inl.data_ptr(),
                                     win.data_ptr(), flags.data_ptr(), hypotheses=hyp, seed=1))

    with torch.cuda.stream(stream):
        s_med, s_min, s_max = kernel_ms(ctx, stream, "k_sim3", sim3, reps)
        c, w, s = cons.cpu().numpy(), win.cpu().numpy(), srt.cpu().numpy()[:, 7]
        p_med, p_min, p_max = kernel_ms(ctx, stream, "k_pnp", pnp, reps)
        pc = cons.cpu().numpy()
    good = n - int(round(n * outliers))
    return dict(P=P, rows=n, good_rows=good, hypotheses=hyp, k_sim3_ms=s_med, k_sim3_ms_min=s_min, k_sim3_ms_max=s_max, k_pnp_ms=p_med,
                k_pnp_ms_min=p_min, k_pnp_ms_max=p_max, mean_consensus=round(float(c.mean()), 1), min_consensus=int(c.min()),
                refitted=int(w[:, 1].sum()), worst_scale_error=float(np.abs(s / 1.3 - 1.0).max()), pnp_mean_consensus=round(float(pc.mean()), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_size(ctx, stream, int(P), args.rows, args.outliers, args.hypotheses, args.reps) for P in args.sizes.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_sim3", device=torch.cuda.get_device_name(0), reps=args.reps, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
