"""What tb_sim3_optimize_batch_dev costs: P problems of 300 pixel rows, seeded by tb_sim3_ransac_batch_dev on the same rows.

For P = 16 / 64 / 256: stereo points 5-40 m in front of camera 2 (KITTI's K, 0.5 px pixel noise, the depth noise of a 0.5 px
disparity error at a 0.54 m baseline), camera 1 a similarity away (s = 1, 0.1 rad, 1.1 m), a tenth of the rows displaced by
metres; every problem of a batch has its own draws. k_sim3 (256 hypotheses) solves the rows' 3D part; its srt and mask seed
k_sim3_opt at the default parameters. A call's figure is the library's own per-kernel profile (HIP events around the kernel):
after a warm-up call, --reps timed calls, reported as median, minimum and maximum. Beside it, in the same session, k_sim3 itself
and k_pose (tb_pose_opt_batch_dev on the rows' camera-2 points and camera-1 pixels, seeded with the true pose) on rows of the same
count. Nothing exists to compare with: the figures are the record.
Prints one JSON line and writes it to profiles/sim3_opt_bench.json (--out).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trackingbench_slam_amd import capi  # noqa: E402
from bench_sim3 import K, W, H, kernel_ms, points  # noqa: E402

BF = 0.54 * K[0]
ANGLE, DIST = 0.1, 1.1


def truth():
    a = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ANGLE) * Kx + (1 - np.cos(ANGLE)) * (Kx @ Kx)
    return R, DIST * np.array([0.6, -0.1, 0.3]) / np.linalg.norm([0.6, -0.1, 0.3])


def stereo(rng, X):
    n = len(X)
    uv = np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], -1) + rng.normal(0, 0.5, (n, 2))
    z = X[:, 2] + rng.normal(0, 0.5, n) * X[:, 2] ** 2 / BF
    return uv, np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)


def problem(seed, n, outliers):
    """(pixel rows float32 [n, 12], tb_sim3_row float32 [n, 8], tb_obs float32 [n, 6])"""
    rng = np.random.default_rng(seed)
    R, t = truth()
    X2 = points(rng, n)
    X1 = X2 @ R.T + t
    bad = rng.permutation(n)[:int(round(n * outliers))]
    X1[bad] += rng.uniform(2.0, 6.0, (len(bad), 1)) * np.array([1.0, 0.3, 0.0])
    uv1, M1 = stereo(rng, X1)
    uv2, M2 = stereo(rng, X2)
    one = np.ones((n, 1))
    return (np.concatenate([M1, M2, uv1, uv2, one, one], 1).astype(np.float32), np.concatenate([M1, M2, one, one], 1).astype(np.float32),
            np.concatenate([uv1, M2, one], 1).astype(np.float32))


def run_size(ctx, stream, P, n, outliers, hyp, reps):
    built = [problem(9000 + p, n, outliers) for p in range(P)]
    rows, rows3, obs = (torch.from_numpy(np.stack([b[k] for b in built])).cuda() for k in range(3))
    counts = torch.full((P,), n, dtype=torch.int32, device="cuda")
    S12 = torch.zeros((P, 16), dtype=torch.float32, device="cuda")
    srt0 = torch.zeros((P, 8), dtype=torch.float64, device="cuda")
    srt = torch.zeros((P, 8), dtype=torch.float64, device="cuda")
    cons = torch.zeros(P, dtype=torch.int32, device="cuda")
    inl0 = torch.zeros((P, n), dtype=torch.uint8, device="cuda")
    inl = torch.zeros((P, n), dtype=torch.uint8, device="cuda")
    win = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
    flags = torch.zeros(P, dtype=torch.int32, device="cuda")
    ninl = torch.zeros(P, dtype=torch.int32, device="cuda")
    stats = torch.zeros((P, 8), dtype=torch.float64, device="cuda")
    R, t = truth()
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    Tin = torch.from_numpy(np.tile(T.reshape(1, 16), (P, 1))).cuda()
    Tout = torch.zeros((P, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    Kd = (C.c_double * 4)(*K)
    p = lambda x: C.c_void_p(x.data_ptr())

    def sim3():
        ctx.check(ctx.sim3_ransac_dev(P, K, rows3.data_ptr(), counts.data_ptr(), n, S12.data_ptr(), srt0.data_ptr(), cons.data_ptr(),
                                      inl0.data_ptr(), win.data_ptr(), flags.data_ptr(), hypotheses=hyp, fixed_scale=True, seed=1))

    def opt():
        ctx.check(ctx.sim3_optimize_dev(P, K, rows.data_ptr(), counts.data_ptr(), n, srt0.data_ptr(), inl.data_ptr(), active_ptr=inl0.data_ptr(),
                                        srt_out_ptr=srt.data_ptr(), S12_ptr=S12.data_ptr(), inliers_ptr=ninl.data_ptr(),
                                        stats_ptr=stats.data_ptr(), fixed_scale=True))

    def pose():
        ctx.check(capi.lib().tb_pose_opt_batch_dev(ctx._h, P, Kd, p(Tin), p(obs), p(counts), n, p(inl), p(Tout), p(ninl), None))

    with torch.cuda.stream(stream):
        s_med, s_min, s_max = kernel_ms(ctx, stream, "k_sim3", sim3, reps)
        o_med, o_min, o_max = kernel_ms(ctx, stream, "k_sim3_opt", opt, reps)
        st, ni, c = stats.cpu().numpy(), ninl.cpu().numpy(), cons.cpu().numpy()
        p_med, p_min, p_max = kernel_ms(ctx, stream, "k_pose", pose, reps)
    return dict(P=P, rows=n, displaced_rows=int(round(n * outliers)), hypotheses=hyp, k_sim3_opt_ms=o_med, k_sim3_opt_ms_min=o_min,
                k_sim3_opt_ms_max=o_max, k_sim3_ms=s_med, k_sim3_ms_min=s_min, k_sim3_ms_max=s_max, k_pose_ms=p_med, k_pose_ms_min=p_min,
                k_pose_ms_max=p_max, mean_consensus=round(float(c.mean()), 1), mean_inliers=round(float(ni.mean()), 1),
                mean_iterations=round(float(st[:, 0].mean()), 2), mean_trials=round(float(st[:, 3].mean()), 2),
                mean_nbad=round(float(st[:, 4].mean()), 1), flagged=int((st[:, 7] != 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_size(ctx, stream, int(P), args.rows, args.outliers, args.hypotheses, args.reps) for P in args.sizes.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_sim3_opt", device=torch.cuda.get_device_name(0), reps=args.reps, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
