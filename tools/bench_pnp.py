"""What tb_pnp_ransac_batch_dev costs: S problems of 300 rows at 50 % outliers, 256 hypotheses each.

For S = 16 / 64 / 256: a scene 3-40 m in front of a camera (K = 360, 360, 320, 120), 0.5 px noise on the good rows, uniformly random
pixels on the others; every problem of a batch has its own draws. A call's figure is the library's own per-kernel profile (HIP
events around k_pnp), the median over --reps calls after a warm-up call. Beside it, in the same session and on the same rows,
tb_pose_opt_batch_dev (k_pose) seeded with the true pose: what the seeded path of candidate verification spends on a pair. Nothing
exists to compare with: the figures are the record. Prints one JSON line and writes it to profiles/pnp_bench.json (--out).
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

K = (360.0, 360.0, 320.0, 120.0)
W, H = 640, 240


def problem(seed, n, outliers):
    """(rows float32 [n, 6], Tcw float32 [4, 4]): n rows of a scene seen from a pose away from the identity"""
    rng = np.random.default_rng(seed)
    a, b = 0.3, -0.1
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ry @ Rx, (1.5, -0.4, 2.0)
    uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
    z = rng.uniform(3.0, 40.0, n)
    cam = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], -1)
    Xw = ((cam - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    px = uv + rng.normal(0, 0.5, (n, 2))
    bad = rng.permutation(n)[:int(round(n * outliers))]
    px[bad] = np.stack([rng.uniform(0, W, len(bad)), rng.uniform(0, H, len(bad))], -1)
    return np.concatenate([px, Xw, np.ones((n, 1))], 1).astype(np.float32), T.astype(np.float32)


def median_kernel_ms(ctx, stream, name, call, reps):
    call()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        ctx.profile_enable(True)
        call()
        stream.synchronize()
        ms.append(ctx.profile_report()[name][1])
        ctx.profile_enable(False)
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def run_size(ctx, stream, S, n, outliers, hyp, reps):
    probs = [problem(7000 + s, n, outliers) for s in range(S)]
    rows = torch.from_numpy(np.stack([p[0] for p in probs])).cuda()
    Ttrue = torch.from_numpy(np.stack([p[1] for p in probs]).reshape(S, 16)).cuda()
    counts = torch.full((S,), n, dtype=torch.int32, device="cuda")
    T = torch.zeros((S, 16), dtype=torch.float32, device="cuda")
    cons = torch.zeros(S, dtype=torch.int32, device="cuda")
    inl = torch.zeros((S, n), dtype=torch.uint8, device="cuda")
    win = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
    flags = torch.zeros(S, dtype=torch.int32, device="cuda")
    outl = torch.zeros((S, n), dtype=torch.uint8, device="cuda")
    ninl = torch.zeros(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib = capi.lib()
    Kd = np.ascontiguousarray(K, np.float64)
    p = lambda t: capi.C.c_void_p(t.data_ptr())

    def pnp():
        ctx.check(ctx.pnp_ransac_dev(S, K, rows.data_ptr(), counts.data_ptr(), n, 0, T.data_ptr(), cons.data_ptr(), inl.data_ptr(),
                                     win.data_ptr(), flags.data_ptr(), hypotheses=hyp, seed=1))

    def pose():
        outl.zero_()
        ctx.check(lib.tb_pose_opt_batch_dev(ctx._h, S, capi._p(Kd), p(Ttrue), p(rows), p(counts), n, p(outl), p(T), p(ninl), None))

    with torch.cuda.stream(stream):
        pnp_ms, pnp_min = median_kernel_ms(ctx, stream, "k_pnp", pnp, reps)
        c = cons.cpu().numpy()
        pose_ms, pose_min = median_kernel_ms(ctx, stream, "k_pose", pose, reps)
        ni = ninl.cpu().numpy()
    good = n - int(round(n * outliers))
    return dict(S=S, rows=n, good_rows=good, hypotheses=hyp, k_pnp_ms=pnp_ms, k_pnp_ms_min=pnp_min, k_pose_ms=pose_ms, k_pose_ms_min=pose_min,
                mean_consensus=round(float(c.mean()), 1), min_consensus=int(c.min()), mean_pose_inliers_from_the_true_seed=round(float(ni.mean()), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_size(ctx, stream, int(S), args.rows, args.outliers, args.hypotheses, args.reps) for S in args.sizes.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_pnp", device=torch.cuda.get_device_name(0), reps=args.reps, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
