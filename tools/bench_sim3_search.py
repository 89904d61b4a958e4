"""What tb_search_by_sim3_batch_dev costs: P pairs of 2000-key frames at 1241 x 376.

For P = 16 / 64 / 256: 2000 scene points 5-40 m in front of camera 2 (KITTI's K, 8 levels at 0.8), camera 1 a rigid motion away
(s = 1, 0.1 rad, 1.1 m); both frames carry a key for every point (0.5 px pixel noise, the octave following the distance, a few bits
of descriptor noise), nine keys in ten have a point and three in ten are matched already; every pair of a batch has its own draws.
A call's figure is the time between two HIP events on the context's stream around the whole call (both launches: k_sim3_search and
k_sim3_search_agree): one warm-up call, then --reps timed calls, reported as median, minimum and maximum; the library's own
per-kernel profile of one more call splits it. Beside it, in the same session and on the same frames, the nearest existing kernel:
tb_search_by_projection_batch_dev (frame 2's points projected into frame 1 through the same motion, its lookup grids built
beforehand and not timed). Nothing exists to compare with: the figures are the record.
Prints one JSON line and writes it to profiles/sim3_search_bench.json (--out).
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
from trackingbench_slam_amd.projection import BatchedProjection  # noqa: E402
from bench_sim3 import K, W, H, points  # noqa: E402

NLEVELS, SCALE = 8, 0.8
ANGLE, DIST = 0.1, 1.1


def motion():
    a = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ANGLE) * Kx + (1 - np.cos(ANGLE)) * (Kx @ Kx)
    return R, DIST * np.array([0.6, -0.1, 0.3]) / np.linalg.norm([0.6, -0.1, 0.3])


def srt_of(R, t):
    w = np.sqrt(1.0 + np.trace(R)) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return np.concatenate([q / np.linalg.norm(q), t, [1.0]])


def frames(seed, n):
    """one pair: per side (KEYPOINT [n], desc [n][32], camera points float32 [n][3], valid [n], matched [n])"""
    rng = np.random.default_rng(seed)
    R, t = motion()
    X2 = points(rng, n)
    X1 = X2 @ R.T + t
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    o1 = rng.integers(0, NLEVELS, n)
    o2 = np.clip(np.round(o1 + np.log(np.linalg.norm(X1, axis=1) / np.linalg.norm(X2, axis=1)) / np.log(1.0 / SCALE)), 0, NLEVELS - 1)
    out = []
    for X, octv in ((X1, o1), (X2, o2)):
        order = rng.permutation(n)
        Xs = X[order]
        keys = np.zeros(n, capi.KEYPOINT)
        u, v = K[0] * Xs[:, 0] / Xs[:, 2] + K[2], K[1] * Xs[:, 1] / Xs[:, 2] + K[3]
        inside = (Xs[:, 2] > 0.5) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        keys["x"] = np.where(inside, u + rng.normal(0, 0.5, n), rng.uniform(0, W, n))
        keys["y"] = np.where(inside, v + rng.normal(0, 0.5, n), rng.uniform(0, H, n))
        keys["octave"], keys["size"], keys["class_id"] = octv[order], 31.0, -1
        bits = np.unpackbits(base[order], axis=1)
        desc = np.packbits(bits ^ (rng.integers(0, 256, bits.shape) < 4).astype(np.uint8), axis=1)
        out.append((keys, desc, Xs.astype(np.float32), (inside & (rng.uniform(0, 1, n) < 0.9)).astype(np.uint8),
                    (rng.uniform(0, 1, n) < 0.3).astype(np.uint8)))
    return out


def event_ms(stream, call, reps):
    """(median, min, max) of the time between two events around call() over reps calls after one warm-up call"""
    call()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)


def run_size(ctx, stream, P, n, reps):
    built = [frames(9000 + p, n) for p in range(P)]
    R, t = motion()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype == capi.KEYPOINT else np.ascontiguousarray(a)).cuda()
    sides = []
    for k in range(2):
        ts = [dev(np.stack([b[k][j] for b in built])) for j in range(5)]
        sides.append(tuple(x.data_ptr() for x in ts) + (torch.full((P,), n, dtype=torch.int32, device="cuda"),) + (ts,))
    srt = torch.from_numpy(np.tile(srt_of(R, t), (P, 1))).cuda()
    i32 = lambda *sh: torch.zeros(sh, dtype=torch.int32, device="cuda")
    m1, m2, pr, pc, st = i32(P, n), i32(P, n), i32(P, n, 4), i32(P), i32(P, 8)
    s1 = sides[0][:5] + (sides[0][5].data_ptr(), n)
    s2 = sides[1][:5] + (sides[1][5].data_ptr(), n)

    def search():
        ctx.check(ctx.search_by_sim3_dev(P, K, W, H, NLEVELS, SCALE, s1, s2, srt.data_ptr(), 7.5, 100, m1.data_ptr(), m2.data_ptr(), pr.data_ptr(), n,
                                         pc.data_ptr(), st.data_ptr()))

    # the nearest existing kernel on the same frames: frame 2's points into frame 1
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    cam = np.zeros(1, capi.CAMERA)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"] = K[0], K[1], K[2], K[3], W, H
    sf = capi.scale_factors(NLEVELS, SCALE)[0]
    cases = []
    for (k1, d1, _, _, mt1), (k2, d2, X2, v2, _) in built:
        mp = np.zeros(n, capi.MAPPOINT)
        mp["pos"], mp["bad"] = X2, 1 - v2.astype(np.int32)
        cases.append(dict(cam=cam, width=W, height=H, sf=sf, k1=k1, d1=d1, taken1=mt1, k2=k2, mp=mp, mp_desc=d2, Tcw=T))
    bp = BatchedProjection(ctx, cases, nratio=7.5, th_high=100)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        bp.build_grids()
        s_med, s_min, s_max = event_ms(stream, search, reps)
        stats, found = st.cpu().numpy(), pc.cpu().numpy()
        ctx.profile_enable(True)
        search()
        stream.synchronize()
        prof = ctx.profile_report()
        ctx.profile_enable(False)
        p_med, p_min, p_max = event_ms(stream, bp.search, reps)
        pfound = bp.out_counts.cpu().numpy()
    return dict(P=P, keys=n, search_by_sim3_ms=s_med, search_by_sim3_ms_min=s_min, search_by_sim3_ms_max=s_max,
                k_sim3_search_ms=round(float(prof["k_sim3_search"][1]), 4), k_sim3_search_agree_ms=round(float(prof["k_sim3_search_agree"][1]), 4),
                search_by_projection_ms=p_med, search_by_projection_ms_min=p_min, search_by_projection_ms_max=p_max,
                mean_tried=round(float(stats[:, [0, 2]].mean()), 1), mean_searched=round(float(stats[:, [1, 3]].mean()), 1),
                mean_accepted=round(float(stats[:, [4, 5]].mean()), 1), mean_new_pairs=round(float(found.mean()), 1),
                flagged=int((stats[:, 7] != 0).sum()), projection_mean_matches=round(float(pfound.mean()), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_search_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    try:
        res = [run_size(ctx, stream, int(P), args.keys, args.reps) for P in args.sizes.split(",")]
    finally:
        ctx.close()
    line = json.dumps(dict(tool="bench_sim3_search", device=torch.cuda.get_device_name(0), width=W, height=H, nlevels=NLEVELS, reps=args.reps,
                           results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
