"""What the depth filter costs a frame: S sequences x 2048 seeds at 1241 x 376.

Four rendered sequences (synth_seq, 0.5 m a frame, ground-truth poses) are tiled over S = 16 / 64 / 256; every sequence is seeded at
frame 0 with 2048 keys (the CPU oracle's ORB keys at target 2000, repeated to fill the pitch). k_df_update is timed at update 1
(fresh seeds, 0.5 m of baseline: the line from depth_min to infinity is some 50 samples) and at update 6 (after frames 1..5: the
seeds that matched have short lines, the ones that never did a line of 3 m of baseline, and many have left the image): the
seed state before the update is saved and restored before every repetition, so each repetition does the same work. A call's figure
is the library's own per-kernel profile (HIP events around the kernel): after a warm-up call, --reps timed calls, as median,
minimum and maximum. With it: the mean sample count n + 1 of the seeds that reached the search, the patch bytes that implies
(64 a sample and seed, an upper bound: samples that repeat a pixel or leave the image are not read) over the kernel time, k_df_add
with k_df_copy (a cleared filter, 2048 keys a sequence), and as the yardstick of a per-point patch kernel here k_lk_track
(tb_optical_flow_pyr_lk_batch_dev, frame 0 -> 1) on the same keys. No target exists for a kernel that did not exist: the figures
are the record. Prints one JSON line and writes it to profiles/depth_filter_bench.json (--out).
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
import oracle  # noqa: E402
from trackingbench_slam_amd import capi, synth_seq  # noqa: E402
from trackingbench_slam_amd.depth_filter import DepthFilter  # noqa: E402
from trackingbench_slam_amd.vo import _DevArray  # noqa: E402
from bench_sim3 import kernel_ms  # noqa: E402

W, H, K = 1241, 376, synth_seq.KITTI_K
PITCH = 2048
NRENDER = 4
NFRAMES = 7


def renders():
    L, G, keys = [], [], []
    for seed in range(NRENDER):
        left, _, Tcw = synth_seq.sequence(seed, NFRAMES, speed=0.5)
        levels, sf = oracle.pyramid(left[0], 5, 0.8)
        kps, _, _ = oracle.orb_extract(levels, sf, 2000, 80, 30)
        xy = np.stack([kps["x"], kps["y"]], -1).astype(np.float32).reshape(-1, 2)
        keys.append(np.resize(xy, (PITCH, 2)))
        L.append(left)
        G.append(Tcw)
    return np.stack(L, 1), np.stack(G, 1), np.stack(keys)


def run_size(S, L, G, keys, reps):
    idx = np.arange(S) % NRENDER
    df = DepthFilter(S, W, H, K, pitch=PITCH)
    ctx, stream = df.ctx, df.stream
    try:
        imgs = [torch.from_numpy(L[t][idx]).cuda() for t in range(NFRAMES)]
        poses = [torch.from_numpy(G[t][idx]).cuda() for t in range(NFRAMES)]
        kxy = torch.from_numpy(keys[idx]).cuda()
        counts = torch.full((S,), PITCH, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        out = dict(S=S, seeds=PITCH)

        def add():
            df.clear()
            df.add_keyframe(imgs[0], poses[0], kxy, counts)

        with torch.cuda.stream(stream):
            for name in ("k_df_add", "k_df_copy"):
                out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = kernel_ms(ctx, stream, name, add, reps)
            add()
            live = torch.as_tensor(_DevArray(df.df.state_dev()["seeds"], (S, PITCH, capi.DF_SEED.itemsize), "|u1"), device=df.dev)
            for t in range(1, NFRAMES):
                if t in (1, 6):
                    saved = live.clone()

                    def update():
                        live.copy_(saved)
                        df.update(imgs[t], poses[t])

                    med, lo, hi = kernel_ms(ctx, stream, "k_df_update", update, reps)
                    tr = df.trace()
                    searched = (tr["flag"] >= 0) & (tr["n"] > 0) & (tr["n"] <= df.params.max_steps)
                    samples = float((tr["n"][searched] + 1).sum())
                    out["update%d" % t] = dict(k_df_update_ms=med, k_df_update_ms_min=lo, k_df_update_ms_max=hi,
                                               flags=np.bincount(tr["flag"].reshape(-1) + 1, minlength=9).tolist(),
                                               seeds_searched=int(searched.sum()), mean_samples=round(samples / max(int(searched.sum()), 1), 1),
                                               patch_GB_per_s=round(samples * 64 / (med * 1e-3) / 1e9, 2))
                else:
                    df.update(imgs[t], poses[t])
            nxt = torch.zeros((S, PITCH, 2), dtype=torch.float32, device="cuda")
            status = torch.zeros((S, PITCH), dtype=torch.uint8, device="cuda")

            def lk():
                ctx.optical_flow_pyr_lk_batch_dev(S, imgs[0].data_ptr(), imgs[1].data_ptr(), W, H, W, W * H, kxy.data_ptr(), counts.data_ptr(), PITCH,
                                                  nxt.data_ptr(), status.data_ptr())

            out["k_lk_track_ms"], out["k_lk_track_ms_min"], out["k_lk_track_ms_max"] = kernel_ms(ctx, stream, "k_lk_track", lk, reps)
    finally:
        df.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_filter_bench.json"))
    args = ap.parse_args()
    L, G, keys = renders()
    res = [run_size(int(S), L, G, keys, args.reps) for S in args.sizes.split(",")]
    line = json.dumps(dict(tool="bench_depth_filter", device=torch.cuda.get_device_name(0), reps=args.reps, width=W, height=H,
                           flag_order=["idle", "updated", "behind", "outside", "warp", "degenerate", "no_match", "converged", "nonfinite"],
                           results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
