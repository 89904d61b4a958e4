"""What the window BA costs the optical-flow VO loop, and what it does to the drift (trackingbench_slam_amd.vo.StereoVO,
window_ba=...).

For every batch size S (tools/bench_vo.py's sizes: 1241 x 376, 2000 keys, keyframe_every 10): the loop over T frames of synthetic
stereo sequences (synth_seq, uploaded before anything is timed) with the feature off and with it on. Both use the same library in
the same session: the tool starts --procs fresh processes per mode, alternating off / on, and a mode's figure is the median over
its processes of that process's median over --reps runs. The yardstick is the off run (and the parent commit's loop, which it
is, launch for launch), never the on run. Per step kind -- tracking steps, keyframe steps t > 0 (the ones that carry a window)
and frame 0 -- the mean step time from HIP events on the loop's stream, host gaps included (the BA's termination test
synchronises once per keyframe step). The on run also reports, from the per-kernel timers, the share of the three segment
kernels (and the segment start) and of the BA call's kernels in the run, and both modes report the drift against ground truth at
the last frame and its maximum over the run, per distinct sequence. No throughput target is set for a step that did not exist:
the tool records what is measured. Prints one JSON line and writes it to profiles/vo_window_bench.json (--out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG_KERNELS = ("k_vo_seg_start", "k_vo_seg_log", "k_vo_seg_window", "k_vo_seg_adopt")


def centre(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return -T[:3, :3].T @ T[:3, 3]


def child(args):
    import torch
    from trackingbench_slam_amd import synth_seq
    from trackingbench_slam_amd.vo import StereoVO
    S, T, every, on = args.child_size, args.steps, args.keyframe_every, args.child == "on"
    seqs = [synth_seq.sequence(s, T, speed=args.speed) for s in range(args.distinct)]
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    G0 = rep(G)[0]
    vo = StereoVO(S, keyframe_every=every, window_ba=True if on else None)
    kf = np.array([t % every == 0 for t in range(T)])
    kfw = kf & (np.arange(T) > 0)

    def run(poses=None):
        vo.reset(G0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(T + 1)]
        torch.cuda.synchronize()
        for t in range(T):
            ev[t].record(vo.stream)
            vo.step(dL[t], dR[t] if kf[t] else None)
            if poses is not None:
                poses.append(vo.Tcw()[:D].cpu().numpy())
        ev[T].record(vo.stream)
        torch.cuda.synchronize()
        return np.array([ev[t].elapsed_time(ev[t + 1]) for t in range(T)])

    try:
        run()                                   # sizes every buffer, captures the BA's graph
        ms = np.stack([run() for _ in range(args.reps)])
        poses = []
        run(poses)
        out = dict(mode=args.child, S=S, ms_per_track_step=float(np.median(ms[:, ~kf].mean(1))),
                   ms_per_keyframe_step=float(np.median(ms[:, kfw].mean(1))) if kfw.any() else None,
                   ms_frame0=float(np.median(ms[:, 0])), ms_per_step=float(np.median(ms.mean(1))))
        drift = np.array([[np.linalg.norm(centre(poses[t][s]) - centre(G[t, s])) for t in range(T)] for s in range(D)])
        out["drift_last_frame_m"] = [round(float(x), 4) for x in drift[:, -1]]
        out["drift_max_m"] = [round(float(x), 4) for x in drift.max(1)]
        if on:
            out["adopted_last_window"] = int(vo.window()["adopted"].sum().item())
            vo.reset(G0)
            torch.cuda.synchronize()
            vo.profile_enable(True)
            for t in range(T):
                vo.step(dL[t], dR[t] if kf[t] else None)
            rp = vo.profile_report()
            vo.profile_enable(False)
            total = sum(v[1] for v in rp.values())
            seg = sum(rp[k][1] for k in SEG_KERNELS if k in rp)
            ba = sum(v[1] for k, v in rp.items() if k.startswith("k_ba_"))
            out["kernel_ms_over_T_steps"] = dict(all=round(total, 3), segment_kernels=round(seg, 4), ba_call=round(ba, 3))
            out["segment_kernels_share_percent"] = round(100.0 * seg / total, 3)
            out["ba_call_share_percent"] = round(100.0 * ba / total, 2)
            out["segment_kernels"] = {k: dict(calls=rp[k][0], ms=round(rp[k][1], 4)) for k in SEG_KERNELS if k in rp}
    finally:
        vo.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=3, help="fresh processes per mode and size, alternated off / on")
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic sequences, repeated to fill a batch")
    ap.add_argument("--keyframe-every", type=int, default=10)
    ap.add_argument("--speed", type=float, default=0.5, help="metres per frame of the synthetic sequences")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_window_bench.json"))
    ap.add_argument("--child", choices=("off", "on"), help=argparse.SUPPRESS)
    ap.add_argument("--child-size", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for S in [int(x) for x in args.sizes.split(",")]:
        runs = {"off": [], "on": []}
        for _ in range(args.procs):
            for mode in ("off", "on"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-size", str(S), "--steps", str(args.steps),
                       "--reps", str(args.reps), "--distinct", str(args.distinct), "--keyframe-every", str(args.keyframe_every),
                       "--speed", str(args.speed)]
                txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
                runs[mode].append(json.loads([l for l in txt.splitlines() if l.startswith("RESULT ")][-1][7:]))
                print("S = %d %s: %.3f ms per step" % (S, mode, runs[mode][-1]["ms_per_step"]), file=sys.stderr, flush=True)
        r = dict(S=S, T=args.steps)
        for mode in ("off", "on"):
            for k in ("ms_per_track_step", "ms_per_keyframe_step", "ms_frame0", "ms_per_step"):
                r["%s_%s" % (k, mode)] = round(float(np.median([x[k] for x in runs[mode]])), 4)
            r["drift_last_frame_m_" + mode] = runs[mode][0]["drift_last_frame_m"]
            r["drift_max_m_" + mode] = runs[mode][0]["drift_max_m"]
        r["track_step_overhead_ms"] = round(r["ms_per_track_step_on"] - r["ms_per_track_step_off"], 4)
        r["keyframe_step_overhead_ms"] = round(r["ms_per_keyframe_step_on"] - r["ms_per_keyframe_step_off"], 4)
        for k in ("segment_kernels_share_percent", "ba_call_share_percent", "kernel_ms_over_T_steps", "segment_kernels", "adopted_last_window"):
            r[k] = runs["on"][0][k]
        results.append(r)
    line = json.dumps(dict(tool="bench_vo_window", width=1241, height=376, keys=2000, keyframe_every=args.keyframe_every, reps=args.reps,
                           procs_per_mode=args.procs, distinct_sequences=args.distinct, speed_m_per_frame=args.speed,
                           window_ba=dict(iters=10, fixed=1, min_obs=2, min_points=3), results=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
