"""Step times of the optical-flow VO loop with and without the mono mode (StereoVO(mono=True)), same build, same frames.

For every batch size S: S sequences x T frames (synth_seq; `--distinct` different sequences repeated to fill the batch), uploaded
before anything is timed. Each mode runs one untimed pass (it sizes every buffer), `--repeats` timed passes -- HIP events on the
loop's stream around every step, one synchronisation at the end of a pass -- and one pass with the library's per-kernel event
timing on, which gives k_linear_triangle and k_vo_kf_merge in isolation. The stereo loop gets the right images at every
keyframe, the mono loop at frame 0 only. Frame 0, the stereo keyframe both modes share, is reported apart from the later
keyframes. A step time is the mean over the steps of its kind in one pass; "spread" is the range of that mean over the passes.
Prints one JSON line and writes it to --out (default profiles/vo_mono_bench.json).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trackingbench_slam_amd import synth_seq   # noqa: E402
from trackingbench_slam_amd.vo import StereoVO  # noqa: E402


def _passes(vo, dL, dR, G0, T, every, mono, repeats):
    def run(events=None):
        vo.reset(G0)
        torch.cuda.synchronize()
        for t in range(T):
            right = dR[t] if (t == 0 if mono else t % every == 0) else None
            if events:
                events[t][0].record(vo.stream)
            vo.step(dL[t], right)
            if events:
                events[t][1].record(vo.stream)
        torch.cuda.synchronize()

    run()
    kf = np.array([t % every == 0 for t in range(T)])
    later = kf.copy(); later[0] = False
    track, keyframe, first = [], [], []
    for _ in range(repeats):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
        run(ev)
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        track.append(float(ms[~kf].mean())); keyframe.append(float(ms[later].mean())); first.append(float(ms[0]))
    vo.profile_enable(True)
    run()
    rep = vo.profile_report()
    vo.profile_enable(False)
    stat = lambda v: dict(mean=round(float(np.mean(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))   # noqa: E731
    out = dict(ms_per_track_step=stat(track), ms_per_keyframe_step=stat(keyframe), ms_first_keyframe_step=stat(first))
    if mono:
        out["kernels_ms_per_call"] = {k: round(rep[k][1] / rep[k][0], 4) for k in ("k_linear_triangle", "k_vo_kf_merge", "k_vo_mono_alive")
                                      if k in rep}
        m = vo.mono()
        out["last_keyframe"] = dict(accepted_mean=round(float(m["tri_tally"][:, 1].float().mean().item()), 1),
                                    survivors_mean=round(float(m["survivors"].float().mean().item()), 1),
                                    added_mean=round(float(m["added"].float().mean().item()), 1))
    out["keyframe_kernels_ms_over_pass"] = {k: round(v[1], 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])[:8]}
    return out


def run_size(S, L, R, G, T, every, repeats):
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    G0 = rep(G)[0]
    res = dict(S=S, T=T)
    for name, mono in (("stereo", None), ("mono", True)):
        vo = StereoVO(S, keyframe_every=every, mono=mono)
        try:
            res[name] = _passes(vo, dL, dR, G0, T, every, bool(mono), repeats)
        finally:
            vo.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic sequences, repeated to fill a batch")
    ap.add_argument("--keyframe-every", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per mode: their range is the run-to-run spread")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_mono_bench.json"))
    args = ap.parse_args()
    T = args.steps
    seqs = [synth_seq.sequence(s, T) for s in range(args.distinct)]
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    res = [run_size(int(S), L, R, G, T, args.keyframe_every, args.repeats) for S in args.sizes.split(",")]
    line = json.dumps(dict(tool="bench_vo_mono", device=torch.cuda.get_device_name(0), width=1241, height=376,
                           keyframe_every=args.keyframe_every, distinct_sequences=args.distinct, repeats=args.repeats, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
