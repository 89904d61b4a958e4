"""Step times of the optical-flow VO loop with and without the mono mode (StereoVO(mono=True)), same build, same frames.

For every batch size S: S sequences x T frames (synth_seq; `--distinct` different sequences repeated to fill the batch), uploaded
before anything is timed. Each mode runs one untimed pass (it sizes every buffer), `--repeats` timed passes -- HIP events on the
loop's stream around every step, one synchronisation at the end of a pass -- and one pass with the library's per-kernel event
timing on, which gives k_linear_triangle and k_vo_kf_merge in isolation. The stereo loop gets the right images at every
keyframe, the mono loop at frame 0 only. Frame 0, the stereo keyframe both modes share, is reported apart from the later
keyframes. A step time is the mean over the steps of its kind in one pass; "spread" is the range of that mean over the passes.
Prints one JSON line and writes it to --out (default profiles/vo_mono_bench.json).

--init adds a third column, StereoVO(mono=True, init=dict(baseline=...)): no right image at any step, frame 0 runs ORB only and
the first keyframe whose tracks satisfy the two-view operator initialises a sequence; its keyframe steps carry k_two_view and the
two small kernels around it, which are reported per call, with the frames at which the sequences initialised. --modes picks the
columns (e.g. --modes mono, to time the loop that does not use the new entry points under another build of the library through
TB_HIP_LIB, run by run in alternation).
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


def _passes(vo, dL, dR, G0, T, every, mono, repeats, init=False):
    def run(events=None):
        vo.reset(G0)
        torch.cuda.synchronize()
        for t in range(T):
            right = None if init else dR[t] if (t == 0 if mono else t % every == 0) else None
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
        out["kernels_ms_per_call"] = {k: round(rep[k][1] / rep[k][0], 4) for k in ("k_linear_triangle", "k_vo_kf_merge", "k_vo_mono_alive",
                                                                                   "k_two_view", "k_vo_init_prep", "k_vo_init_adopt")
                                      if k in rep}
        m = vo.mono()
        out["last_keyframe"] = dict(accepted_mean=round(float(m["tri_tally"][:, 1].float().mean().item()), 1),
                                    survivors_mean=round(float(m["survivors"].float().mean().item()), 1),
                                    added_mean=round(float(m["added"].float().mean().item()), 1))
    if init:
        mi = vo.mono_init()
        frames = mi["init_frame"].cpu().numpy()
        out["init_frames"] = {str(int(f)): int((frames == f).sum()) for f in np.unique(frames)}
        out["attempts_mean"] = round(float(mi["attempts"].float().mean().item()), 2)
    out["keyframe_kernels_ms_over_pass"] = {k: round(v[1], 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])[:8]}
    return out


def run_size(S, L, R, G, T, every, repeats, modes, baseline):
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    G0 = rep(G)[0]
    res = dict(S=S, T=T)
    for name, mono, init in (("stereo", None, None), ("mono", True, None), ("mono_init", True, dict(baseline=baseline))):
        if name not in modes:
            continue
        vo = StereoVO(S, keyframe_every=every, mono=mono, init=init)
        try:
            res[name] = _passes(vo, dL, dR, G0, T, every, bool(mono), repeats, bool(init))
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
    ap.add_argument("--init", action="store_true", help="add the column of the mono loop that starts without a right image")
    ap.add_argument("--modes", default="stereo,mono", help="the columns to run (stereo, mono, mono_init)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_mono_bench.json"))
    args = ap.parse_args()
    T = args.steps
    seqs = [synth_seq.sequence(s, T) for s in range(args.distinct)]
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    modes = args.modes.split(",") + (["mono_init"] if args.init else [])
    c = lambda M: -M[:3, :3].T @ M[:3, 3]   # noqa: E731
    baseline = float(np.linalg.norm(c(G[args.keyframe_every, 0].astype(np.float64)) - c(G[0, 0].astype(np.float64))))   # the init pair's
    res = [run_size(int(S), L, R, G, T, args.keyframe_every, args.repeats, modes, baseline) for S in args.sizes.split(",")]
    line = json.dumps(dict(tool="bench_vo_mono", device=torch.cuda.get_device_name(0), width=1241, height=376,
                           keyframe_every=args.keyframe_every, distinct_sequences=args.distinct, repeats=args.repeats, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
