"""What ragged batches cost the VO loop (trackingbench_slam_amd.vo.StereoVO: reset(which=), step(active=, keyframe=)).

For every batch size S, three loops over T frames of synthetic stereo sequences (synth_seq, KITTI geometry, 2000 keys, uploaded
before anything is timed), alternating in one session:

  a  the lock-step loop through tb_vo_step_dev -- the yardstick: the path a loop without ragged batches runs, unchanged;
  b  the same schedule through tb_vo_step_ragged_dev with NULL masks (it must launch what a launches);
  c  a staggered schedule: sequence s is reset at step s % keyframe_every and is active from then on, so from step
     keyframe_every - 1 on every step carries about S / keyframe_every keyframes among tracking frames.

A loop's figure is the median over --reps of its mean step time (HIP events on the loop's stream around every step, one
synchronisation at the end). For c the steady steps (all sequences started) are reported next to the figure to
hold them against: a tracking step of a plus 1 / keyframe_every of a's keyframe block. The final poses of a and b must be equal bit
for bit. One more run of c under tb_profile gives the new kernels' share. Prints one JSON line and writes it to
profiles/vo_ragged_bench.json (--out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trackingbench_slam_amd import synth, synth_seq   # noqa: E402
from trackingbench_slam_amd.vo import StereoVO  # noqa: E402

NEW_KERNELS = ("k_vo_hold", "k_vo_kf_snapshot", "k_vo_kf_gather", "k_vo_reset_seq")


def _events(vo, T, body):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(T + 1)]
    torch.cuda.synchronize()
    for t in range(T):
        ev[t].record(vo.stream)
        body(t)
    ev[T].record(vo.stream)
    torch.cuda.synchronize()
    return np.array([ev[t].elapsed_time(ev[t + 1]) for t in range(T)])


def run_lock(vo, dL, dR, G0, T, every, ragged_entry):
    """a / b: reset + T lock-step frames -> (ms per step [T], final poses)"""
    S, H, W = dL.shape[1:]
    vo.reset(G0)

    def body(t):
        r = dR[t] if t % every == 0 else None
        if ragged_entry:
            vo._enter(dL[t], r)
            vo.ctx.check(vo.vo.step_ragged_dev(dL[t].data_ptr(), r.data_ptr() if r is not None else None, W, W * H))
        else:
            vo.step(dL[t], r)
    return _events(vo, T, body), vo.Tcw().cpu().numpy()


def run_staggered(vo, cL, cR, G0, T, every):
    """c: sequence s joins at step s % every; cL / cR [T, S, H, W] hold every sequence's own frame of the step"""
    S = cL.shape[1]
    start = np.arange(S) % every
    vo.reset(G0, which=np.zeros(S, bool))   # ragged mode, nobody started

    def body(n):
        new = start == n
        if new.any():
            vo.reset(G0, which=new)
        vo.step(cL[n], cR[n], active=start <= n)
    return _events(vo, T, body)


def run_size(S, L, R, G, T, every, tracker, voc, reps):
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    G0 = rep(G)[0]
    # the staggered schedule's frames: sequence s shows its frame n - s % every at step n (frame 0 before it starts: not read)
    fidx = torch.from_numpy(np.clip(np.arange(T)[:, None] - (np.arange(S) % every)[None], 0, T - 1)).cuda()
    sidx = torch.arange(S, device="cuda")[None].expand(T, S)
    cL, cR = dL[fidx, sidx].contiguous(), dR[fidx, sidx].contiguous()
    kw = dict(keyframe_every=every, tracker=tracker)
    if tracker == "bow":
        kw["vocab"] = voc
    loops = {k: StereoVO(S, **kw) for k in "abc"}
    run = {"a": lambda: run_lock(loops["a"], dL, dR, G0, T, every, False), "b": lambda: run_lock(loops["b"], dL, dR, G0, T, every, True),
           "c": lambda: (run_staggered(loops["c"], cL, cR, G0, T, every), None)}
    try:
        for k in "abc":                        # the first run sizes every buffer
            run[k]()
        ms, poses = {k: [] for k in "abc"}, {}
        for _ in range(reps):
            for k in "abc":
                m, poses[k] = run[k]()
                ms[k].append(m)
        vo = loops["c"]
        vo.profile_enable(True)
        run["c"]()
        prof = vo.profile_report()
        vo.profile_enable(False)
    finally:
        for vo in loops.values():
            vo.close()
    med = {k: np.median(np.array(v), 0) for k, v in ms.items()}   # per step, over reps
    kf = np.arange(T) % every == 0
    steady = np.arange(T) >= every - 1
    track_a, key_a = float(med["a"][~kf].mean()), float(med["a"][kf].mean())
    spread_a = float(np.ptp(np.array(ms["a"]).mean(1)))
    all_ms = sum(v[1] for v in prof.values())
    kern = {n: dict(calls=prof[n][0], ms=round(prof[n][1], 4)) for n in NEW_KERNELS if n in prof}
    return dict(S=S, T=T, same_final_poses_a_b=bool(poses["a"].tobytes() == poses["b"].tobytes()),
                ms_per_step=dict(a=round(float(med["a"].mean()), 4), b=round(float(med["b"].mean()), 4), c=round(float(med["c"].mean()), 4)),
                ms_per_track_step=dict(a=round(track_a, 4), b=round(float(med["b"][~kf].mean()), 4)),
                ms_per_keyframe_step=dict(a=round(key_a, 4), b=round(float(med["b"][kf].mean()), 4)),
                run_to_run_spread_a_ms=round(spread_a, 4),
                c_steady_ms_per_step=round(float(med["c"][steady].mean()), 4),
                c_expected_ms_per_step=round(track_a + (key_a - track_a) / every, 4),
                c_keyframes_per_steady_step=round(S / every, 2),
                new_kernels_in_c=kern, new_kernels_share_of_kernel_time_in_c=round(sum(v["ms"] for v in kern.values()) / all_ms, 5) if all_ms else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic sequences, repeated to fill a batch")
    ap.add_argument("--keyframe-every", type=int, default=10)
    ap.add_argument("--tracker", default="opflow", choices=("opflow", "bf", "violence", "projection", "bow"))
    ap.add_argument("--speed", type=float, default=0.5, help="metres per frame of the synthetic sequences")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_ragged_bench.json"))
    args = ap.parse_args()
    T = args.steps
    seqs = [synth_seq.sequence(s, T, speed=args.speed) for s in range(args.distinct)]
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    voc = synth.vocabulary(1, 10, 5) if args.tracker == "bow" else None
    res = [run_size(int(S), L, R, G, T, args.keyframe_every, args.tracker, voc, args.reps) for S in args.sizes.split(",")]
    line = json.dumps(dict(tool="bench_vo_ragged", device=torch.cuda.get_device_name(0), width=1241, height=376, keys=2000,
                           keyframe_every=args.keyframe_every, tracker=args.tracker, reps=args.reps, distinct_sequences=args.distinct,
                           speed_m_per_frame=args.speed, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
