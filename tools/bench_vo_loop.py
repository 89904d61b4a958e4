"""What loop correction costs the searchByBow VO loop when nothing closes (trackingbench_slam_amd.vo.StereoVO, loop_close=...).

For every batch size S: the bow loop with the keyframe database and store (keyframe_db=N, relocalize=M) over T frames of synthetic
stereo sequences (synth_seq, uploaded before anything is timed), run with loop correction off and with it on in the same session
-- the yardstick is the loop with correction off. min_inliers is so high by default that nothing ever closes, so every keyframe
step t > 0 pays exactly the healthy stage: the database query, the verification of the candidates, the graph kernel (edge count
0), the solver's kernel (every graph returns at its check) and the adopt kernel, which finds nothing to adopt; tracking steps pay
nothing. Both loops are run --reps times, alternating; a loop's figure is the median over reps of its mean step time (HIP events
on the loop's stream around the T steps, one synchronisation at the end). The loops' final states -- poses, carried map points,
the keyframe snapshot's points, the store's poses and points -- must be equal bit for bit. Prints one JSON line and writes it to
profiles/vo_loop_bench.json (--out).
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


def timed_run(vo, dL, dR, G0, T, every):
    """reset + T steps -> (total ms, ms of the tracking steps' mean, final poses)"""
    vo.reset(G0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(T + 1)]
    torch.cuda.synchronize()
    for t in range(T):
        ev[t].record(vo.stream)
        vo.step(dL[t], dR[t] if t % every == 0 else None)
    ev[T].record(vo.stream)
    torch.cuda.synchronize()
    ms = np.array([ev[t].elapsed_time(ev[t + 1]) for t in range(T)])
    kf = np.array([t % every == 0 for t in range(T)])
    # the state a correction could touch, live entries only (what lies beyond a count or under a cleared flag was never written)
    n = lambda x: x.cpu().numpy()   # noqa: E731
    st, snap, (mp, mv) = vo.keyframe_store(), vo.keyframe(), vo.map_points()
    live = n(st["kf_ids"]) >= 0
    final = b"".join(a.tobytes() for a in (n(vo.Tcw()), n(mp)[n(mv) != 0], n(snap["map_points"])[n(snap["mp_valid"]) != 0],
                                           n(st["Tcw"])[live], n(st["map_points"])[n(st["mp_valid"]) != 0], n(st["kf_ids"])))
    return float(ms.sum()), float(ms[~kf].mean()), float(ms[kf].mean()), final


def run_size(S, L, R, G, T, every, voc, cap, loop, reps):
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    G0 = rep(G)[0]
    loops = {"off": StereoVO(S, keyframe_every=every, tracker="bow", vocab=voc, keyframe_db=cap, relocalize=cap),
             "on": StereoVO(S, keyframe_every=every, tracker="bow", vocab=voc, keyframe_db=cap, relocalize=cap, loop_close=loop)}
    try:
        res = {k: [] for k in loops}
        poses = {}
        for k, vo in loops.items():          # the first run sizes every buffer
            timed_run(vo, dL, dR, G0, T, every)
        for _ in range(reps):
            for k, vo in loops.items():
                total, track, key, poses[k] = timed_run(vo, dL, dR, G0, T, every)
                res[k].append((total / T, track, key))
        closed = int(loops["on"].loop()["closed"].sum().item())
        kern = {}
        vo = loops["on"]
        vo.reset(G0)
        torch.cuda.synchronize()
        vo.profile_enable(True)
        for t in range(T):
            vo.step(dL[t], dR[t] if t % every == 0 else None)
        rep_ = vo.profile_report()
        vo.profile_enable(False)
        for name in ("k_vo_loop_graph", "k_pgo", "k_vo_loop_adopt", "k_reloc_pairs", "k_reloc_rows", "k_reloc_select", "k_bow_search",
                     "k_pose", "k_bow_score", "k_bow_db_rank", "k_kf_store_add"):
            if name in rep_:
                kern[name] = dict(calls=rep_[name][0], ms=round(rep_[name][1], 4))
    finally:
        for vo in loops.values():
            vo.close()
    med = {k: np.median(np.array(v), 0) for k, v in res.items()}
    out = dict(S=S, T=T, same_final_state=bool(poses["on"] == poses["off"]), closed_in_last_stage=closed)
    for k in ("off", "on"):
        out["ms_per_step_" + k] = round(float(med[k][0]), 4)
        out["ms_per_track_step_" + k] = round(float(med[k][1]), 4)
        out["ms_per_keyframe_step_" + k] = round(float(med[k][2]), 4)
    out["overhead_ms_per_track_step"] = round(float(med["on"][1] - med["off"][1]), 4)
    out["overhead_ms_per_keyframe_step"] = round(float(med["on"][2] - med["off"][2]), 4)
    out["overhead_percent_per_step"] = round(100.0 * float(med["on"][0] / med["off"][0] - 1.0), 2)
    out["stage_kernels_ms_over_T_steps"] = kern
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic sequences, repeated to fill a batch")
    ap.add_argument("--keyframe-every", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=4, help="keyframe_db = relocalize = topk")
    ap.add_argument("--min-inliers", type=int, default=1000000, help="so high that nothing closes")
    ap.add_argument("--speed", type=float, default=0.5, help="metres per frame of the synthetic sequences")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_loop_bench.json"))
    args = ap.parse_args()
    T = args.steps
    seqs = [synth_seq.sequence(s, T, speed=args.speed) for s in range(args.distinct)]
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    voc = synth.vocabulary(1, 10, 5)
    loop = dict(topk=args.capacity, exclude_newest=1, min_inliers=args.min_inliers, iters=10, w_rot=1.0, w_trans=1.0)
    res = [run_size(int(S), L, R, G, T, args.keyframe_every, voc, args.capacity, loop, args.reps) for S in args.sizes.split(",")]
    line = json.dumps(dict(tool="bench_vo_loop", device=torch.cuda.get_device_name(0), width=1241, height=376, keys=2000,
                           keyframe_every=args.keyframe_every, capacity=args.capacity, loop_close=loop, reps=args.reps,
                           distinct_sequences=args.distinct, speed_m_per_frame=args.speed, results=res))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
