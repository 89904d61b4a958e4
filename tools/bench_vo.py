"""Throughput of the device-resident stereo VO loop (trackingbench_slam_amd.vo.StereoVO) on synthetic stereo sequences.

For every batch size S: S sequences x T frames, rendered once on the host (synth_seq; `--distinct` different sequences,
repeated to fill the batch) and uploaded before anything is timed, so the steps read device-resident frames. Three passes:

    stats   one untimed run that reads the state after every step: pose observations and inliers per tracking frame,
            translation drift against the ground truth
    timed   reset + T steps, HIP events on the loop's stream around every step, one synchronisation at the end
    prof    the same steps with the library's per-kernel event timing on (tb_profile_*): the per-kernel split

--tracker picks the loop's tracking line (test_vo.cpp:712-716): opflow (default), bf or violence with the reference's arguments;
the descriptor trackers also report their matches per tracking frame. projection and projection_map are the two lines of
test_projection.cpp:512-517; the map tracker's step grows with its map, so its tracking step is also reported by the number of
keyframes the map holds (--map-keyframes, default 4; --steps 41 fills four at the default keyframe period). bow is the fourth
line of test_vo.cpp (:711, searchByBow against the keyframe, SetBow on every frame) with a vocabulary trained by
tb_vocab_train_dev on the ORB descriptors of the sequences' first frames (k = 10, one result set per --voc-levels entry;
--bow-set picks test_kitti's or test_vo_1's arguments). lsh is the line test_vo_1 itself runs (:213, searchByNN) with the
reference's LshIndexParams(20, 10, 2) and the bit table of seed 0. Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trackingbench_slam_amd import capi, synth_seq   # noqa: E402
from trackingbench_slam_amd.vo import BOW_TEST_VO_1, StereoVO  # noqa: E402


def train_on_first_frames(first, L, info):
    """vocab= for StereoVO(tracker="bow"): ORB (the loop's arguments) on the sequences' first left images, then
    tb_vocab_train_dev on the extractor's output, all on the loop's context. info receives the tree's size."""
    def make(ctx):
        D, H, W = first.shape
        exr = capi.Extractor(ctx, W, H, 5, 0.8, D, 2000)
        try:
            cap = exr.results_dev()[3]
            kps = torch.zeros((D, cap, 7), dtype=torch.float32, device="cuda")
            desc = torch.zeros((D, cap, 32), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(D, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()   # the context has its own stream
            n = exr.set_images_host(first)
            exr.build_pyramid(n)
            exr.orb(n, 2000, 80.0, 30.0)
            exr.copy_results_dev(n, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), cap)
            ctx.synchronize()
            h, voc, st = ctx.vocab_train_dev(desc, counts, 10, L)
        finally:
            exr.close()
        leaves = np.flatnonzero(np.diff(voc.child_start) == 0)
        info.update(k=10, L=L, descriptors=int(counts.sum().item()), nodes=st["nnodes"], words=st["nwords"],
                    stopped_words=int((voc.weight[leaves[leaves > 0]] == 0).sum()))
        return h
    return make


def centre(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return -T[:3, :3].T @ T[:3, 3]


def run_size(S, L, R, G, T, every, timed_only=False, tracker="opflow", params=None, voc_L=None):
    D = L.shape[1]
    rep = lambda a: a[:, np.arange(S) % D]   # noqa: E731
    dL = torch.from_numpy(np.ascontiguousarray(rep(L))).cuda()
    dR = torch.from_numpy(np.ascontiguousarray(rep(R))).cuda()
    Gs = rep(G)
    voc_info = {}
    kw = dict(vocab=train_on_first_frames(np.ascontiguousarray(L[0]), voc_L, voc_info)) if tracker == "bow" else {}
    vo = StereoVO(S, keyframe_every=every, tracker=tracker, **kw, **(params or {}))
    try:
        # stats (and the first step, which sizes every buffer)
        vo.reset(Gs[0])
        obs, inl, drift, mts = [], [], [], []
        for t in range(T):
            vo.step(dL[t], dR[t] if t % every == 0 else None)
            if timed_only:
                continue
            if t % every:
                obs.append(vo.obs()[1].cpu().numpy()); inl.append(vo.n_inliers().cpu().numpy())
                if tracker != "opflow":
                    mts.append(vo.matches()[1].cpu().numpy())
            Tcw = vo.Tcw().cpu().numpy()
            drift.append([float(np.linalg.norm(centre(Tcw[s]) - centre(Gs[t, s]))) for s in range(S)])
        obs, inl, drift = np.array(obs), np.array(inl), np.array(drift)
        torch.cuda.synchronize()
        # timed
        vo.reset(Gs[0])
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
        torch.cuda.synchronize()
        for t in range(T):
            ev[t][0].record(vo.stream)
            vo.step(dL[t], dR[t] if t % every == 0 else None)
            ev[t][1].record(vo.stream)
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        total_ms = ev[0][0].elapsed_time(ev[-1][1])
        kf = np.array([t % every == 0 for t in range(T)])
        if timed_only:
            return dict(S=S, T=T, frames_per_s=round(S * T / (total_ms / 1e3), 1), total_ms=round(total_ms, 3),
                        **(dict(vocabulary=voc_info) if voc_info else {}))
        # per-kernel split
        vo.reset(Gs[0])
        torch.cuda.synchronize()
        vo.profile_enable(True)
        for t in range(T):
            vo.step(dL[t], dR[t] if t % every == 0 else None)
        rep_ = vo.profile_report()
        vo.profile_enable(False)
    finally:
        vo.close()
    kern = {k: dict(calls=c, ms=round(m, 4)) for k, (c, m) in sorted(rep_.items(), key=lambda kv: -kv[1][1])}
    extra = dict(vocabulary=voc_info) if voc_info else {}
    if mts:
        mts = np.array(mts)
        extra["matches_per_frame"] = dict(mean=round(float(mts.mean()), 1), min=int(mts.min()))
    if tracker == "projection_map":
        # tracking frame t matches against the points of min(t // every + 1, map_keyframes) keyframes
        held = np.array([min(t // every + 1, params["map_keyframes"]) for t in range(T)])
        extra["ms_per_track_step_by_map_keyframes"] = {str(k): round(float(ms[~kf & (held == k)].mean()), 4)
                                                       for k in sorted(set(held[~kf].tolist()))}
    return dict(S=S, T=T, frames_per_s=round(S * T / (total_ms / 1e3), 1), total_ms=round(total_ms, 3),
                ms_per_track_step=round(float(ms[~kf].mean()), 4), ms_per_keyframe_step=round(float(ms[kf].mean()), 4),
                ms_first_keyframe_step=round(float(ms[0]), 4), kernels_ms_over_T_steps=kern,
                obs_per_frame=dict(mean=round(float(obs.mean()), 1), min=int(obs.min())),
                inliers_per_frame=dict(mean=round(float(inl.mean()), 1), min=int(inl.min())),
                drift_m=dict(final_mean=round(float(drift[-1].mean()), 4), final_max=round(float(drift[-1].max()), 4),
                             all_max=round(float(drift.max()), 4)), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic sequences, repeated to fill a batch")
    ap.add_argument("--keyframe-every", type=int, default=10)
    ap.add_argument("--tracker", choices=("opflow", "bf", "violence", "projection", "projection_map", "bow", "lsh"), default="opflow")
    ap.add_argument("--voc-levels", default="5,6", help="bow: depths L of the trained vocabularies (k = 10)")
    ap.add_argument("--bow-set", choices=("test_kitti", "test_vo_1"), default="test_kitti", help="bow: searchByBow's arguments")
    ap.add_argument("--map-keyframes", type=int, default=4, help="projection_map: keyframes the map holds")
    ap.add_argument("--speed", type=float, default=0.5, help="metres per frame of the synthetic sequences")
    ap.add_argument("--timed-only", action="store_true", help="first pass without state reads, then the timed pass only "
                    "(for a trace of the steps: no host <-> device copy between them)")
    args = ap.parse_args()
    T = args.steps
    seqs = [synth_seq.sequence(s, T, speed=args.speed) for s in range(args.distinct)]
    params = dict(map_keyframes=args.map_keyframes) if args.tracker == "projection_map" else None
    L = np.stack([q[0] for q in seqs], 1); R = np.stack([q[1] for q in seqs], 1); G = np.stack([q[2] for q in seqs], 1)
    if args.tracker == "bow":
        params = dict(BOW_TEST_VO_1) if args.bow_set == "test_vo_1" else None
        res = [run_size(int(S), L, R, G, T, args.keyframe_every, args.timed_only, args.tracker, params, int(vl))
               for vl in args.voc_levels.split(",") for S in args.sizes.split(",")]
    else:
        res = [run_size(int(S), L, R, G, T, args.keyframe_every, args.timed_only, args.tracker, params) for S in args.sizes.split(",")]
    print(json.dumps(dict(tool="bench_vo", tracker=args.tracker, device=torch.cuda.get_device_name(0), width=1241, height=376,
                          keyframe_every=args.keyframe_every, distinct_sequences=args.distinct, speed_m_per_frame=args.speed,
                          **(params or {}), results=res)))


if __name__ == "__main__":
    main()
