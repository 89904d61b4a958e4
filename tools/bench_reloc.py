#!/usr/bin/env python3
"""Measurement for the verification of keyframe-database candidates on the device (tb_relocalize_batch_dev: k_reloc_pairs,
k_bow_search_batch, k_bow_accept_batch, k_reloc_rows, k_pose, k_reloc_select): S query frames, each against the topk stored
keyframes its own ring of N = 16 lists, for S in 16 / 64 / 256.

The frames are 2000-key ORB frames of synth_seq scenes (extracted on the device), their FeatureVectors those of a synthetic
vocabulary (k = 10, L = 5, levelsup 4); a stored keyframe's map points are its keys back-projected with the renderer's depth at
the ground-truth pose, which is also the pose it is stored with. --frames distinct frames are rendered; ring entry (s, j) and
query s cycle through them. The candidates are the first topk slots of a fixed permutation per sequence.

One JSON line per S: per-call wall ms (mean over --reps after a warm-up, synchronised), the per-kernel split from
tb_profile_report, and the yardstick measured in the same session: the same work issued as topk separate
tb_search_by_bow_batch_dev + tb_pose_opt_batch_dev calls on gathered copies of the candidates (the gather is timed on its own; the
rows between the two calls are the ones the batched call made, which the yardstick is not charged for). Its match counts and
inlier counts must equal the batched call's.

--pnp enables tb_kf_store_pnp_enable (256 hypotheses, min_consensus 10, expand 1) on the store: the line then carries the PnP
kernels in its split and how many pairs took the PnP path, and no yardstick (the separate calls have no PnP to compare with).

    python tools/bench_reloc.py [--frames 32] [--keys 2000] [--sizes 16 64 256] [--ring 16] [--topk 4] [--reps 10] [--pnp] [--out FILE]"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from trackingbench_slam_amd import synth, synth_seq  # noqa: E402

W, H = 1241, 376
PER_SEQ = 16
NLEVELS, SCALE = 5, 0.8


def _render(job):
    seed, frames = job
    planes = synth_seq.scene(seed)
    Tcw = synth_seq.trajectory(seed, max(frames) + 1, 0.5)
    out = []
    for f in frames:
        img, aux = synth_seq.render(planes, Tcw[f], W, H, aux=True)
        out.append((img, aux["depth"].astype(np.float32), Tcw[f].astype(np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--topk", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--pnp", action="store_true", help="P3P-RANSAC in front of the pose stage (tb_kf_store_pnp_enable)")
    ap.add_argument("--out", default=None, help="also write the lines to this JSON file (a list)")
    args = ap.parse_args()

    # frames first (worker processes), the GPU after: nothing GPU-side is forked
    jobs = [(s, list(range(min(PER_SEQ, args.frames - s * PER_SEQ)))) for s in range((args.frames + PER_SEQ - 1) // PER_SEQ)]
    with concurrent.futures.ProcessPoolExecutor(args.workers) as ex:
        rendered = [x for chunk in ex.map(_render, jobs) for x in chunk]
    images = np.stack([r[0] for r in rendered]); depth = np.stack([r[1] for r in rendered]); poses = np.stack([r[2] for r in rendered])

    import torch
    from trackingbench_slam_amd import capi
    from trackingbench_slam_amd.synth_seq import KITTI_K as K
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    lib = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    F = len(images)
    exr = capi.Extractor(ctx, W, H, NLEVELS, SCALE, F, args.keys)
    P = exr.results_dev()[3]
    kps = torch.zeros((F, P, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((F, P, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    wid = torch.zeros((F, P), dtype=torch.int32, device=dev); nid = torch.zeros((F, P), dtype=torch.int32, device=dev)
    wt = torch.zeros((F, P), dtype=torch.float64, device=dev)
    fv = torch.zeros((F, P), dtype=torch.int64, device=dev); fvc = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # the context has its own stream
    n = exr.set_images_host(images)
    exr.build_pyramid(n)
    exr.orb(n, args.keys, 40, 10)
    exr.copy_results_dev(n, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), P)
    h = ctx.vocab_create(synth.vocabulary(1, 10, 5))
    ctx.check(lib.tb_bow_transform_batch_dev(ctx._h, h, F, p(desc), p(counts), P, 4, p(wid), p(nid), p(wt), p(fv), p(fvc)))
    ctx.synchronize()
    # map points: the keys back-projected with the renderer's depth at the ground-truth pose
    hk, hc = kps.cpu().numpy(), counts.cpu().numpy()
    mp = np.zeros((F, P, 3), np.float32); valid = np.zeros((F, P), np.uint8)
    for f in range(F):
        m = hc[f]
        x, y = hk[f, :m, 0].astype(np.float64), hk[f, :m, 1].astype(np.float64)
        z = depth[f][np.clip(np.rint(y).astype(int), 0, H - 1), np.clip(np.rint(x).astype(int), 0, W - 1)].astype(np.float64)
        ok = np.isfinite(z) & (z > 0.1) & (z < 80.0)
        z = np.where(ok, z, 1.0)
        Xc = np.stack([(x - K[2]) / K[0] * z, (y - K[3]) / K[1] * z, z], -1)
        T = poses[f].astype(np.float64)
        mp[f, :m] = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
        valid[f, :m] = ok
    mp_d, valid_d, poses_d = torch.from_numpy(mp).to(dev), torch.from_numpy(valid).to(dev), torch.from_numpy(poses).to(dev)
    kps_i = kps.view(torch.int32)
    Kd = (C.c_double * 4)(*K)
    N, topk = args.ring, min(args.topk, args.ring)
    lines = []
    for S in args.sizes:
        entry = (np.arange(S)[:, None] * 7 + np.arange(N)[None, :]) % F          # frame of ring entry (s, j)
        query = (np.arange(S) * 13 + 5) % F
        st = capi.KeyframeStore(ctx, S, N, P, topk)
        if args.pnp:
            ctx.check(st.pnp_enable())
        for j in range(N):
            idx = torch.from_numpy(entry[:, j]).to(dev)
            a = [t[idx].contiguous() for t in (kps_i, desc, counts, fv, fvc, mp_d, valid_d, poses_d)]
            torch.cuda.synchronize()
            st.add(*a, kf_id=j)
            ctx.synchronize()
        qi = torch.from_numpy(query).to(dev)
        q = [t[qi].contiguous() for t in (kps_i, desc, counts, fv, fvc)]
        cand_np = np.stack([np.random.default_rng(s).permutation(N)[:topk] for s in range(S)]).astype(np.int32)
        cand = torch.from_numpy(cand_np).to(dev)
        torch.cuda.synchronize()
        call = lambda: st.relocalize(K, NLEVELS, SCALE, *q, cand, min_inliers=50)
        for _ in range(2):
            out = call()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = call()
        ctx.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.reps
        ctx.profile_enable(True)
        for _ in range(args.reps):
            call()
        ctx.synchronize()
        prof = ctx.profile_report()
        ctx.profile_enable(False)
        if args.pnp:
            pn = st.pnp_state(dev, topk)
            inl = out["cand_inliers"].cpu().numpy()
            line = {"metric": "candidate verification with PnP wall time (tb_relocalize_batch_dev after tb_kf_store_pnp_enable)",
                    "value": round(ms, 4), "unit": "ms", "higher_is_better": False, "n_gpus": 1,
                    "data": "%d synth_seq frames, %d keys/frame, cycled through the rings" % (F, args.keys),
                    "config": {"S": S, "N": N, "topk": topk, "pitch": P, "reps": args.reps, "vocabulary": "synth k=10 L=5, levelsup 4",
                               "pnp": {"hypotheses": 256, "chi2_max": 5.991, "seed": 0, "min_consensus": 10, "expand": 1}},
                    "pairs": S * topk, "pairs_per_s": round(S * topk / (ms * 1e-3), 1),
                    "mean_rows_before_pnp": round(float(pn["row_counts"].float().mean().item()), 1),
                    "mean_consensus": round(float(pn["consensus"].float().mean().item()), 1),
                    "pairs_on_the_pnp_path": int(pn["took"].sum().item()),
                    "mean_rows_per_pair": round(float(out["cand_rows"].float().mean().item()), 1),
                    "pairs_with_50_inliers": int((inl >= 50).sum()), "sequences_relocalised": int((out["best_rank"] >= 0).sum().item()),
                    "kernels_ms_per_call": {k: round(v[1] / args.reps, 4) for k, v in sorted(prof.items())}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            st.close()
            continue
        work = {k: v.clone() for k, v in st.work(dev, topk).items()}
        torch.cuda.synchronize()
        # the yardstick: rank by rank on gathered copies
        sd = st.state_dev()
        full = st.state(dev)
        flat = torch.from_numpy((np.arange(S)[:, None] * N + cand_np).astype(np.int64)).to(dev)     # [S, topk] frame indices
        torch.cuda.synchronize()

        def gather(r):
            i = flat[:, r]
            return [full[k].reshape((S * N,) + tuple(full[k].shape[2:]))[i].contiguous() for k in ("keys", "desc", "fv_keys", "fv_counts", "mp_valid", "Tcw")]

        t0 = time.perf_counter()
        gathered = [gather(r) for r in range(topk)]
        torch.cuda.synchronize()
        gather_ms = 1e3 * (time.perf_counter() - t0)
        rows = [work["rows"].reshape(S, topk, P, 6)[:, r].contiguous() for r in range(topk)]
        rcnt = [work["row_counts"].reshape(S, topk)[:, r].contiguous() for r in range(topk)]
        y_m = torch.zeros((S, P, 4), dtype=torch.int32, device=dev); y_mc = torch.zeros((topk, S), dtype=torch.int32, device=dev)
        y_fl = torch.zeros(S, dtype=torch.int32, device=dev); y_out = torch.zeros((S, P), dtype=torch.uint8, device=dev)
        y_T = torch.zeros((S, 16), dtype=torch.float32, device=dev); y_ni = torch.zeros((topk, S), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def yard():
            for r in range(topk):
                gk, gd, gf, gfc, gv, gT = gathered[r]
                ctx.check(lib.tb_search_by_bow_batch_dev(ctx._h, S, p(q[0]), p(q[1]), P, p(q[3]), p(q[4]), p(gk), p(gd), P, p(gf), p(gfc), p(gv),
                                                         1, 50, C.c_float(6.0), 30, 1, p(y_m), P, p(y_mc[r]), p(y_fl)))
                ctx.check(lib.tb_pose_opt_batch_dev(ctx._h, S, Kd, p(gT), p(rows[r]), p(rcnt[r]), P, p(y_out), p(y_T), p(y_ni[r]), None))

        for _ in range(2):
            yard()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            yard()
        ctx.synchronize()
        yard_ms = 1e3 * (time.perf_counter() - t0) / args.reps
        same = bool((y_mc.t() == out["cand_matches"]).all().item() and (y_ni.t() == out["cand_inliers"]).all().item())
        inl = out["cand_inliers"].cpu().numpy()
        line = {"metric": "candidate verification wall time (tb_relocalize_batch_dev)", "value": round(ms, 4), "unit": "ms",
                "higher_is_better": False, "n_gpus": 1,
                "data": "%d synth_seq frames, %d keys/frame, cycled through the rings" % (F, args.keys),
                "config": {"S": S, "N": N, "topk": topk, "pitch": P, "reps": args.reps, "vocabulary": "synth k=10 L=5, levelsup 4"},
                "pairs": S * topk, "pairs_per_s": round(S * topk / (ms * 1e-3), 1),
                "mean_matches_per_pair": round(float(out["cand_matches"].float().mean().item()), 1),
                "mean_rows_per_pair": round(float(out["cand_rows"].float().mean().item()), 1),
                "pairs_with_50_inliers": int((inl >= 50).sum()), "sequences_relocalised": int((out["best_rank"] >= 0).sum().item()),
                "kernels_ms_per_call": {k: round(v[1] / args.reps, 4) for k, v in sorted(prof.items())},
                "yardstick_separate_calls": {"ms": round(yard_ms, 4), "gather_ms_once": round(gather_ms, 4),
                                             "same_match_and_inlier_counts": same}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        st.close()
        del sd, full, gathered
    ctx.vocab_destroy(h)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
