#!/usr/bin/env python3
"""features_bench.py — the live tracking call (System::Tracking: ObtainPatchesPoints(previous) + EstimatePoseFeatures(previous,
current), src/System.cpp:214-219) on one GPU.  Prints ONE JSON line:

  latency_ms      per live call of one pair, host key points in, pose on the host, the frames already prepared; the new call
                  (uwt_estimate_pose_features_batch) beside today's per-pair path (uwt_obtain_patch_points +
                  uwt_estimate_pose_points), at 640x480 with and without depth, 736x480 (EUROC intrinsics, fx != fy), 733x471
  frame_ms        the same per-frame sequence with the new frame's upload, pyramid and gradients included
  throughput      alignments/s of uwt_track_features_batch_async at 1, 64 and 1024 pairs (640x480), calls back to back
  roofline        algorithmic bytes (22 B per evaluated point-iteration: 16 B table row + I1 + GX + GY + I2) over 8 TB/s
  parity          poses bit-identical to the CPU oracle (patch_points + align_pair_points, one pair at a time)

Inputs: uw-slam_amd/synth.py frames, seeded random key points (the texture covers every pixel).

--weights identity|tukey|huber and --bilinear: the new call runs under those uwt_table_options (uwt_estimate_pose_features_batch_opt)
and "per-pair path" is that path on a context whose params carry the same weights and sampler (none exists for Tukey over the
bilinear sampler: null).  The throughput block then holds the identity figures of the same run (taken before and again after)
beside the mode's, parity is against the oracle under the mode, and frame_ms is left out.  New call and per-pair path are timed in
alternating blocks.  --no-parity leaves the oracle comparison out.

    python tools/features_bench.py [--reps 50] [--weights huber] [--bilinear]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FEATURES = dict(n_levels=5, first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002, handoff_scale_t=1)
SIZES = {"640x480": (640, 480, (525.0, 525.0, 319.5, 239.5), False),
         "640x480_depth": (640, 480, (525.0, 525.0, 319.5, 239.5), True),
         "736x480": (736, 480, (458.654, 457.296, 367.215, 248.375), False),
         "733x471": (733, 471, (458.654, 457.296, 366.0, 235.0), False)}
HBM_BYTES_PER_S = 8e12
ROW_BYTES = 22


def scenes(synth, w, h, intr, depth, n):
    return [synth.render_pair(w, h, *intr, seed=900 + s, z=1.1 + 0.03 * s, with_depth=depth)[:3] for s in range(n)]


def load(ctx, sc, depth):
    frames = np.stack([f for r, t, _ in sc for f in (r, t)])
    deps = np.stack([d for _, _, d in sc for _ in (0, 1)]) if depth else None
    ctx.upload_frames(0, frames, deps)
    ctx.build_pyramids(0, len(frames))
    ctx.apply_gradient(0, len(frames))


def kps_for(rng, w, h, n=200):
    return rng.uniform([6, 6], [w - 7, h - 7], (n, 2)).astype(np.float32)


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def timed_interleaved(fa, fb, reps, blocks=5):
    """ms per call of fa and of fb (None: not run), measured in alternating blocks within one process"""
    fa()
    if fb:
        fb()
    n = max(1, reps // blocks)
    ta = tb = 0.0
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(n):
            fa()
        t1 = time.perf_counter()
        if fb:
            for _ in range(n):
                fb()
        t2 = time.perf_counter()
        ta += t1 - t0
        tb += t2 - t1
    return ta / (n * blocks) * 1e3, (tb / (n * blocks) * 1e3 if fb else None)


WEIGHTS = {"identity": 0, "tukey": 1, "huber": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--weights", choices=list(WEIGHTS), default=None)
    ap.add_argument("--bilinear", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="leave the oracle comparison out (timing runs)")
    args = ap.parse_args()
    # --weights / --bilinear: the new call runs under those uwt_table_options (uwt_estimate_pose_features_batch_opt), "per-pair path"
    # is that path on a context whose params carry the same weights and sampler (none exists for Tukey over the bilinear sampler:
    # null), the two timed in alternating blocks; throughput then holds the identity figures of the same run beside the mode's
    mode = (WEIGHTS[args.weights or "identity"], int(args.bilinear)) if (args.weights or args.bilinear) else None
    opt = dict(weights=mode[0], sampler=mode[1]) if mode else {}
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    import torch
    out = {"metric": "live_call", "latency_ms": {}, "frame_ms": {}, "throughput": {}}
    if mode:
        out["table_options"] = {"weights": args.weights or "identity", "sampler": "bilinear" if args.bilinear else "round"}
    rng = np.random.default_rng(1)

    for name, (w, h, intr, depth) in SIZES.items():
        sc = scenes(synth, w, h, intr, depth, 2)
        over = dict(FEATURES, has_depth=1) if depth else dict(FEATURES)
        ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=4, max_pairs=1, **over))
        load(ctx, sc, depth)
        pp = ctx                                       # the per-pair path's context: its params carry the mode
        if mode:
            pp = None
            if mode != (1, 1):
                pp = capi.Context(capi.default_params(w, h, *intr, max_frames=4, max_pairs=1, **dict(over, **opt)))
                load(pp, sc, depth)
        kp = kps_for(rng, w, h)

        def new_call():
            ctx.estimate_pose_features_batch([0], [1], [kp], raise_on_pair_failure=True, **opt)

        def old_call():
            pts, _ = pp.obtain_patch_points(0, kp)
            return pp.estimate_pose_points(0, 1, {0: pts})

        new_ms, old_ms = timed_interleaved(new_call, old_call if pp else None, args.reps)
        pose_new, _ = ctx.estimate_pose_features_batch([0], [1], [kp], **opt)
        out["latency_ms"][name] = {"new": round(new_ms, 4), "per_pair_path": round(old_ms, 4) if pp else None,
                                   "same_pose": bool(np.array_equal(pose_new[0], old_call()[0])) if pp else None}
        # whole frame: the new current frame arrives (upload into slot 1, its pyramid and gradients), then the live call
        cur = sc[1][1]
        dcur = sc[1][2][None] if depth else None

        def frame(call):
            def run():
                ctx.upload_frames(1, cur[None], dcur)
                ctx.build_pyramids(1, 1)
                ctx.apply_gradient(1, 1)
                call()
            return run
        if not mode:
            out["frame_ms"][name] = {"new": round(timed(frame(new_call), args.reps), 4),
                                     "per_pair_path": round(timed(frame(old_call), args.reps), 4)}
        if pp is not ctx and pp is not None:
            pp.close()
        ctx.close()

    # throughput and roofline at 640x480: 16 scenes, pairs over them, 200 key points each
    w, h, intr, _ = SIZES["640x480"]
    sc = scenes(synth, w, h, intr, False, 16)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=32, max_pairs=1024, **FEATURES))
    load(ctx, sc, False)
    for P in (1, 64, 1024):
        ref = (np.arange(P) % 16 * 2).astype(np.int32)
        tgt = ref + 1
        kps = [kps_for(rng, w, h) for _ in range(P)]
        d_poses = torch.zeros((P, 7), dtype=torch.float32, device="cuda")
        d_stats = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        calls = max(3, min(args.reps, 20000 // P))
        _, cnt = ctx.obtain_patch_points_batch(ref, kps)
        for key, kw in ([("identity", {}), ("mode", opt), ("identity_again", {})] if mode else [(None, {})]):
            ctx.track_features_batch_async(ref, tgt, kps, d_poses.data_ptr(), d_stats.data_ptr(), **kw)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                ctx.track_features_batch_async(ref, tgt, kps, d_poses.data_ptr(), d_stats.data_ptr(), **kw)
            ctx.sync()
            dt = (time.perf_counter() - t0) / calls
            st = d_stats.cpu().numpy()
            point_iters = float((cnt.astype(np.float64) * st[:, 1]).sum())
            floor_s = point_iters * ROW_BYTES / HBM_BYTES_PER_S
            res = {"alignments_per_s": round(P / dt, 1), "ms_per_call": round(dt * 1e3, 4),
                   "mean_iterations": round(float(st[:, 1].mean()), 3),
                   "roofline_ms": round(floor_s * 1e3, 5), "roofline_fraction": round(floor_s / dt, 4)}
            if key is None:
                out["throughput"][str(P)] = res
            else:
                out["throughput"].setdefault(str(P), {})[key] = res
            if P == 64 and key in (None, "mode"):
                parity_batch = (ref, tgt, kps, d_poses.cpu().numpy(), st)
    ctx.close()

    if args.no_parity:
        print(json.dumps(out))
        return
    # parity: the 64-pair batch against the oracle, one pair at a time
    from oracle import oracle as O
    O.build()
    ref, tgt, kps, poses, st = parity_batch
    same = 0
    for i in range(len(ref)):
        r, t = sc[ref[i] // 2][0], sc[tgt[i] // 2][1]
        pts, _ = O.patch_points(kps[i], None, w, h)
        so, pose_cpu, tr = O.align_pair_points(O.default_params(w, h, *intr, **dict(FEATURES, **opt)), r, t, {0: pts}, want_trace=True)
        same += int(so == st[i, 0] and np.array_equal(poses[i], pose_cpu) and st[i, 1] == len(tr))
    out["parity"] = {"bit_identical": same, "pairs": len(ref)}
    out["roofline"] = {"bytes_per_point_iteration": ROW_BYTES, "hbm_bytes_per_s": HBM_BYTES_PER_S}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
