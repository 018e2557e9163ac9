#!/usr/bin/env python3
"""candidates_bench.py — semi-dense tracking (Tracker::ObtainCandidatePoints(previous) + EstimatePose(previous, current),
src/Tracker.cpp:1314-1362, :362-597) on one GPU.  Prints ONE JSON line, one block per schedule:

  latency_ms      per call of one pair, pose on the host, the frames already prepared; the new call
                  (uwt_estimate_pose_candidates_batch) beside the per-pair path (uwt_obtain_candidate_points on every iterated
                  level + uwt_estimate_pose_points), at 640x480 with and without depth, 736x480 (EUROC intrinsics, fx != fy), 733x471
  throughput      alignments/s of uwt_track_candidates_batch_async at 1, 64 and 1024 pairs (640x480, depth), calls back to back
  candidates      mean table rows per level of those pairs; mean_iterations: evaluations per pair, all levels
  parity          poses bit-identical to the CPU oracle (candidate_points per level + align_pair_points, one pair at a time)

Schedules: "reference" (the context's defaults: levels 4 -> 1, 50 iterations, early exit) and "fixed4x10" (levels 4 -> 1,
10 iterations each, no early exit).  Inputs: uw-slam_amd/synth.py frames.

--weights identity|tukey|huber and --bilinear: the new call runs under those uwt_table_options (uwt_estimate_pose_candidates_batch_opt
on a context with identity params) and "per-pair path" is that path on a context whose params carry the same weights and sampler
(none exists for Tukey over the bilinear sampler: null).  The two are timed in alternating blocks.  The throughput block then holds
the identity figures of the same run (taken before and again after) beside the mode's, and parity is against the oracle under the mode.
--no-parity leaves the oracle comparison out.

    python tools/candidates_bench.py [--reps 50] [--schedule reference|fixed4x10] [--weights huber] [--bilinear]
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

WEIGHTS = {"identity": 0, "tukey": 1, "huber": 2}
SCHEDULES = {"reference": {}, "fixed4x10": dict(max_iters=10, early_exit=0)}
SIZES = {"640x480": (640, 480, (525.0, 525.0, 319.5, 239.5), False),
         "640x480_depth": (640, 480, (525.0, 525.0, 319.5, 239.5), True),
         "736x480": (736, 480, (458.654, 457.296, 367.215, 248.375), False),
         "733x471": (733, 471, (458.654, 457.296, 366.0, 235.0), False)}
N_SCENES = 16


def scenes(synth, w, h, intr, depth, n):
    return [synth.render_pair(w, h, *intr, seed=900 + s, z=1.1 + 0.03 * s, with_depth=depth)[:3] for s in range(n)]


def load(ctx, sc, depth):
    frames = np.stack([f for r, t, _ in sc for f in (r, t)])
    deps = np.stack([d for _, _, d in sc for _ in (0, 1)]) if depth else None
    ctx.upload_frames(0, frames, deps)
    ctx.build_pyramids(0, len(frames))
    ctx.apply_gradient(0, len(frames))


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


def per_pair_path(ctx, a, b):
    p = ctx.params
    tables = {l: ctx.obtain_candidate_points(a, l, 20.0)[0] for l in range(p.last_level, p.first_level + 1)}
    return ctx.estimate_pose_points(a, b, tables)


def run_schedule(capi, synth, O, over, reps, mode=None, parity=True):
    """mode: None (the existing entries) or (weights, sampler) for the _opt entries"""
    import torch
    out = {"latency_ms": {}, "throughput": {}}
    opt = dict(weights=mode[0], sampler=mode[1]) if mode else {}
    for name, (w, h, intr, depth) in SIZES.items():
        sc = scenes(synth, w, h, intr, depth, 8)
        o = dict(over, has_depth=1) if depth else dict(over)
        ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=16, max_pairs=1, **o))
        load(ctx, sc, depth)
        pp = ctx                                       # the per-pair path's context: its params carry the mode
        if mode:
            pp = None
            if mode != (1, 1):
                pp = capi.Context(capi.default_params(w, h, *intr, max_frames=16, max_pairs=1, **dict(o, **opt)))
                load(pp, sc, depth)
        # the first scene that has candidates on every level (the synthetic texture saturates gradient_, and on some scenes no
        # cell of a level exceeds mean + 20: ERR_NO_VALID_POINTS, the oracle's verdict too)
        j = next(j for j in range(len(sc)) if ctx.estimate_pose_candidates_batch([2 * j], [2 * j + 1], **opt)[1][0]["status"] == 0)
        a, b = 2 * j, 2 * j + 1

        def new_call():
            ctx.estimate_pose_candidates_batch([a], [b], raise_on_pair_failure=True, **opt)

        def old_call():
            per_pair_path(pp, a, b)

        new_ms, old_ms = timed_interleaved(new_call, old_call if pp else None, reps)
        pose_new, st_new = ctx.estimate_pose_candidates_batch([a], [b], **opt)
        pose_old, st_old = per_pair_path(pp, a, b) if pp else (None, None)
        out["latency_ms"][name] = {"new": round(new_ms, 4), "per_pair_path": round(old_ms, 4) if pp else None, "scene": j,
                                   "iterations": st_new[0]["iterations"],
                                   "same_pose_and_stats": bool(np.array_equal(pose_new[0], pose_old) and st_new[0] == st_old) if pp else None}
        if pp is not ctx and pp is not None:
            pp.close()
        ctx.close()

    w, h, intr, _ = SIZES["640x480_depth"]
    sc = scenes(synth, w, h, intr, True, N_SCENES)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2 * N_SCENES, max_pairs=1024, has_depth=1, **over))
    load(ctx, sc, True)
    p = ctx.params
    levels = range(p.last_level, p.first_level + 1)
    for P in (1, 64, 1024):
        ref = (np.arange(P) % N_SCENES * 2).astype(np.int32)
        tgt = ref + 1
        d_poses = torch.zeros((P, 7), dtype=torch.float32, device="cuda")
        d_stats = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        calls = max(3, min(reps, 20000 // P))
        for key, kw in ([("identity", {}), ("mode", opt), ("identity_again", {})] if mode else [(None, {})]):
            ctx.track_candidates_batch_async(ref, tgt, d_poses.data_ptr(), d_stats.data_ptr(), **kw)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                ctx.track_candidates_batch_async(ref, tgt, d_poses.data_ptr(), d_stats.data_ptr(), **kw)
            ctx.sync()
            dt = (time.perf_counter() - t0) / calls
            st = d_stats.cpu().numpy()
            res = {"alignments_per_s": round(P / dt, 1), "ms_per_call": round(dt * 1e3, 4),
                   "mean_iterations": round(float(st[:, 1].mean()), 3), "failed_pairs": int((st[:, 0] != 0).sum())}
            if key is None:
                out["throughput"][str(P)] = res
            else:
                out["throughput"].setdefault(str(P), {})[key] = res
            if P == 64 and key in (None, "mode"):
                parity_batch = (ref, tgt, d_poses.cpu().numpy(), st)
    rows = {str(l): [] for l in levels}
    for j in range(N_SCENES):
        for l in levels:
            rows[str(l)].append(ctx.obtain_candidate_points(2 * j, l, 20.0)[1])
    out["candidates"] = {"rows_per_level_mean": {l: round(float(np.mean(v)), 1) for l, v in rows.items()},
                         "grid_slices_per_level": {str(l): -(-ctx.level_info(l).w * ctx.level_info(l).h // 1024) for l in levels}}
    ctx.close()

    if not parity:
        return out
    ref, tgt, poses, st = parity_batch
    same = 0
    for i in range(len(ref)):
        r, t, d = sc[ref[i] // 2][0], sc[tgt[i] // 2][1], sc[ref[i] // 2][2]
        op = O.default_params(w, h, *intr, **dict(over, **opt))
        op.has_depth = 1
        imgs, deps = O.pyramid(r, op.n_levels), O.pyramid(d, op.n_levels)
        tables = {}
        for l in levels:
            L = O.level_intrinsics(op, l)
            tables[l] = O.candidate_points(O.gradient_mag(*O.scharr3(imgs[l])), deps[l], 20.0, grid=(L.w, L.h))[0]
        so, pose_cpu, tr = O.align_pair_points(op, r, t, tables, ref_depth=d, want_trace=True)
        same += int(so == st[i, 0] and (so != 0 or (np.array_equal(poses[i], pose_cpu) and st[i, 1] == len(tr))))
    out["parity"] = {"bit_identical": same, "pairs": len(ref)}   # status, iterations and (status 0) the pose equal
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--schedule", choices=list(SCHEDULES), action="append")
    ap.add_argument("--weights", choices=list(WEIGHTS), default=None)
    ap.add_argument("--bilinear", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="leave the oracle comparison out (timing runs)")
    args = ap.parse_args()
    mode = (WEIGHTS[args.weights or "identity"], int(args.bilinear)) if (args.weights or args.bilinear) else None
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    from oracle import oracle as O
    O.build()
    out = {"metric": "semi_dense_tracking"}
    if mode:
        out["table_options"] = {"weights": args.weights or "identity", "sampler": "bilinear" if args.bilinear else "round"}
    for name in args.schedule or list(SCHEDULES):
        out[name] = run_schedule(capi, synth, O, SCHEDULES[name], args.reps, mode, not args.no_parity)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
