#!/usr/bin/env python3
"""System::Tracking for resident pairs: the staged sequence of entry points (SURF -> matcher -> RANSAC -> getGoodKeypoints on the host
-> the live call; what the mirrors' Tracking loop does, and all there was before uwt_tracking_batch) against the chained call, in
which nothing leaves the device between the stages.

  python tools/live_bench.py --out profiles/r13/live_bench.json [--staged-only]
      host-to-host milliseconds of one resident 640 x 480 pair (warm-up, 50 calls, median) and pairs per second of resident batches
      of 16 and 256 pairs, each for both forms, profiler off; and the predicate's effect: a batch of 16 with every previous frame
      on the provided path against every one on detection.  --staged-only: the staged figures alone (a library without the chained
      call: the parent commit)
  python tools/live_bench.py --orb --out profiles/r18/live_bench_orb.json
      RobustMatcher(1): the staged ORB sequence against the ORB chain (uwt_tracking_orb_batch*), with the SURF chain alongside, host to
      host on one resident pair and on resident batches of 16 and 256; the three forms take turns within every round, so a drift of
      the clocks falls on all of them alike
  rocprofv3 --kernel-trace --stats -d <dir> --output-format csv -- python tools/live_bench.py --trace-run chained|staged
      a few one-pair calls of one form for the kernel trace, in a run of its own (no counters together with tracing)

Both forms go through the ctypes binding; the staged one packs and unpacks its intermediate arrays in numpy, as the Python mirror
does — that is part of what it costs a Python caller, and is named in the record."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, CAP, SCENES = 640, 480, 2048, 16
INTR = (525.0, 525.0, 319.5, 239.5)


def setup(max_pairs):
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    ctx = capi.Context(capi.default_params(W, H, *INTR, max_frames=2 * SCENES, max_pairs=max_pairs))
    frames = []
    for s in range(SCENES):
        ref, tgt = synth.render_pair(W, H, *INTR, seed=31 + s)[:2]
        frames += [ref, tgt]
    ctx.upload_frames(0, np.stack(frames))
    ctx.build_pyramids(0, 2 * SCENES)
    ctx.apply_gradient(0, 2 * SCENES)
    return capi, ctx


def pair_lists(n):
    return [2 * (i % SCENES) for i in range(n)], [2 * (i % SCENES) + 1 for i in range(n)]


def staged(ctx, ref, tgt):
    """the staged sequence for a batch of pairs through the batched entry points, host to host; returns (poses, matches kept)"""
    P = len(ref)
    res = ctx.surf_detect_describe_batch(list(ref) + list(tgt), cap=CAP)
    xy = [np.stack([k["x"], k["y"]], 1) for k, _ in res]
    sym = ctx.match_descriptors_batch([(res[i][1], res[P + i][1]) for i in range(P)], cap=CAP)
    rs = ctx.ransac_inliers_batch([(sym[i], xy[i], xy[P + i]) for i in range(P)], cap=CAP, kp_cap=CAP)
    kept = [xy[i][rs[i][1]["query_idx"]] for i in range(P)]
    poses, _ = ctx.estimate_pose_features_batch(ref, tgt, [k[:200] for k in kept])
    return poses, [len(k) for k in kept]


def timed(fn, warm, calls):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def summary(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), calls=len(v))


def measure(out_path, staged_only):
    import torch
    capi, ctx = setup(256)
    chained = hasattr(ctx, "tracking_batch") and not staged_only
    rec = dict(width=W, height=H, cap=CAP, source_id=capi.source_id(), forms=["staged"] + (["chained"] if chained else []))
    ref1, tgt1 = pair_lists(1)
    poses, kept = staged(ctx, ref1, tgt1)
    rec["matches_kept_pair0"] = kept[0]
    rec["one_pair_host_to_host_ms"] = dict(staged=summary([t * 1e3 for t in timed(lambda: staged(ctx, ref1, tgt1), 5, 50)]))
    if chained:
        out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, CAP), capi.MATCH),
               np.zeros((1, CAP), capi.KEYPOINT), np.zeros((1, CAP), capi.KEYPOINT))
        r = ctx.tracking_batch(ref1, tgt1, cap=CAP, out=out)
        assert r["poses"].tobytes() == poses.tobytes() and int(r["info"]["n_matches"][0]) == kept[0]
        rec["keypoints_pair0"] = [int(r["info"]["n_kp_prev"][0]), int(r["info"]["n_kp_cur"][0])]
        rec["one_pair_host_to_host_ms"]["chained"] = summary([t * 1e3 for t in timed(lambda: ctx.tracking_batch(ref1, tgt1, cap=CAP, out=out), 5, 50)])
    rec["resident_batch_pairs_per_s"] = {}
    for P, calls in ((16, 10), (256, 2)):
        ref, tgt = pair_lists(P)
        e = rec["resident_batch_pairs_per_s"][str(P)] = dict(staged=summary([P / t for t in timed(lambda: staged(ctx, ref, tgt), 1, calls)]))
        if not chained:
            continue
        i32 = dict(dtype=torch.int32, device="cuda")
        s = dict(poses=torch.zeros((P, 7), **i32), stats=torch.zeros((P, 4), **i32), info=torch.zeros((P, 8), **i32),
                 good=torch.zeros((P, CAP, 3), **i32), kept_prev=torch.zeros((P, CAP, 8), **i32), kept_cur=torch.zeros((P, CAP, 8), **i32),
                 n_matches=torch.zeros((P,), **i32))
        torch.cuda.synchronize()
        io = {k: v.data_ptr() for k, v in s.items()}

        def call(io=io):
            ctx.tracking_batch_async(ref, tgt, io, cap=CAP)
            ctx.sync()
        e["chained"] = summary([P / t for t in timed(call, 1, calls * 3)])
        if P == 16:   # the predicate: every previous frame described at the records it kept, against every one detected
            s2 = {k: torch.zeros_like(v) for k, v in s.items()}
            torch.cuda.synchronize()
            io2 = {k: v.data_ptr() for k, v in s2.items()}
            io2.update(prev_kp=s["kept_prev"].data_ptr(), n_prev=s["n_matches"].data_ptr())
            tp = capi.default_tracking_params(min_matches=1)
            ctx.tracking_batch_async(ref, tgt, io2, params=tp, cap=CAP)
            ctx.sync()
            assert bool(s2["info"].cpu()[:, 1].all())

            def provided():
                ctx.tracking_batch_async(ref, tgt, io2, params=tp, cap=CAP)
                ctx.sync()
            rec["predicate_batch16_pairs_per_s"] = dict(all_detected=e["chained"], all_provided=summary([P / t for t in timed(provided, 1, calls * 3)]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def staged_orb(ctx, ref, tgt):
    """staged() under RobustMatcher(1): ORB and the Hamming matcher (the rows' dtype chooses the norm)"""
    P = len(ref)
    res = ctx.orb_detect_describe_batch(list(ref) + list(tgt), cap=CAP)
    xy = [np.stack([k["x"], k["y"]], 1) for k, _ in res]
    sym = ctx.match_descriptors_batch([(res[i][1], res[P + i][1]) for i in range(P)], cap=CAP)
    rs = ctx.ransac_inliers_batch([(sym[i], xy[i], xy[P + i]) for i in range(P)], cap=CAP, kp_cap=CAP)
    kept = [xy[i][rs[i][1]["query_idx"]] for i in range(P)]
    poses, _ = ctx.estimate_pose_features_batch(ref, tgt, [k[:200] for k in kept])
    return poses, [len(k) for k in kept]


def measure_orb(out_path):
    import torch
    capi, ctx = setup(256)
    rec = dict(width=W, height=H, cap=CAP, source_id=capi.source_id(), forms=["orb_staged", "orb_chained", "surf_chained"], host_to_host={})
    for P, warm, rounds in ((1, 5, 30), (16, 2, 8), (256, 1, 3)):
        ref, tgt = pair_lists(P)
        i32 = dict(dtype=torch.int32, device="cuda")
        s = dict(poses=torch.zeros((P, 7), **i32), stats=torch.zeros((P, 4), **i32), info=torch.zeros((P, 8), **i32),
                 good=torch.zeros((P, CAP, 3), **i32), kept_prev=torch.zeros((P, CAP, 8), **i32), kept_cur=torch.zeros((P, CAP, 8), **i32),
                 n_matches=torch.zeros((P,), **i32))
        torch.cuda.synchronize()
        io = {k: v.data_ptr() for k, v in s.items()}
        out = (np.zeros((P, 7), np.float32), np.zeros(P, capi.STATS), np.zeros(P, capi.TRACKING_INFO), np.zeros((P, CAP), capi.MATCH),
               np.zeros((P, CAP), capi.KEYPOINT), np.zeros((P, CAP), capi.KEYPOINT))

        def orb_chained():
            if P == 1:   # one pair: the synchronous form, results on the host, as the staged sequence leaves them
                return ctx.tracking_orb_batch(ref, tgt, cap=CAP, out=out)
            ctx.tracking_orb_batch_async(ref, tgt, io, cap=CAP)
            ctx.sync()

        def surf_chained():
            if P == 1:
                return ctx.tracking_batch(ref, tgt, cap=CAP, out=out)
            ctx.tracking_batch_async(ref, tgt, io, cap=CAP)
            ctx.sync()

        forms = dict(orb_staged=lambda: staged_orb(ctx, ref, tgt), orb_chained=orb_chained, surf_chained=surf_chained)
        if P == 1:   # the forms agree before they are timed
            poses, kept = staged_orb(ctx, ref, tgt)
            r = ctx.tracking_orb_batch(ref, tgt, cap=CAP, out=out)
            assert r["poses"].tobytes() == poses.tobytes() and int(r["info"]["n_matches"][0]) == kept[0]
            rec["orb_matches_kept_pair0"] = kept[0]
            rec["orb_keypoints_pair0"] = [int(r["info"]["n_kp_prev"][0]), int(r["info"]["n_kp_cur"][0])]
        times = {k: [] for k in forms}
        for k, fn in forms.items():
            for _ in range(warm):
                fn()
        for _ in range(rounds):
            for k, fn in forms.items():
                t = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t)
        rec["host_to_host"][str(P)] = {k: dict(ms=summary([t * 1e3 for t in v]), pairs_per_s=summary([P / t for t in v])) for k, v in times.items()}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def trace_run(form):
    capi, ctx = setup(1)
    ref, tgt = pair_lists(1)
    for _ in range(4):
        if form == "chained":
            ctx.tracking_batch(ref, tgt, cap=CAP)
        else:
            staged(ctx, ref, tgt)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "live_bench.json"))
    ap.add_argument("--staged-only", action="store_true")
    ap.add_argument("--trace-run", choices=["chained", "staged"])
    ap.add_argument("--orb", action="store_true")
    a = ap.parse_args()
    if a.trace_run:
        trace_run(a.trace_run)
    elif a.orb:
        measure_orb(a.out)
    else:
        measure(a.out, a.staged_only)
