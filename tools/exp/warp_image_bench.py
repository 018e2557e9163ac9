#!/usr/bin/env python3
"""warp_image_bench.py — Tracker::ObtainImageTransformed on the device (uwt_warp_image_batch*), 640 x 480, level 0, with depth, on one
GPU.  Prints ONE JSON line:

  one_pair_host     ms per uwt_warp_image_batch call of one resident pair, poses and results on the host
  batch_16 / _256   resident batches with the poses and results in device memory (uwt_warp_image_batch_async + uwt_sync): ms per call
                    (wall clock), pairs/s, device_ms (events on the context's stream around the call: the two memsets, k_warp_scatter
                    and k_warp_resolve), under the rendered ground-truth poses and under a contracting pose (tz = +0.3: ~40 % of the
                    landed rows lose their pixel to a later row, the worst case for the atomics); and beside them
  residual_level0   one level-0 residual evaluation of the same batch (first_level = last_level = 0, one iteration, no early exit):
                    the launch time uwt_profile_read_levels reports — the yardstick: it touches the same planes once
  bytes_per_pixel   algorithmic bytes per source pixel as the code implies them

Every figure is the median of --reps timed repetitions (at least 10) after 3 warm-ups; the warp and the yardstick are taken in two
interleaved rounds.  Inputs: uw-slam_amd/synth.py frames.

    python tools/exp/warp_image_bench.py [--reps 10] [--pairs 16,256]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, INTR = 640, 480, (525.0, 525.0, 319.5, 239.5)
N_SCENES = 8
CONTRACT = np.array([0, 0, 0, 1, 0, 0, 0.3], np.float32)
WARMUPS = 3


def median_ms(fn, reps):
    for _ in range(WARMUPS):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", default="16,256")
    a = ap.parse_args()
    reps = max(10, a.reps)
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    sizes = [int(v) for v in a.pairs.split(",")]
    scenes = [synth.render_pair(W, H, *INTR, seed=900 + s, with_depth=True) for s in range(N_SCENES)]
    gt = np.stack([np.concatenate([synth._quat_from_R(R), t]).astype(np.float32) for _, _, _, R, t in scenes])
    ctx = capi.Context(capi.default_params(W, H, *INTR, max_frames=2 * N_SCENES, max_pairs=max(sizes), has_depth=1, first_level=0,
                                           last_level=0, max_iters=1, early_exit=0))
    ctx.upload_frames(0, np.stack([f for r, t, *_ in scenes for f in (r, t)]), np.stack([d for _, _, d, *_ in scenes for _ in (0, 1)]))
    ctx.build_pyramids(0, 2 * N_SCENES)
    ctx.apply_gradient(0, 2 * N_SCENES)   # (the yardstick needs the gradients; the warp does not)
    L = ctx.level_info(0)
    out = dict(size=[W, H], level=0, depth=True, reps=reps, source_id=capi.source_id())

    host = median_ms(lambda: ctx.warp_image_batch([0], [1], gt[:1], lvl=0, raise_on_pair_failure=True), reps)
    out["one_pair_host"] = dict(ms=statistics.median(host), pairs_per_s=1e3 / statistics.median(host))

    stream = torch.cuda.ExternalStream(ctx.stream())
    for P in sizes:
        ref = [2 * (i % N_SCENES) for i in range(P)]
        tgt = [r + 1 for r in ref]
        plane = L.pitch * L.img_h
        u8 = dict(dtype=torch.uint8, device="cuda")
        bufs = dict(warped=torch.zeros((P, plane), **u8), valid=torch.zeros((P, plane), **u8), absdiff=torch.zeros((P, plane), **u8),
                    quality=torch.zeros((P, 48), **u8))
        io = {k: v.data_ptr() for k, v in bufs.items()}
        poses = {"ground_truth": torch.from_numpy(np.stack([gt[i % N_SCENES] for i in range(P)])).cuda(),
                 "contracting": torch.from_numpy(np.tile(CONTRACT, (P, 1))).cuda()}
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        def warp(kind):
            """one call: (wall ms, device ms)"""
            t0 = time.perf_counter()
            e0.record(stream)
            ctx.warp_image_batch_async(ref, tgt, poses[kind].data_ptr(), io, lvl=0)
            e1.record(stream)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

        def residual():
            """one level-0 evaluation of the batch: (wall ms, the launches' ms by uwt_profile_read_levels, launches)"""
            ctx.profile_enable(True)
            t0 = time.perf_counter()
            ctx.estimate_pose_batch(ref, tgt)
            ms = (time.perf_counter() - t0) * 1e3
            lv = ctx.profile_read_levels()[0]
            ctx.profile_enable(False)
            return ms, lv[0], lv[1]

        wall, dev = {k: [] for k in poses}, {k: [] for k in poses}
        resid_wall, resid_dev, launches = [], [], 0
        for _ in range(2):   # two interleaved rounds
            for kind in poses:
                for _ in range(WARMUPS):
                    warp(kind)
                for _ in range(reps):
                    w_ms, d_ms = warp(kind)
                    wall[kind].append(w_ms)
                    dev[kind].append(d_ms)
            for _ in range(WARMUPS):
                residual()
            for _ in range(reps):
                w_ms, d_ms, launches = residual()
                resid_wall.append(w_ms)
                resid_dev.append(d_ms)
        q = bufs["quality"].cpu().numpy().reshape(-1).view(capi.WARP_QUALITY)
        block = dict(residual_level0=dict(ms=statistics.median(resid_wall), launch_ms=statistics.median(resid_dev), launches=int(launches)))
        for kind in poses:
            ms = statistics.median(wall[kind])
            block[kind] = dict(ms=ms, pairs_per_s=P / ms * 1e3, device_ms=statistics.median(dev[kind]),
                               device_ns_per_source_pixel=statistics.median(dev[kind]) * 1e6 / (P * L.w * L.h))
        block["last_quality_pair0"] = {k: int(q[0][k]) for k in ("n_points", "n_landed", "n_covered")}
        out["batch_%d" % P] = block
        del bufs, poses
    # the scatter reads 2 B depth and makes one 4-B atomic; the resolve reads 4 B winner, 1 B gather, 1 B target and 1 B of image1 at
    # the target pixel (sum_abs_unaligned), and writes warped, valid and absdiff; ahead of both the 4-B memset of the winner plane
    out["bytes_per_pixel"] = dict(memset=4, scatter_read=2, scatter_atomic=4, resolve_read=7, resolve_write=3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
