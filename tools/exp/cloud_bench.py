#!/usr/bin/env python3
"""cloud_bench.py — the RGB-D point-cloud map on the device (uwt_point_cloud_batch*), 640 x 480 with depth, on one GPU.  Prints ONE
JSON line:

  one_frame_host    ms per uwt_point_cloud_batch call of one resident frame, pose and cloud on the host: stride 100 (the reference's)
                    and stride 1
  batch_16 / _256   resident batches at stride 1 with poses, cloud and records in device memory (uwt_point_cloud_batch_async +
                    uwt_sync), dense source, skip_invalid 0 (offsets closed-form: one launch) and 1 (count + scan + write); at the
                    largest batch also the candidate source (the producer of the semi-dense calls, then count + scan + write): ms per
                    call (wall clock), frames/s, device_ms (events on the context's stream around the call), points, and beside each
  copy_same_bytes   a device-to-device hipMemcpyAsync of as many bytes as the call wrote, on the same stream: the floor of a pass that
                    mostly writes
  residual_level0   one level-0 residual evaluation of the same batch (first_level = last_level = 0, one iteration, no early exit):
                    the launch time uwt_profile_read_levels reports, the yardstick of profiles/r21

Every figure is the median of --reps timed repetitions (at least 10) after 3 warm-ups, the call and its yardsticks taken in the same
run, in two interleaved rounds.  Inputs: uw-slam_amd/synth.py frames; a depth plane with 1 % holes.

    python tools/exp/cloud_bench.py [--reps 10] [--frames 16,256]
"""
import argparse
import ctypes as C
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
WARMUPS = 3
THRESHOLD = 20.0


def timed(fn, reps):
    for _ in range(WARMUPS):
        fn()
    return [fn() for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", default="16,256")
    a = ap.parse_args()
    reps = max(10, a.reps)
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    sizes = [int(v) for v in a.frames.split(",")]
    scenes = [synth.render_pair(W, H, *INTR, seed=900 + s, with_depth=True) for s in range(N_SCENES)]
    ctx = capi.Context(capi.default_params(W, H, *INTR, max_frames=max(max(sizes), 2 * N_SCENES), max_pairs=max(sizes), has_depth=1,
                                           first_level=0, last_level=0, max_iters=1, early_exit=0))
    ctx.upload_frames(0, np.stack([f for r, t, *_ in scenes for f in (r, t)]), np.stack([d for _, _, d, *_ in scenes for _ in (0, 1)]))
    ctx.build_pyramids(0, 2 * N_SCENES)
    ctx.apply_gradient(0, 2 * N_SCENES)   # (the candidate source and the yardstick need the gradients; the dense source does not)
    L = ctx.level_info(0)
    n_px = L.w * L.h
    out = dict(size=[W, H], depth=True, reps=reps, source_id=capi.source_id())
    rng = np.random.default_rng(4)

    def poses(n):
        q = rng.normal(0, 0.02, (n, 4)) + [0, 0, 0, 1]
        return np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), rng.normal(0, 1, (n, 3))], 1).astype(np.float32)

    one = {}
    for stride in (100, 1):
        p = capi.default_cloud_params(stride=stride)
        tr = poses(1)
        def host():
            t0 = time.perf_counter()
            ctx.point_cloud_batch([0], tr, p, raise_on_failure=True)
            return (time.perf_counter() - t0) * 1e3
        ms = statistics.median(timed(host, reps))
        one["stride_%d" % stride] = dict(ms=ms, frames_per_s=1e3 / ms, points=-(-n_px // stride))
    out["one_frame_host"] = one

    hip_copy = C.CDLL(None).hipMemcpyAsync   # the runtime the library itself runs on
    hip_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.ExternalStream(ctx.stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for F in sizes:
        slots = [i % (2 * N_SCENES) for i in range(F)]
        ref = [2 * (i % N_SCENES) for i in range(F)]
        tgt = [r + 1 for r in ref]
        cap = F * n_px
        d_pts = torch.zeros((cap, 16), dtype=torch.uint8, device="cuda")
        d_src = torch.zeros((cap, 16), dtype=torch.uint8, device="cuda")
        d_info = torch.zeros((F + 1, 32), dtype=torch.uint8, device="cuda")
        d_traj = torch.from_numpy(poses(F)).cuda()
        torch.cuda.synchronize()
        cases = [("dense_emit_all", capi.default_cloud_params(stride=1, skip_invalid=0)),
                 ("dense_skip_invalid", capi.default_cloud_params(stride=1, skip_invalid=1))]
        if F == max(sizes):
            cases.append(("candidates", capi.default_cloud_params(stride=1, skip_invalid=1, source=1, threshold=THRESHOLD)))

        def cloud(p):
            t0 = time.perf_counter()
            e0.record(stream)
            ctx.point_cloud_batch_async(slots, d_traj.data_ptr(), d_pts.data_ptr(), cap, d_info.data_ptr(), p)
            e1.record(stream)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

        def copy(n_bytes):
            e0.record(stream)
            st = hip_copy(d_pts.data_ptr(), d_src.data_ptr(), n_bytes, 3, ctx.stream())   # hipMemcpyDeviceToDevice
            e1.record(stream)
            ctx.sync()
            assert st == 0
            return e0.elapsed_time(e1)

        def residual():
            ctx.profile_enable(True)
            t0 = time.perf_counter()
            ctx.estimate_pose_batch(ref, tgt)
            ms = (time.perf_counter() - t0) * 1e3
            lv = ctx.profile_read_levels()[0]
            ctx.profile_enable(False)
            return ms, lv[0], lv[1]

        wall, dev, cp = {k: [] for k, _ in cases}, {k: [] for k, _ in cases}, {k: [] for k, _ in cases}
        points = {}
        resid_wall, resid_dev, launches = [], [], 0
        for _ in range(2):   # two interleaved rounds
            for name, p in cases:
                for w_ms, d_ms in timed(lambda: cloud(p), reps):
                    wall[name].append(w_ms)
                    dev[name].append(d_ms)
                call = d_info.cpu().numpy().reshape(-1).view(capi.CLOUD_INFO)[F]
                assert call["status"] == 0 and call["written"] == call["offset"]
                points[name] = int(call["offset"])
                cp[name] += timed(lambda: copy(16 * points[name]), reps)
            for w_ms, d_ms, launches in timed(residual, reps):
                resid_wall.append(w_ms)
                resid_dev.append(d_ms)
        block = dict(residual_level0=dict(ms=statistics.median(resid_wall), launch_ms=statistics.median(resid_dev), launches=int(launches)))
        for name, _ in cases:
            ms, d_ms, c_ms = statistics.median(wall[name]), statistics.median(dev[name]), statistics.median(cp[name])
            block[name] = dict(ms=ms, frames_per_s=F / ms * 1e3, device_ms=d_ms, points=points[name], bytes_written=16 * points[name],
                               write_GBps=16 * points[name] / d_ms / 1e6, copy_same_bytes_ms=c_ms, device_over_copy=d_ms / c_ms,
                               device_over_residual=d_ms / statistics.median(resid_dev))
        out["batch_%d" % F] = block
        del d_pts, d_src, d_info, d_traj
    # algorithmic bytes per selected pixel: the dense source reads 2 B of depth and 1 B of the image and writes 16 B; with
    # skip_invalid the count pass reads the 2 B of depth once more; the candidate source reads its 16-B rows twice
    out["bytes_per_selected_row"] = dict(dense_read=3, dense_count_read=2, table_read=16 + 1, table_count_read=16, write=16)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
