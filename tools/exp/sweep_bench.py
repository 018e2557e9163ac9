#!/usr/bin/env python3
"""sweep_bench.py — the depth sweep (uwt_sweep_depth_batch*), 640 x 480, level 0, radius 2, on one GPU.  Prints ONE JSON line:

  one_job           one resident job, per configuration (source 0 / 1, 32 / 64 hypotheses, one / two views): host_ms, a
                    uwt_sweep_depth_batch call with poses and results on the host; device_ms, events on the context's stream around
                    uwt_sweep_depth_batch_async (the list copies, the record's memset, k_grad_mag_slots for source 1, k_sweep); and what
                    the job estimated
  batch_16 / _256   resident batches with the poses and results in device memory (uwt_sweep_depth_batch_async + uwt_sync), 32
                    hypotheses, both sources, one and two views: ms per call (wall clock), jobs/s, device_ms; and beside them
  residual_level0   one level-0 residual evaluation of a batch of as many pairs (first_level = last_level = 0, one iteration, no early
                    exit): the launch time uwt_profile_read_levels reports — the yardstick: it touches the same planes once

Every figure is the median of --reps timed repetitions (at least 10) after 3 warm-ups; the sweeps and the yardstick are taken in two
interleaved rounds.  Inputs: a textured plane at 1 m and two views rendered through its homography (the tests' renderer), codes
uniform in inverse depth over 0.5 .. 2.5 m.

    python tools/exp/sweep_bench.py [--reps 10] [--jobs 16,256]
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, INTR = 640, 480, (525.0, 525.0, 319.5, 239.5)
N_SCENES = 4
WARMUPS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--jobs", default="16,256")
    a = ap.parse_args()
    reps = max(10, a.reps)
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    import depth_sweep_cases as DC   # render_view: the renderer of the tests' designed inputs
    sizes = [int(v) for v in a.jobs.split(",")]
    frames, poses = [], []
    for s in range(N_SCENES):   # scene s: slots 3 s (the reference), 3 s + 1, 3 s + 2 (its views)
        ref = synth.texture(W, H, 700 + s)
        v0, p0 = DC.render_view(synth, ref, INTR, DC.ROT, (0.08, 0.02, 0.0), 1.0)
        v1, p1 = DC.render_view(synth, ref, INTR, -DC.ROT, (-0.03, 0.07, 0.01), 1.0)
        frames += [ref, v0, v1]
        poses.append(np.stack([p0, p1]))
    ctx = capi.Context(capi.default_params(W, H, *INTR, max_frames=3 * N_SCENES, max_pairs=max(sizes + [1]), has_depth=0, first_level=0,
                                           last_level=0, max_iters=1, early_exit=0))
    ctx.upload_frames(0, np.stack(frames))
    ctx.build_pyramids(0, 3 * N_SCENES)
    ctx.apply_gradient(0, 3 * N_SCENES)
    L = ctx.level_info(0)
    plane = L.pitch * L.img_h
    out = dict(size=[W, H], level=0, radius=2, reps=reps, source_id=capi.source_id())
    stream = torch.cuda.ExternalStream(ctx.stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    u8 = dict(dtype=torch.uint8, device="cuda")

    def job_lists(J, nv):
        ref = [3 * (i % N_SCENES) for i in range(J)]
        views = [r + 1 + v for r in ref for v in range(nv)]
        d_poses = torch.from_numpy(np.stack([poses[i % N_SCENES][:nv] for i in range(J)])).cuda()
        return ref, views, d_poses

    def sweep_call(ref, views, d_poses, codes, io, params):
        """one asynchronous call and its wait: (wall ms, device ms)"""
        t0 = time.perf_counter()
        e0.record(stream)
        ctx.sweep_depth_async(ref, views, d_poses.data_ptr(), codes, io, params)
        e1.record(stream)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def residual(ref, tgt):
        """one level-0 evaluation of the batch: (wall ms, the launches' ms by uwt_profile_read_levels, launches)"""
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        ctx.estimate_pose_batch(ref, tgt)
        ms = (time.perf_counter() - t0) * 1e3
        lv = ctx.profile_read_levels()[0]
        ctx.profile_enable(False)
        return ms, lv[0], lv[1]

    # ---- one job ------------------------------------------------------------------------------------------------------------------
    bufs = dict(depth=torch.zeros(2 * plane, **u8), cost=torch.zeros(2 * plane, **u8), outcome=torch.zeros(plane, **u8),
                info=torch.zeros(64, **u8))
    io = {k: v.data_ptr() for k, v in bufs.items()}
    configs = [(src, nh, nv) for src in (0, 1) for nh in (32, 64) for nv in (1, 2)]
    host = {c: [] for c in configs}
    dev = {c: [] for c in configs}
    est = {}
    torch.cuda.synchronize()
    for _ in range(2):   # two interleaved rounds
        for c in configs:
            src, nh, nv = c
            codes = capi.sweep_hypotheses(0.5, 2.5, 0.0002, nh)
            params = capi.default_sweep_params(source=src, n_hyp=nh, n_views=nv)
            ref, views, d_poses = job_lists(1, nv)
            torch.cuda.synchronize()
            for k in range(WARMUPS + reps):
                t0 = time.perf_counter()
                r = ctx.sweep_depth(ref, [views], poses[0][:nv], codes, params)
                if k >= WARMUPS:
                    host[c].append((time.perf_counter() - t0) * 1e3)
            est[c] = dict(n_selected=int(r["info"]["n_selected"][0]), n_estimated=int(r["info"]["n_outcome"][0][1]))
            for k in range(WARMUPS + reps):
                _, d_ms = sweep_call(ref, views, d_poses, codes, io, params)
                if k >= WARMUPS:
                    dev[c].append(d_ms)
    out["one_job"] = {"source%d_hyp%d_views%d" % c: dict(host_ms=statistics.median(host[c]), device_ms=statistics.median(dev[c]),
                                                         device_ns_per_selected_pixel=statistics.median(dev[c]) * 1e6 / max(est[c]["n_selected"], 1),
                                                         **est[c]) for c in configs}
    del bufs

    # ---- resident batches -----------------------------------------------------------------------------------------------------------
    codes = capi.sweep_hypotheses(0.5, 2.5, 0.0002, 32)
    for J in sizes:
        bufs = dict(depth=torch.zeros((J, 2 * plane), **u8), cost=torch.zeros((J, 2 * plane), **u8), outcome=torch.zeros((J, plane), **u8),
                    info=torch.zeros((J, 64), **u8))
        io = {k: v.data_ptr() for k, v in bufs.items()}
        kinds = [(src, nv) for src in (0, 1) for nv in (1, 2)]
        lists = {nv: job_lists(J, nv) for nv in (1, 2)}
        torch.cuda.synchronize()
        wall, dv = {k: [] for k in kinds}, {k: [] for k in kinds}
        resid_wall, resid_dev, launches = [], [], 0
        r_ref = lists[1][0]
        r_tgt = [r + 1 for r in r_ref]
        for _ in range(2):   # two interleaved rounds
            for kind in kinds:
                src, nv = kind
                params = capi.default_sweep_params(source=src, n_hyp=32, n_views=nv)
                for k in range(WARMUPS + reps):
                    w_ms, d_ms = sweep_call(*lists[nv], codes, io, params)
                    if k >= WARMUPS:
                        wall[kind].append(w_ms)
                        dv[kind].append(d_ms)
            for k in range(WARMUPS + reps):
                w_ms, d_ms, launches = residual(r_ref, r_tgt)
                if k >= WARMUPS:
                    resid_wall.append(w_ms)
                    resid_dev.append(d_ms)
        info = bufs["info"].cpu().numpy().reshape(-1).view(capi.SWEEP_INFO)
        block = dict(residual_level0=dict(ms=statistics.median(resid_wall), launch_ms=statistics.median(resid_dev), launches=int(launches)))
        for kind in kinds:
            ms = statistics.median(wall[kind])
            block["source%d_views%d" % kind] = dict(ms=ms, jobs_per_s=J / ms * 1e3, device_ms=statistics.median(dv[kind]),
                                                    device_ms_per_job=statistics.median(dv[kind]) / J)
        block["last_info_job0"] = dict(n_selected=int(info[0]["n_selected"]), n_estimated=int(info[0]["n_outcome"][1]))
        out["batch_%d" % J] = block
        del bufs, lists
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
