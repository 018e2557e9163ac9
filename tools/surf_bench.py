#!/usr/bin/env python3
"""SURF detection and description on the device (uwt_surf_detect_describe_batch*): what it costs.  There is no parent implementation
to compare against, so this is a record, not a bar.

  python tools/surf_bench.py --out profiles/r11/surf_bench.json
      host-to-host milliseconds of one resident 640 x 480 frame (the synchronous call: key points and descriptors in host memory),
      and frames per second of a resident batch (the asynchronous call into device memory, then uwt_sync), profiler off
  rocprofv3 --kernel-trace --stats -d <dir> --output-format csv -- python tools/surf_bench.py --trace-run
      a few batch calls for the kernel trace, in a run of its own
  python tools/surf_bench.py --merge <dir> --out profiles/r11/surf_bench.json
      adds the per-kernel times of that trace next to each kernel's algorithmic bytes, and writes the README beside the JSON

Algorithmic bytes (computed from the shapes, code below): integral image 1 B read + 4 B written per pixel per pass pair (the column
pass reads and writes its 4 B again); response 32 gathered dwords per grid point per layer; describe 9 dwords per Haar sample,
109 + 400 samples per key point, plus the 256 B descriptor."""
import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, BATCH, CALLS = 640, 480, 16, 300


def setup():
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    ctx = capi.Context(capi.default_params(W, H, 525.0, 525.0, 319.5, 239.5, n_levels=1, first_level=0, last_level=0,
                                           max_frames=BATCH, max_pairs=1))
    ctx.upload_frames(0, np.stack([synth.texture(W, H, 100 + i) for i in range(BATCH)]))
    return capi, ctx


def algorithmic_bytes(n_frames, keypoints):
    layers, out = 4, {}
    px = W * H
    out["k_surf_integral_rows"] = n_frames * px * (1 + 4)
    out["k_surf_integral_cols"] = n_frames * px * (4 + 4)
    resp = 0
    for o in range(4):
        if (9 + 6 * (layers - 1)) << o <= min(W, H):
            resp += (W >> o) * (H >> o) * layers * 32 * 4
    out["k_surf_response"] = n_frames * resp
    out["k_surf_select"] = keypoints * (32 + 8) * 2
    out["k_surf_describe"] = keypoints * ((109 + 400) * 9 * 4 + 256 + 32)
    return out


def measure(out_path):
    import torch
    capi, ctx = setup()
    cap = capi.UWT_MATCH_MAX_ROWS
    res = ctx.surf_detect_describe_batch(list(range(BATCH)))          # warm-up of both shapes, and the counts
    counts = [len(k) for k, _ in res]
    kp = np.zeros((1, cap), capi.KEYPOINT)
    desc = np.zeros((1, cap, 64), np.float32)
    cnt = np.zeros(1, np.int32)
    for _ in range(5):
        ctx.surf_detect_describe_batch([0], out=(kp, desc, cnt))
    one = []
    for _ in range(50):
        t = time.perf_counter()
        ctx.surf_detect_describe_batch([0], out=(kp, desc, cnt))
        one.append((time.perf_counter() - t) * 1e3)
    d_kp = torch.zeros((BATCH, cap, 8), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((BATCH, cap, 64), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    slots = list(range(BATCH))
    for _ in range(3):
        ctx.surf_detect_describe_batch_async(slots, d_kp.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr())
    ctx.sync()
    batch = []
    for _ in range(5):                                                # five windows of CALLS calls (a quarter of a second each): the spread
        t = time.perf_counter()
        for _ in range(CALLS):
            ctx.surf_detect_describe_batch_async(slots, d_kp.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr())
        ctx.sync()
        batch.append(CALLS * BATCH / (time.perf_counter() - t))
    assert d_cnt.cpu().numpy().tolist() == counts
    rec = dict(width=W, height=H, batch=BATCH, keypoints_per_frame=counts,
               one_frame_host_to_host_ms=dict(median=float(np.median(one)), min=float(np.min(one)), max=float(np.max(one)), calls=len(one)),
               resident_batch_frames_per_s=dict(median=float(np.median(batch)), min=float(np.min(batch)), max=float(np.max(batch)),
                                                windows=len(batch), calls_per_window=CALLS),
               source_id=capi.source_id())
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def trace_run():
    capi, ctx = setup()
    for _ in range(4):
        ctx.surf_detect_describe_batch(list(range(BATCH)))
    ctx.close()


def merge(trace_dir, out_path):
    rec = json.load(open(out_path))
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no kernel_stats.csv under " + trace_dir)
    calls_traced = 4
    kp = sum(rec["keypoints_per_frame"])
    bytes_per_call = algorithmic_bytes(rec["batch"], kp)
    kernels = {}
    for row in csv.DictReader(open(files[0])):
        for name in bytes_per_call:
            if name + "(" in row["Name"] or row["Name"].split("(")[0].endswith(name):
                k = kernels.setdefault(name, dict(launches=0, total_us=0.0))
                k["launches"] += int(row["Calls"])
                k["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for name, k in kernels.items():
        k["us_per_batch_call"] = k["total_us"] / calls_traced
        k["algorithmic_bytes_per_batch_call"] = int(bytes_per_call[name])
        k["algorithmic_GB_per_s"] = bytes_per_call[name] / (k["us_per_batch_call"] * 1e-6) / 1e9 if k["us_per_batch_call"] else None
    rec["kernels"] = kernels
    rec["trace"] = dict(batch_calls=calls_traced, frames_per_call=rec["batch"], tool="rocprofv3 --kernel-trace --stats")
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    lines = ["## Measured on the device (tools/surf_bench.py)", "",
             "One MI355X, %d x %d `synth.texture` frames, default parameters, %d..%d key points per frame." %
             (rec["width"], rec["height"], min(rec["keypoints_per_frame"]), max(rec["keypoints_per_frame"])), "",
             "- one resident frame, host to host (synchronous call, key points and descriptors in host memory): median %.3f ms (min %.3f, max %.3f, %d calls)"
             % tuple(rec["one_frame_host_to_host_ms"][k] for k in ("median", "min", "max", "calls")),
             "- resident batch of %d frames, asynchronous call into device memory: median %.0f frames/s (min %.0f, max %.0f over %d windows of %d calls)"
             % ((rec["batch"],) + tuple(rec["resident_batch_frames_per_s"][k] for k in ("median", "min", "max", "windows", "calls_per_window"))), "",
             "Per kernel, from one `rocprofv3 --kernel-trace --stats` run of its own (%d batch calls of %d frames), next to the bytes the"
             % (calls_traced, rec["batch"]), "algorithm needs (computed from the shapes): where each kernel stands.", "",
             "| kernel | launches | us per batch call | algorithmic MB per batch call | algorithmic GB/s |", "|---|---|---|---|---|"]
    for name, k in sorted(kernels.items(), key=lambda e: -e[1]["total_us"]):
        lines.append("| %s | %d | %.1f | %.2f | %.1f |" % (name, k["launches"], k["us_per_batch_call"],
                                                          k["algorithmic_bytes_per_batch_call"] / 1e6, k["algorithmic_GB_per_s"] or 0.0))
    with open(os.path.join(os.path.dirname(os.path.abspath(out_path)), "surf_bench.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "surf_bench.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge", default="")
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    elif a.merge:
        merge(a.merge, a.out)
    else:
        measure(a.out)
