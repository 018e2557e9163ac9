#!/usr/bin/env python3
"""ORB detection and description on the device (uwt_orb_detect_describe_batch*): what it costs, next to SURF on the same frames in the
same run (uwt_surf_detect_describe_batch*, the only comparable figure the project has).  Nobody has measured this before and the
reference publishes no figure, so this is a record, not a bar.

  python tools/orb_bench.py --out profiles/r16/orb_bench.json
      per detector: host-to-host milliseconds of one resident 640 x 480 frame (the synchronous call: key points and descriptors in
      host memory), and frames per second of a resident batch of 16 and of 256 frames (the asynchronous call into device memory,
      then uwt_sync), profiler off.  The 256 frames are the 16 resident slots, each named 16 times.
  rocprofv3 --kernel-trace --stats -d <dir> --output-format csv -- python tools/orb_bench.py --trace-run
      a few batch calls of each detector for the kernel trace, in a run of its own
  python tools/orb_bench.py --merge <dir> --out profiles/r16/orb_bench.json
      adds the per-kernel times of that trace and writes orb_bench.md beside the JSON"""
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
W, H, SLOTS, BATCHES, WINDOW_S, TRACE_CALLS = 640, 480, 16, (16, 256), 0.3, 4
ROW = {"orb": (32, "uint8"), "surf": (64, "float32")}


def setup():
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    ctx = capi.Context(capi.default_params(W, H, 525.0, 525.0, 319.5, 239.5, n_levels=1, first_level=0, last_level=0,
                                           max_frames=SLOTS, max_pairs=1))
    ctx.upload_frames(0, np.stack([synth.texture(W, H, 100 + i) for i in range(SLOTS)]))
    return capi, ctx


def entries(ctx, name):
    return (getattr(ctx, name + "_detect_describe_batch"), getattr(ctx, name + "_detect_describe_batch_async"))


def measure_one(capi, ctx, name):
    import torch
    sync_call, async_call = entries(ctx, name)
    cap = capi.UWT_MATCH_MAX_ROWS
    dim, dtype = ROW[name]
    counts = [len(k) for k, _ in sync_call(list(range(SLOTS)))]          # warm-up, and the counts
    out = (np.zeros((1, cap), capi.KEYPOINT), np.zeros((1, cap, dim), dtype), np.zeros(1, np.int32))
    for _ in range(5):
        sync_call([0], out=out)
    one = []
    for _ in range(50):
        t = time.perf_counter()
        sync_call([0], out=out)
        one.append((time.perf_counter() - t) * 1e3)
    rec = dict(keypoints_per_frame=counts,
               one_frame_host_to_host_ms=dict(median=float(np.median(one)), min=float(np.min(one)), max=float(np.max(one)), calls=len(one)))
    for batch in BATCHES:
        slots = [i % SLOTS for i in range(batch)]
        d_kp = torch.zeros((batch, cap, 8), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((batch, cap, dim), dtype=getattr(torch, dtype), device="cuda")
        d_cnt = torch.zeros(batch, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
        run = lambda: async_call(slots, d_kp.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr())
        for _ in range(2):
            run()
        ctx.sync()
        t = time.perf_counter()
        run()
        ctx.sync()
        calls = max(2, int(WINDOW_S / max(time.perf_counter() - t, 1e-6)))
        rates = []
        for _ in range(5):                                                # five windows of about WINDOW_S each: the spread
            t = time.perf_counter()
            for _ in range(calls):
                run()
            ctx.sync()
            rates.append(calls * batch / (time.perf_counter() - t))
        assert d_cnt.cpu().numpy().tolist() == [counts[s] for s in slots]
        rec["resident_batch_%d_frames_per_s" % batch] = dict(median=float(np.median(rates)), min=float(np.min(rates)),
                                                             max=float(np.max(rates)), windows=len(rates), calls_per_window=calls)
        del d_kp, d_desc, d_cnt
    return rec


def measure(out_path):
    capi, ctx = setup()
    rec = dict(width=W, height=H, slots=SLOTS, source_id=capi.source_id())
    for name in ("orb", "surf"):
        rec[name] = measure_one(capi, ctx, name)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def trace_run():
    capi, ctx = setup()
    for name in ("orb", "surf"):
        for _ in range(TRACE_CALLS):
            entries(ctx, name)[0](list(range(SLOTS)))
    ctx.close()


def merge(trace_dir, out_path):
    rec = json.load(open(out_path))
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no kernel_stats.csv under " + trace_dir)
    kernels = {}
    for row in csv.DictReader(open(files[0])):
        short = row["Name"].split("(")[0].split("::")[-1].split(" ")[-1]
        if short.startswith("k_orb_") or short.startswith("k_surf_"):
            k = kernels.setdefault(short, dict(launches=0, total_us=0.0))
            k["launches"] += int(row["Calls"])
            k["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for k in kernels.values():
        k["us_per_batch_call"] = k["total_us"] / TRACE_CALLS
    rec["kernels"] = kernels
    rec["trace"] = dict(batch_calls=TRACE_CALLS, frames_per_call=SLOTS, tool="rocprofv3 --kernel-trace --stats")
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    lines = ["## Measured on the device (tools/orb_bench.py)", "",
             "One MI355X, %d x %d `synth.texture` frames in %d slots, default parameters of both detectors, profiler off." %
             (rec["width"], rec["height"], rec["slots"]), "",
             "| | ORB | SURF |", "|---|---|---|",
             "| key points per frame | %d..%d | %d..%d |" % (min(rec["orb"]["keypoints_per_frame"]), max(rec["orb"]["keypoints_per_frame"]),
                                                           min(rec["surf"]["keypoints_per_frame"]), max(rec["surf"]["keypoints_per_frame"]))]
    o, s = rec["orb"]["one_frame_host_to_host_ms"], rec["surf"]["one_frame_host_to_host_ms"]
    lines.append("| one resident frame, host to host, ms: median (min .. max, %d calls) | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) |"
                 % (o["calls"], o["median"], o["min"], o["max"], s["median"], s["min"], s["max"]))
    for batch in BATCHES:
        o, s = (rec[n]["resident_batch_%d_frames_per_s" % batch] for n in ("orb", "surf"))
        lines.append("| resident batch of %d, asynchronous into device memory, frames/s: median (min .. max, %d windows) | %.0f (%.0f .. %.0f) | %.0f (%.0f .. %.0f) |"
                     % (batch, o["windows"], o["median"], o["min"], o["max"], s["median"], s["min"], s["max"]))
    lines += ["", "Per kernel, from one `rocprofv3 --kernel-trace --stats` run of its own (%d synchronous batch calls of %d frames per detector):"
              % (TRACE_CALLS, SLOTS), "", "| kernel | launches | us per batch call | share of its detector |", "|---|---|---|---|"]
    for prefix in ("k_orb_", "k_surf_"):
        total = sum(k["total_us"] for n, k in kernels.items() if n.startswith(prefix)) or 1.0
        for name, k in sorted(kernels.items(), key=lambda e: -e[1]["total_us"]):
            if name.startswith(prefix):
                lines.append("| %s | %d | %.1f | %.0f %% |" % (name, k["launches"], k["us_per_batch_call"], 100.0 * k["total_us"] / total))
    with open(os.path.join(os.path.dirname(os.path.abspath(out_path)), "orb_bench.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "orb_bench.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge", default="")
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    elif a.merge:
        merge(a.merge, a.out)
    else:
        measure(a.out)
