#!/usr/bin/env python3
"""ransac_bench.py — the RANSAC inlier selection (RobustMatcher::ransacTest, src/Tracker.cpp:105-169, as uwt_ransac_inliers_batch
states it) on one GPU.  Prints ONE JSON line:

  latency_ms   one pair of N matches, 30 % outliers: uwt_ransac_inliers_batch host to host (median, min, max over the repetitions)
               and device_ms: uwt_ransac_inliers_batch_async from matches resident on the device, enqueued and waited for (key-point
               upload included, no result copy); under confidence 0.99 (the adaptive count ends the loop) and 1.0 (all 1000
               hypotheses); hypotheses_run as the device reports it
  throughput   pairs/s of the asynchronous call at 1024 pairs, calls back to back
  parity       every distinct pair, compared as integers with the restatement (tests/ransac_ref.py)

Inputs: tests/ransac_cases.py scene() (two views of random 3-D points, 0.3 px noise).

    python tools/ransac_bench.py [--reps 30]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = (200, 2000)
DISTINCT = 4


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    capi = importlib.import_module("uw-slam_amd.capi")
    import ransac_cases as K
    import ransac_ref as R
    import torch
    reps = max(2, args.reps)
    out = {"metric": "ransac_inliers", "latency_ms": {}, "throughput": {}, "parity": {}}
    ctx = capi.Context(capi.default_params(160, 96, 131.25, 131.25, 79.5, 47.5, max_frames=2, max_pairs=1))
    for n in SIZES:
        pairs = [K.scene(800 + s, n, 0.3, 0.3)[:3] for s in range(DISTINCT)]
        for conf in (0.99, 1.0):
            par = capi.default_ransac_params(confidence=conf)
            key = "n%d_conf%g" % (n, conf)
            got = ctx.ransac_inliers_batch(pairs[:1], params=par)
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.ransac_inliers_batch(pairs[:1], params=par)
                ms.append((time.perf_counter() - t0) * 1e3)
            lat = stats(ms)
            lat["hypotheses_run"] = int(got[0][2]["hypotheses_run"])
            for P in (1, 1024):
                batch = [pairs[i % DISTINCT] for i in range(P)]
                cap, kp_cap, mt, nm, k0, n0, k1, n1 = capi.Context._ransac_block(batch, n, n)
                d_m = torch.from_numpy(mt.view(np.int32).reshape(P, cap, 3)).cuda()
                d_n = torch.from_numpy(nm).cuda()
                d_mask = torch.zeros((P, cap), dtype=torch.uint8, device="cuda")
                d_good = torch.zeros((P, cap, 3), dtype=torch.int32, device="cuda")
                d_cnt = torch.zeros((P,), dtype=torch.int32, device="cuda")
                d_info = torch.zeros((P, 11), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                ptr = lambda a, t: a.ctypes.data_as(capi.C.POINTER(t))
                lib, Cc = capi.lib(), capi.C

                def enqueue():
                    st = lib.uwt_ransac_inliers_batch_async(ctx._h, P, Cc.c_void_p(d_m.data_ptr()), Cc.c_void_p(d_n.data_ptr()), cap,
                                                            ptr(k0, Cc.c_float), ptr(n0, Cc.c_int32), ptr(k1, Cc.c_float), ptr(n1, Cc.c_int32),
                                                            kp_cap, Cc.byref(par), Cc.c_void_p(d_mask.data_ptr()), Cc.c_void_p(d_good.data_ptr()),
                                                            Cc.c_void_p(d_cnt.data_ptr()), Cc.c_void_p(d_info.data_ptr()))
                    assert st == 0, st
                enqueue()
                ctx.sync()
                if P == 1:
                    dev = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        enqueue()
                        ctx.sync()
                        dev.append((time.perf_counter() - t0) * 1e3)
                    lat["device_ms"] = stats(dev)
                else:
                    calls = max(2, min(reps, 8))
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        enqueue()
                    ctx.sync()
                    dt = (time.perf_counter() - t0) / calls
                    out["throughput"][key] = {"pairs": P, "pairs_per_s": round(P / dt, 1), "ms_per_call": round(dt * 1e3, 4), "calls": calls}
                del d_m, d_n, d_mask, d_good, d_cnt, d_info
            out["latency_ms"][key] = lat
            got = ctx.ransac_inliers_batch(pairs, params=par)
            clean = 0
            for (mask, good, info), pr in zip(got, pairs):
                wm, wg, wi = R.ransac(*pr, confidence=conf)
                clean += int(mask.tobytes() == wm.tobytes() and good.tobytes() == wg.tobytes() and info.tobytes() == wi.tobytes())
            out["parity"][key] = {"identical": clean, "pairs": len(pairs)}
    ctx.close()
    out["parity"]["clean"] = all(v["identical"] == v["pairs"] for v in out["parity"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
