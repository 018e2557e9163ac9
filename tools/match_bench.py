#!/usr/bin/env python3
"""match_bench.py — descriptor matching (the matching half of RobustMatcher::DetectAndTrackFeatures, src/Tracker.cpp:202-236:
knnMatch both ways, ratioTest twice, symmetryTest) on one GPU.  Prints ONE JSON line:

  latency_ms      uwt_match_descriptors_batch of one pair, host descriptors in, matches on the host: median, min and max over
                  the repetitions; device_ms: the same pair enqueued from page-locked arrays and waited for (no result copy)
  throughput      pairs/s of uwt_match_descriptors_batch_async at 1, 64 and 1024 pairs, calls back to back from page-locked
                  arrays (uploads included), and the distance terms (n x m x words x 2 directions) per second that makes
  valu_fraction   vector operations of the contract (L2: 3 f32 operations per term; Hamming: xor + popcount-add per 32 bits) over
                  the vector unit's rate for such operations: 256 CUs x 4 SIMDs x 32 packed f32 (16 integer) lanes x 2.4 GHz
  parity          every pair of a small batch, records compared as integers with the restatement (tests/match_ref.py)

Sizes: 500 x 500 x 32 B (ORB defaults, Hamming), 2000 x 2000 x 64 f32 (SURF), 2000 x 2000 x 128 f32 (SURF extended).
Inputs: uw-slam_amd/synth.py descriptor_pair (60 % true correspondences).

    python tools/match_bench.py [--reps 30]
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

SIZES = {"orb_500x500x32B": (500, 500, 32, "hamming"),
         "surf_2000x2000x64": (2000, 2000, 64, "l2"),
         "surf_2000x2000x128": (2000, 2000, 128, "l2")}
DISTINCT = 4              # generated pairs per size; larger batches repeat them
PEAK_OPS = {"l2": 256 * 4 * 32 * 2.4e9, "hamming": 256 * 4 * 16 * 2.4e9}
OPS_PER_WORD = {"l2": 3, "hamming": 2}


def packed(capi, pairs, P, cap):
    """P pairs (the given ones, repeated) in page-locked fixed-stride arrays"""
    a0 = pairs[0][0]
    q = capi.pinned_empty((P, cap, a0.shape[1]), a0.dtype)
    t = capi.pinned_empty((P, cap, a0.shape[1]), a0.dtype)
    nq, nt = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for i in range(P):
        a, b = pairs[i % len(pairs)]
        q[i, :len(a)], t[i, :len(b)] = a, b
        nq[i], nt[i] = len(a), len(b)
    return q, nq, t, nt


def same_records(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    capi = importlib.import_module("uw-slam_amd.capi")
    synth = importlib.import_module("uw-slam_amd.synth")
    import match_ref as R
    import torch
    out = {"metric": "descriptor_matching", "latency_ms": {}, "throughput": {}, "parity": {}}
    ctx = capi.Context(capi.default_params(160, 96, 131.25, 131.25, 79.5, 47.5, max_frames=2, max_pairs=1))
    for name, (n, m, dim, kind) in SIZES.items():
        pairs = [synth.descriptor_pair(500 + s, n, m, dim, kind)[:2] for s in range(DISTINCT)]
        cap = max(n, m)
        words = dim if kind == "l2" else dim // 4
        # one pair, results on the host
        one = (pairs[0][0][None], np.array([n], np.int32), pairs[0][1][None], np.array([m], np.int32))
        ctx.match_descriptors_batch(packed=one)
        ms = []
        for _ in range(max(2, args.reps)):
            t0 = time.perf_counter()
            ctx.match_descriptors_batch(packed=one)
            ms.append((time.perf_counter() - t0) * 1e3)
        lat = {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}
        thr = {}
        for P in (1, 64, 1024):
            blk = packed(capi, pairs, P, cap)
            d_m = torch.zeros((P, cap, 3), dtype=torch.int32, device="cuda")
            d_c = torch.zeros((P,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            calls = max(2, min(args.reps, 4000 // P))
            ctx.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), packed=blk)
            ctx.sync()
            if P == 1:
                dev = []
                for _ in range(max(2, args.reps)):
                    t0 = time.perf_counter()
                    ctx.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), packed=blk)
                    ctx.sync()
                    dev.append((time.perf_counter() - t0) * 1e3)
                lat["device_ms"] = {"median": round(float(np.median(dev)), 4), "min": round(min(dev), 4), "max": round(max(dev), 4)}
            t0 = time.perf_counter()
            for _ in range(calls):
                ctx.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), packed=blk)
            ctx.sync()
            dt = (time.perf_counter() - t0) / calls
            terms = 2.0 * n * m * words * P
            thr[str(P)] = {"pairs_per_s": round(P / dt, 1), "ms_per_call": round(dt * 1e3, 4), "calls": calls,
                           "word_terms_per_s": round(terms / dt, 1),
                           "valu_fraction": round(terms * OPS_PER_WORD[kind] / dt / PEAK_OPS[kind], 4)}
            if P == 64:   # the asynchronous results of the first DISTINCT pairs go into the parity check
                ctx.sync()
                cnt = d_c.cpu().numpy()
                rec = d_m.cpu().numpy().view(np.uint8).reshape(P, cap, 12)
                async_matches = [np.frombuffer(rec[i, :cnt[i]].tobytes(), capi.MATCH) for i in range(DISTINCT)]
            del blk, d_m, d_c
        out["latency_ms"][name] = lat
        out["throughput"][name] = thr
        # parity: every distinct pair, 2-NN records and matches, synchronous and asynchronous
        got_knn = ctx.knn_match_batch(pairs)
        got = ctx.match_descriptors_batch(pairs)
        clean = 0
        for i, (a, b) in enumerate(pairs):
            want, fwd, _ = R.match(a, b, 0.65)
            clean += int(same_records(got_knn[i], fwd) and same_records(got[i], want) and same_records(async_matches[i], want))
        out["parity"][name] = {"identical": clean, "pairs": len(pairs)}
    ctx.close()
    out["parity"]["clean"] = all(v["identical"] == v["pairs"] for v in out["parity"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
