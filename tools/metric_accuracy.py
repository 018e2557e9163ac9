#!/usr/bin/env python3
"""What the metric Jacobian buys, on the device: the 8 rendered pairs of tests/test_metric_ref_cpu.py's evidence test (320 x 240, fx = fy =
262.5, motions up to 2 degrees and 0.03, 4 levels x 10 iterations without early exit) under the reference and the metric Jacobian
(uwt_set_jacobian), the reference's hand-off and keep, with and without depth; rotation and translation error against the rendered
motion.  usage: python tools/metric_accuracy.py [OUT.json]"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_ref as MR
capi = importlib.import_module("uw-slam_amd.capi")
synth = importlib.import_module("uw-slam_amd.synth")
w, h, intr = 320, 240, (262.5, 262.5, 159.5, 119.5)
pairs = [synth.render_pair(w, h, *intr, seed=s, z=1.0, max_t=0.03, max_deg=2.0, with_depth=True) for s in range(8)]
out = {}
for depth in (True, False):
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=16, max_pairs=8, has_depth=int(depth), n_levels=4, first_level=3,
                                           last_level=0, max_iters=10, early_exit=0))
    ctx.upload_frames(0, np.stack([f for p in pairs for f in p[:2]]), np.stack([p[2] for p in pairs for _ in (0, 1)]) if depth else None)
    ctx.build_pyramids(0, 16); ctx.apply_gradient(0, 16)
    ref, tgt = np.arange(0, 16, 2, dtype=np.int32), np.arange(1, 16, 2, dtype=np.int32)
    rows = {"identity": [np.array([0, 0, 0, 1, 0, 0, 0], np.float32)] * 8}
    rows["reference Jacobian, reference hand-off"] = ctx.estimate_pose_batch(ref, tgt)[0]
    rows["reference Jacobian, keep"] = ctx.estimate_pose_batch_seeded(ref, tgt, None, 1)[0]
    ctx.set_jacobian(1)
    rows["metric Jacobian, reference hand-off"] = ctx.estimate_pose_batch(ref, tgt)[0]
    rows["metric Jacobian, keep"] = ctx.estimate_pose_batch_seeded(ref, tgt, None, 1)[0]
    ctx.close()
    for name, poses in rows.items():
        e = [MR.pose_errors(poses[k], pairs[k][3], pairs[k][4]) for k in range(8)]
        r, t = [x[0] for x in e], [x[1] for x in e]
        out["%s | %s" % (name, "depth" if depth else "no depth")] = dict(rot_median_deg=float(np.median(r)), rot_max_deg=float(max(r)),
                                                                         t_median=float(np.median(t)), t_max=float(max(t)))
for k, v in out.items():
    print("%-55s rot median %.3f max %.3f deg   t median %.4f max %.4f" % (k, v["rot_median_deg"], v["rot_max_deg"], v["t_median"], v["t_max"]))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
