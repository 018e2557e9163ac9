#!/usr/bin/env python3
"""Track a recorded sequence (EUROC cam0 / TUM rgb[+depth] directory layout, launch/uw_slam*.launch:5-8) through the
GPU path and write the trajectory in the reference visualiser's CSV format and in TUM format.

  python tools/track_sequence.py --images <dir> [--depth <dir>] --fx .. --fy .. --cx .. --cy .. \
         [--width 640 --height 480] [--groundtruth <file> --tum|--euroc] [--weights huber] [--bilinear] --out traj
  python tools/track_sequence.py --images <EUROC cam0/data> --fx 458.654 --fy 457.296 --cx 367.215 --cy 248.375 \
         --distortion=-0.28340811,0.07395907,0.00019359,1.76187114e-05 --rectified-size 736,480 --out traj
      the reference's own EUROC path (calibration/calibrationEUROC.xml): every frame rectified with the maps of CameraModel
      (src/CameraModel.cpp:84-90), cropped to the window System::CalculateROI finds on the first one (src/System.cpp:148-191: a
      data-dependent, odd size) and tracked AT THAT SIZE with the unshifted new camera matrix, as the reference does

No dataset ships with this repository (none is available offline); the synthetic test in tests/test_sequence.py
exercises the same code path.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def track_live(w, h, intr, frames, depths, arith=0, detector=0, jacobian="reference"):
    """System::Tracking over consecutive frames through the Python mirror: (poses [n - 1, 7], stats, matches kept per pair).
    detector: 0 SURF, 1 ORB (RobustMatcher(int detector), src/Tracker.cpp:38-46); jacobian: Tracker.SetJacobian"""
    M = importlib.import_module("uw-slam_amd.tracker")
    fx, fy, cx, cy = intr
    tracker = M.Tracker(bool(depths), max_frames=4, arith=arith)
    tracker.InitializePyramid(w, h, np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32))
    tracker.SetJacobian(jacobian)
    rm = M.RobustMatcher(tracker, detector=detector)
    mk = lambda i: M.Frame(frames[i], depths[i] if depths else None, i)
    poses, stats, kept = [], [], []
    prev = mk(0)
    for i in range(1, len(frames)):
        cur = mk(i)
        st = M.Tracking(tracker, rm, prev, cur)
        poses.append(np.array(prev.rigid_transformation_, np.float32))
        stats.append(st)
        kept.append(int(prev.n_matches_))
        prev = cur
    return np.array(poses, np.float32).reshape(-1, 7), stats, kept


def quality_columns(records, w, h):
    """The three per-pair columns of --quality from uwt_warp_quality records at level 0: the share of the frame the previous frame
    covers after alignment, and the mean |difference| to the current frame over those pixels with and without the alignment"""
    cov = np.maximum(records["n_covered"].astype(np.float64), 1.0)
    return dict(coverage=[float(v) for v in records["n_covered"] / float(w * h)], mean_abs=[float(v) for v in records["sum_abs"] / cov],
                mean_abs_unaligned=[float(v) for v in records["sum_abs_unaligned"] / cov])


def sequence_quality(w, h, intr, frames, depths, poses, arith=0):
    """uwt_warp_quality of every consecutive pair under its pose at level 0 (uwt_warp_image_batch), for the modes whose poses are on
    the host"""
    capi = importlib.import_module("uw-slam_amd.capi")
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2, max_pairs=1, has_depth=int(bool(depths)), arith=arith))
    out = np.zeros(len(poses), capi.WARP_QUALITY)
    for k in range(len(poses)):
        ctx.upload_frames(0, np.stack(frames[k:k + 2]), np.stack(depths[k:k + 2]) if depths else None)
        ctx.build_pyramids(0, 2)
        out[k] = ctx.warp_image_batch([0], [1], poses[k:k + 1], lvl=0, absdiff=False)["quality"][0]
    ctx.close()
    return out


CLOUD_MODES = {"reference": 0, "world": 1}


def cloud_accumulation(mode):
    """(t_scale, reference_axes) of the accumulation a cloud mode takes its poses from: the reference's visualiser reads
    previous_pose_ (t_scale 40, unpermuted: src/Visualizer.cpp:307-313, :425); world: the plain SE(3) prefix product"""
    return (40.0, False) if mode == 0 else (1.0, False)


def sequence_cloud(w, h, intr, frames, depths, poses, stride=100, mode=0, arith=0):
    """Visualizer::AddPointCloudFromRGBD over a tracked sequence, for the modes whose poses are on the host: pair k's previous frame
    under the pose accumulated up to pair k (uwt_accumulate_trajectory, uwt_point_cloud_batch).  Returns capi.CLOUD_POINT records."""
    capi = importlib.import_module("uw-slam_amd.capi")
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=1, max_pairs=1, has_depth=int(bool(depths)), arith=arith))
    t_scale, axes = cloud_accumulation(mode)
    traj = ctx.accumulate_trajectory(np.asarray(poses, np.float32), t_scale=t_scale, reference_axes=axes)
    p = capi.default_cloud_params(mode=mode, stride=stride)
    parts = []
    for k in range(len(traj)):
        ctx.upload_frames(0, frames[k][None], depths[k][None] if depths else None)
        rec = ctx.point_cloud_batch([0], traj[k:k + 1], p)["points"].copy()
        rec["tag"] = (rec["tag"] & 255) | np.uint32(k << 8)
        parts.append(rec)
    ctx.close()
    return np.concatenate(parts) if parts else np.zeros(0, capi.CLOUD_POINT)


def track_live_chained(w, h, intr, frames, depths, arith=0, cap=2048, detector=0, quality=False, cloud=None, motion_model="identity",
                       jacobian="reference"):
    """The same loop as successive one-pair uwt_tracking_batch_async calls (detector 1: uwt_tracking_orb_batch_async): what a frame kept
    goes to the next call in device memory (two sets of buffers, taken in turn), nothing is read back between the calls and the host
    waits once, at the end.  Same returns; quality: behind every call uwt_warp_image_batch_async on its device pose, inside the same
    single wait — the records come back as a fourth result.  cloud = (stride, mode): behind every call the trajectory is
    accumulated from the device poses, one pose per call (uwt_accumulate_trajectory_device_from_async), and, frame by frame while it is resident, the cloud
    enqueued (uwt_point_cloud_batch_async), still inside the single wait — the records come back as the last result.
    motion_model "constant": pair k's live alignment starts from pair k - 1's pose, taken from device memory inside the single wait
    (uwt_tracking_batch_seeded_async / uwt_tracking_orb_batch_seeded_async).
    jacobian "metric": uwt_set_jacobian — the live alignment then runs with z_factor 1 (include/uwt.h "the metric Jacobian")."""
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    n = len(frames)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=4, max_pairs=1, has_depth=int(bool(depths)), arith=arith))
    ctx.set_jacobian(jacobian)
    ctx.set_deferred(True)   # pyramids and gradients are enqueued only
    enqueue = ctx.tracking_orb_batch_async if detector == 1 else ctx.tracking_batch_async
    enqueue_seeded = ctx.tracking_orb_batch_seeded_async if detector == 1 else ctx.tracking_batch_seeded_async
    i32 = dict(dtype=torch.int32, device="cuda")
    poses, stats, info = torch.zeros((n - 1, 7), **i32), torch.zeros((n - 1, 4), **i32), torch.zeros((n - 1, 8), **i32)
    sets = [dict(good=torch.zeros((cap, 3), **i32), kept_prev=torch.zeros((cap, 8), **i32), kept_cur=torch.zeros((cap, 8), **i32),
                 n_matches=torch.zeros((1,), **i32)) for _ in range(2)]
    records = torch.zeros((n - 1, 48), dtype=torch.uint8, device="cuda") if quality else None
    if cloud:
        # A frame leaves its slot three calls later, and pair k's accumulated pose exists once pair k's call is enqueued: behind every
        # call ONE pose is accumulated, row k from row k - 1 in device memory, and frame k's points follow it.
        stride, mode = cloud
        per = -(-(w * h) // stride)
        cp = capi.default_cloud_params(mode=mode, stride=stride)
        t_scale, axes = cloud_accumulation(mode)
        traj = torch.zeros((n - 1, 7), dtype=torch.float32, device="cuda")
        cpts = torch.zeros((n - 1, per, 16), dtype=torch.uint8, device="cuda")
        cinfo = torch.zeros((n - 1, 2, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # torch's fills run on torch's stream

    def load(i):
        ctx.set_frame(i % 4, frames[i], depths[i] if depths else None)
        ctx.build_pyramids(i % 4, 1)
        ctx.apply_gradient(i % 4, 1)

    load(0)
    for k in range(n - 1):
        load(k + 1)
        io = {key: t.data_ptr() for key, t in sets[k % 2].items()}
        io.update(poses=poses[k].data_ptr(), stats=stats[k].data_ptr(), info=info[k].data_ptr())
        if k:
            io.update(prev_kp=sets[(k - 1) % 2]["kept_cur"].data_ptr(), n_prev=sets[(k - 1) % 2]["n_matches"].data_ptr())
        if motion_model == "constant" and k:
            enqueue_seeded([k % 4], [(k + 1) % 4], io, cap=cap, d_seeds_ptr=poses[k - 1].data_ptr())
        else:
            enqueue([k % 4], [(k + 1) % 4], io, cap=cap)
        if quality:
            ctx.warp_image_batch_async([k % 4], [(k + 1) % 4], poses[k].data_ptr(), dict(quality=records[k].data_ptr()), lvl=0)
        if cloud:
            if k:
                ctx.accumulate_trajectory_device_from_async(poses[k].data_ptr(), 1, traj[k - 1].data_ptr(), traj[k].data_ptr(),
                                                            t_scale=t_scale, reference_axes=axes)
            else:
                ctx.accumulate_trajectory_device_async(poses[0].data_ptr(), 1, traj[0].data_ptr(), t_scale=t_scale, reference_axes=axes)
            ctx.point_cloud_batch_async([k % 4], traj[k].data_ptr(), cpts[k].data_ptr(), per, cinfo[k].data_ptr(), cp)
    ctx.sync()
    st = stats.cpu().numpy().view(capi.STATS).reshape(-1)
    kept = info.cpu().numpy().view(capi.TRACKING_INFO).reshape(-1)["n_matches"]
    out = poses.cpu().numpy().view(np.float32).reshape(-1, 7).copy()
    rec = records.cpu().numpy().reshape(-1).view(capi.WARP_QUALITY) if quality else None
    if cloud:
        cl = cpts.cpu().numpy().reshape(n - 1, per * 16).view(capi.CLOUD_POINT).copy()
        written = cinfo.cpu().numpy().reshape(n - 1, 2, 32).view(capi.CLOUD_INFO)[:, 1, 0]["written"]
        for k in range(n - 1):
            cl[k]["tag"] = (cl[k]["tag"] & 255) | np.uint32(k << 8)
        cl = np.concatenate([cl[k, :int(written[k])] for k in range(n - 1)]) if n > 1 else np.zeros(0, capi.CLOUD_POINT)
    ctx.close()
    res = (out, [dict(status=int(s["status"]), iterations=int(s["iterations"]), n_valid=int(s["n_valid"]), error=float(s["error"])) for s in st],
           [int(v) for v in kept])
    if quality:
        res = res + (rec,)
    return res + (cl,) if cloud else res


def keyframe_of(i, interval):
    """the frame that frame i >= 1 is tracked against: N * floor((i - 1) / N) — a fixed policy, nothing in it depends on the data"""
    return interval * ((i - 1) // interval)


def track_keyframes(w, h, intr, frames, depths, over, interval=1, motion_model="identity", handoff="reference", jacobian="reference"):
    """Dense tracking of frame i against its keyframe (keyframe_of) through uwt_track_batch_seeded_async, one pair per call, seeds,
    poses and the trajectory in device memory and one wait at the end (plus the early-exit looks of the calls themselves).
    motion_model "constant": the pair's seed is the constant-velocity prediction in keyframe coordinates
    (uwt_predict_seeds_device_async from the two poses before; the first frame behind a new keyframe starts at the identity, the second
    from prev = identity); with interval 1 — frame-to-frame tracking — the prediction IS the previous pair's pose buffer.
    The world pose of frame i is its keyframe's trajectory row times its pose (uwt_accumulate_trajectory_device_from_async).
    jacobian "metric": uwt_set_jacobian on the context (meant to go with handoff "keep").
    Returns (poses [n - 1, 7] keyframe -> frame, stats, trajectory [n - 1, 7], keyframe index per pair)."""
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    n = len(frames)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=3, max_pairs=1, has_depth=int(bool(depths)), **over))
    ctx.set_jacobian(jacobian)
    f32 = dict(dtype=torch.float32, device="cuda")
    poses, seeds, traj = torch.zeros((n - 1, 7), **f32), torch.zeros((n - 1, 7), **f32), torch.zeros((n - 1, 7), **f32)
    stats = torch.zeros((n - 1, 4), dtype=torch.int32, device="cuda")
    ident = torch.tensor([0, 0, 0, 1, 0, 0, 0], **f32)
    torch.cuda.synchronize()   # torch's fills run on torch's stream
    keys = []
    for i in range(1, n):
        p, kf = i - 1, keyframe_of(i, interval)
        keys.append(kf)
        if kf == i - 1:   # the previous frame becomes the keyframe: slot 0
            ctx.set_frame(0, frames[kf], depths[kf] if depths else None)
            ctx.build_pyramids(0, 1)
        cur = 1 + (i % 2)
        ctx.set_frame(cur, frames[i], depths[i] if depths else None)
        seed = None
        if motion_model == "constant" and p >= 1:
            if interval == 1:
                seed = poses[p - 1].data_ptr()
            elif kf != i - 1:
                before = ident if kf == i - 2 else poses[p - 2]
                ctx.predict_seeds_device_async(1, before.data_ptr(), poses[p - 1].data_ptr(), seeds[p].data_ptr())
                seed = seeds[p].data_ptr()
        ctx.track_batch_seeded_async(cur, 1, [0], [cur], poses[p].data_ptr(), stats[p].data_ptr(), d_seeds_ptr=seed, handoff=handoff)
        if kf == 0:
            ctx.accumulate_trajectory_device_async(poses[p].data_ptr(), 1, traj[p].data_ptr())
        else:
            ctx.accumulate_trajectory_device_from_async(poses[p].data_ptr(), 1, traj[kf - 1].data_ptr(), traj[p].data_ptr())
    ctx.sync()
    st = stats.cpu().numpy().view(capi.STATS).reshape(-1)
    out = (poses.cpu().numpy().copy(), [dict(status=int(s["status"]), iterations=int(s["iterations"]), n_valid=int(s["n_valid"]),
                                              error=float(s["error"])) for s in st], traj.cpu().numpy().copy(), keys)
    ctx.close()
    return out


def sweep_keyframes(w, h, intr, frames, poses, keyframes, n_views, codes, arith=0, source=1):
    """Depth for every keyframe of a keyframe-tracked sequence (track_keyframes) from the first n_views frames tracked against it and
    their poses (keyframe -> frame, the tracker's convention): uwt_sweep_depth_batch_async writes the depth codes straight into the
    keyframe's level-0 depth plane (uwt_plane_device_ptr), which is then read back.  Returns (depth [K, h, w] u16, a list of per-keyframe
    dicts: keyframe, views, coverage = estimated pixels / (w h), n_selected and the counts by uwt_sweep_outcome)."""
    import torch
    capi = importlib.import_module("uw-slam_amd.capi")
    # (the sweep reads level 0 alone: two levels, the least a pyramid has)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=1 + n_views, max_pairs=1, has_depth=1, arith=arith, n_levels=2,
                                           first_level=1, last_level=0))
    planes, report = [], []
    for kf in sorted(set(keyframes)):
        pairs = [p for p, k in enumerate(keyframes) if k == kf][:n_views]   # pair p tracks frame p + 1 against keyframes[p]
        if len(pairs) < n_views:
            continue   # the last keyframe of the sequence may have fewer frames behind it
        batch = np.stack([frames[kf]] + [frames[p + 1] for p in pairs])
        ctx.upload_frames(0, batch, np.zeros(batch.shape, np.uint16))
        ctx.build_pyramids(0, 1 + n_views)
        ctx.apply_gradient(0, 1)
        d_poses = torch.tensor(np.asarray(poses, np.float32)[pairs], dtype=torch.float32, device="cuda")
        d_info = torch.zeros(64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()   # torch's copies run on torch's stream
        params = capi.default_sweep_params(n_views=n_views, n_hyp=len(codes), source=source)
        ctx.sweep_depth_async([0], list(range(1, 1 + n_views)), d_poses.data_ptr(), codes,
                              dict(depth=ctx.plane_device_ptr(0, 0, capi.PLANE_DEPTH), info=d_info.data_ptr()), params)
        ctx.sync()
        planes.append(ctx.get_plane(0, 0, capi.PLANE_DEPTH))   # the keyframe's depth plane, as any consumer reads it
        info = d_info.cpu().numpy().view(capi.SWEEP_INFO)[0]
        report.append(dict(keyframe=int(kf), views=[int(p + 1) for p in pairs], coverage=float(info["n_outcome"][1]) / float(w * h),
                           n_selected=int(info["n_selected"]), outcomes=[int(v) for v in info["n_outcome"]]))
    ctx.close()
    return (np.stack(planes) if planes else np.zeros((0, h, w), np.uint16)), report


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", required=True)
    ap.add_argument("--depth")
    ap.add_argument("--fx", type=float, required=True); ap.add_argument("--fy", type=float, required=True)
    ap.add_argument("--cx", type=float, required=True); ap.add_argument("--cy", type=float, required=True)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--distortion", default="", help="k1,k2,p1,p2: rectify + ROI-crop like the reference (System.cpp:148-191, 231-236); "
                    "--width / --height are then ignored: the frame size is the ROI's")
    ap.add_argument("--rectified-size", default="", help="W,H of the rectified frame (out_width / out_height of the calibration file); default: the input size")
    ap.add_argument("--start", type=int, default=0); ap.add_argument("--count", type=int, default=0)
    ap.add_argument("--weights", choices=["identity", "tukey", "huber"], default="identity")
    ap.add_argument("--bilinear", action="store_true")
    ap.add_argument("--arith", choices=["opencv", "legacy"], default="opencv", help="arithmetic set (include/uwt.h uwt_arith)")
    ap.add_argument("--fixed-iters", type=int, default=0, help="0: the reference schedule (levels 4..1, early exit)")
    ap.add_argument("--groundtruth"); ap.add_argument("--euroc", action="store_true"); ap.add_argument("--tum", action="store_true")
    ap.add_argument("--live", action="store_true", help="the reference's live loop, System::Tracking (src/System.cpp:193-223): SURF key "
                    "points detected, described, matched and RANSAC-filtered on the device, then EstimatePoseFeatures on their patches")
    ap.add_argument("--detector", choices=["surf", "orb"], default="surf", help="with --live: the detector of RobustMatcher(int detector) "
                    "(src/Tracker.cpp:38-46)")
    ap.add_argument("--chained", action="store_true", help="with --live: the loop as successive device-resident calls (uwt_tracking_batch_async, "
                    "uwt_tracking_orb_batch_async with --detector orb) that hand their key points on in device memory, one wait at the end; "
                    "the same trajectory")
    ap.add_argument("--quality", action="store_true", help="per pair, at level 0: the share of the frame the previous frame covers "
                    "under the estimated pose and the mean |difference| over it with and without the alignment "
                    "(Tracker::ObtainImageTransformed on the device; with --chained from the device poses, inside the same single wait)")
    ap.add_argument("--cloud", metavar="OUT.ply", help="write the point-cloud map (Visualizer::AddPointCloudFromRGBD on the device: every "
                    "--cloud-stride-th row of each pair's previous frame under the accumulated pose) as a binary PLY; with --live --chained "
                    "the trajectory and the cloud are enqueued behind the tracking calls, inside the same single wait")
    ap.add_argument("--cloud-stride", type=int, default=100, help="the reference takes every 100th row (src/Visualizer.cpp:437)")
    ap.add_argument("--cloud-mode", choices=sorted(CLOUD_MODES), default="reference", help="reference: the visualiser's axes and offset "
                    "(:440-442); world: the camera points under the plain SE(3) prefix product of the pair poses")
    ap.add_argument("--out", default="trajectory")
    return ap


def add_seed_arguments(ap):
    """where an alignment starts and what it is tracked against (the seeded calls, include/uwt.h): main's parser is build_parser's
    plus these"""
    ap.add_argument("--motion-model", choices=["identity", "constant"], default="identity", help="where an alignment starts: identity, "
                    "as the reference (src/Tracker.cpp:385), or constant velocity — pair k starts from pair k - 1's pose (with --live "
                    "--chained from device memory, inside the single wait), a frame tracked against a keyframe from "
                    "uwt_predict_seeds_device_async")
    ap.add_argument("--keyframe-interval", type=int, default=0, metavar="N", help="dense tracking against keyframes: frame i against frame "
                    "N * floor((i - 1) / N), its world pose from the keyframe's trajectory row; a new keyframe starts at the identity "
                    "(0: consecutive frames through the batch path)")
    ap.add_argument("--handoff", choices=["reference", "keep"], default=None, help="how a seeded pose crosses the pyramid levels "
                    "(uwt_seed_options): the reference's hand-off doubles q.xyz at every level, keep leaves the pose as it is "
                    "(default: reference; keep with --jacobian metric)")
    ap.add_argument("--jacobian", choices=["reference", "metric"], default="reference", help="uwt_set_jacobian: reference, the reference's "
                    "Jw with the warped pixel coordinates in columns 2..5, bit for bit; metric, the 3-D point's coordinates there "
                    "(the correct Jacobian, an extension).  Dense tracking in metric mode goes through the seeded entry (frame to "
                    "frame from the identity unless --keyframe-interval / --motion-model say otherwise) under --handoff keep unless "
                    "another is named; with --live the alignment runs with z_factor 1")
    ap.add_argument("--sweep-depth", type=int, default=0, metavar="N", help="with --keyframe-interval: estimate every keyframe's depth from "
                    "the first N (1..4) frames tracked against it and their poses (uwt_sweep_depth_batch_async, an extension), written "
                    "into the keyframe's level-0 depth plane; reports coverage and the outcome counts per keyframe and saves the planes "
                    "as <out>_sweep_depth.npy.  The tool makes no accuracy claim on depth-less data: poses tracked on z = 1 carry that "
                    "assumption, and the depth swept under them inherits it")
    ap.add_argument("--sweep-range", default="0.5,2.5", metavar="ZNEAR,ZFAR", help="the depth range the hypotheses cover, uniform in "
                    "inverse depth (uwt_sweep_hypotheses)")
    ap.add_argument("--sweep-hyp", type=int, default=32, help="depth hypotheses, 3..64")
    return ap


def main():
    ap = add_seed_arguments(build_parser())
    a = ap.parse_args()
    S = importlib.import_module("uw-slam_amd.sequence")
    T = importlib.import_module("uw-slam_amd.trajectory")
    names = S.list_sorted(a.images)[a.start:]
    dnames = S.list_sorted(a.depth)[a.start:] if a.depth else None
    if a.count:
        names = names[:a.count]
        dnames = dnames[:a.count] if dnames else None
    first = S.load_gray(names[0])
    fx, fy, cx, cy = a.fx, a.fy, a.cx, a.cy
    if a.distortion:
        capi = importlib.import_module("uw-slam_amd.capi")
        dist = [float(v) for v in a.distortion.split(",")]
        ih, iw = first.shape
        ow, oh = [int(v) for v in a.rectified_size.split(",")] if a.rectified_size else (iw, ih)
        ing = capi.Ingest([a.fx, a.fy, a.cx, a.cy], dist, iw, ih, ow, oh)
        x0, y0, a.width, a.height = [int(v) for v in ing.calculate_roi(first)]          # w_, h_ = the ROI's (src/System.cpp:186-190)
        fx, fy, cx, cy = [float(v) for v in ing.newK]                                    # K_ = GetK(): not shifted by the crop (:105-112)
        frames = [np.ascontiguousarray(ing.undistort(S.load_gray(n))[y0:y0 + a.height, x0:x0 + a.width]) for n in names]
        depths = None
        ing.close()
        cx, cy = cx + x0, cy + y0                                                        # (undone below: the reference keeps cx, cy)
    else:
        _, x0, y0 = S.centre_crop(first, a.width, a.height)
        frames = [S.centre_crop(S.load_gray(n), a.width, a.height)[0] for n in names]
        depths = [S.centre_crop(S.load_depth(n), a.width, a.height)[0] for n in dnames] if dnames else None
    over = dict(weights={"identity": 0, "tukey": 1, "huber": 2}[a.weights], sampler=int(a.bilinear), arith={"opencv": 0, "legacy": 1}[a.arith])
    if a.fixed_iters:
        over.update(n_levels=4, first_level=3, last_level=0, max_iters=a.fixed_iters, early_exit=0)
    trk = S.SequenceTracker(a.width, a.height, fx, fy, cx - x0, cy - y0, depth=bool(depths), **over)
    t0 = time.perf_counter()
    if a.detector == "orb" and not a.live:
        ap.error("--detector orb goes with --live")
    if a.cloud and a.cloud_stride < 1:
        ap.error("--cloud-stride must be at least 1")
    if a.keyframe_interval < 0:
        ap.error("--keyframe-interval must be at least 1 (0: off)")
    if a.handoff is None:
        a.handoff = "keep" if a.jacobian == "metric" else "reference"
    # (the unseeded dense entry has the reference's hand-off alone: metric mode takes the seeded one, with null seeds where no model is on)
    seeded = a.keyframe_interval > 0 or ((a.motion_model == "constant" or a.jacobian == "metric") and not a.live)
    if seeded and (a.live or a.quality or a.cloud):
        ap.error("--keyframe-interval (and --motion-model constant without --live) is the dense tracker alone: no --live, --quality or --cloud")
    if a.motion_model == "constant" and a.live and not a.chained:
        ap.error("--motion-model constant with --live goes with --chained")
    if a.sweep_depth and (a.keyframe_interval < 1 or not 1 <= a.sweep_depth <= min(4, a.keyframe_interval)):
        ap.error("--sweep-depth N goes with --keyframe-interval K, 1 <= N <= min(4, K)")
    records = cloud = device_traj = sweep_report = None
    cloud_args = (a.cloud_stride, CLOUD_MODES[a.cloud_mode]) if a.cloud else None
    if seeded:
        poses, stats, device_traj, keyframes = track_keyframes(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, over,
                                                               max(1, a.keyframe_interval), a.motion_model, a.handoff, a.jacobian)
        if a.sweep_depth:
            capi = importlib.import_module("uw-slam_amd.capi")
            z_near, z_far = [float(v) for v in a.sweep_range.split(",")]
            codes = capi.sweep_hypotheses(z_near, z_far, 0.0002, a.sweep_hyp)
            sweep_planes, sweep_report = sweep_keyframes(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, poses, keyframes,
                                                         a.sweep_depth, codes, over["arith"])
            np.save(a.out + "_sweep_depth.npy", sweep_planes)
    elif a.live and a.chained and (a.quality or a.cloud):
        res = track_live_chained(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, over["arith"],
                                 detector=int(a.detector == "orb"), quality=a.quality, cloud=cloud_args, motion_model=a.motion_model,
                                 jacobian=a.jacobian)
        poses, stats, n_matches = res[:3]
        records = res[3] if a.quality else None
        cloud = res[-1] if a.cloud else None
    elif a.live:
        if a.chained:
            poses, stats, n_matches = track_live_chained(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, over["arith"],
                                                         detector=int(a.detector == "orb"), motion_model=a.motion_model, jacobian=a.jacobian)
        else:
            poses, stats, n_matches = track_live(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, over["arith"],
                                                 detector=int(a.detector == "orb"), jacobian=a.jacobian)
    else:
        poses, stats = trk.track(frames, depths)
    if a.quality and records is None:
        records = sequence_quality(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, np.asarray(poses, np.float32), over["arith"])
    if a.cloud and cloud is None:
        cloud = sequence_cloud(a.width, a.height, (fx, fy, cx - x0, cy - y0), frames, depths, poses, *cloud_args, arith=over["arith"])
    dt = time.perf_counter() - t0
    if device_traj is not None and a.keyframe_interval > 1:
        # keyframe-relative poses: the trajectory is the one accumulated on the device through the keyframes' rows; the visualiser's
        # scaled accumulation (src/Visualizer.cpp:304-325) is defined over consecutive pairs and has no keyframe form
        traj = ref = device_traj
        if a.groundtruth:
            ap.error("--groundtruth compares per-pair poses of consecutive frames: not with --keyframe-interval above 1")
        np.save(a.out + "_keyframes.npy", np.asarray(keyframes, np.int32))
    else:
        traj = trk.trajectory(poses)
        ref = trk.trajectory(poses, reference_visualiser=True)
    if device_traj is not None:
        np.save(a.out + "_trajectory.npy", device_traj)
    gt = None
    bad = sum(s["status"] != 0 for s in stats)
    metrics = dict(pairs=int(len(poses)), failed=int(bad), seconds=dt, crop_offset=[int(x0), int(y0)],
                   iterations=[int(s["iterations"]) for s in stats])
    if a.live:
        metrics["n_matches"] = n_matches
    if a.quality:
        metrics["quality"] = quality_columns(records, a.width, a.height)
        q = metrics["quality"]
        print("coverage %.3f, mean |difference| %.2f aligned against %.2f unaligned (means over %d pairs)"
              % (np.mean(q["coverage"]), np.mean(q["mean_abs"]), np.mean(q["mean_abs_unaligned"]), len(poses)))
    if sweep_report is not None:
        metrics["sweep_depth"] = sweep_report
        for r in sweep_report:
            print("keyframe %d from frames %s: coverage %.3f, %d selected, outcomes %s" % (r["keyframe"], r["views"], r["coverage"],
                                                                                         r["n_selected"], r["outcomes"][1:]))
    if a.cloud:
        metrics["cloud_points"] = int(cloud.size)
        T.write_ply(a.cloud, cloud)
        print("%d cloud points (every %d-th row, %s) in %s" % (cloud.size, a.cloud_stride, a.cloud_mode, a.cloud))
    if a.groundtruth:
        ts, gtp = (T.read_groundtruth_euroc if a.euroc else T.read_groundtruth_tum)(a.groundtruth)
        idx_all = np.clip(T.ground_truth_indices(len(gtp), len(names), a.start, euroc=a.euroc), 0, len(gtp) - 1)
        gt = gtp[idx_all[1:]]
        # The files hold camera-to-world poses G_k; the tracker's pose of pair k maps the previous camera's coordinates to
        # the current one's, T_k = G_{k+1}^-1 G_k.  RPE: per-pair estimate against that; ATE: the camera trajectory the
        # estimates imply, C_{k+1} = C_k T_k^-1, against G_0^-1 G_k after a rigid alignment.  (The Visualizer-style
        # accumulation previous * SE3(q, t) stays a separate output: <out>_tum.txt / <out>_reference.csv.)
        g_pair = T.pair_ground_truth(gtp[idx_all])
        cam = T.camera_trajectory(poses)
        metrics["ate_rmse_m"] = S.ate_rmse(cam[:, 4:], T.from_first(gtp[idx_all])[:, 4:])
        metrics["rpe_trans_rmse_m"] = S.rpe_translation(poses[:, 4:], g_pair[:, 4:])
        metrics["rpe_rot_rmse_rad"] = T.rpe_rotation(poses, g_pair)
        np.savetxt(a.out + "_camera_tum.txt", np.concatenate([np.arange(1, len(cam) + 1)[:, None], cam[:, 4:], cam[:, :4]], axis=1), fmt="%.9g")
        print("ATE RMSE %.4f m, RPE %.5f m / %.5f rad over %d poses"
              % (metrics["ate_rmse_m"], metrics["rpe_trans_rmse_m"], metrics["rpe_rot_rmse_rad"], len(traj)))
    T.write_reference_csv(a.out + "_reference.csv", ref, gt)
    T.write_tum(a.out + "_tum.txt", np.arange(len(traj), dtype=np.float64), traj)
    np.save(a.out + "_poses.npy", poses)
    import json
    with open(a.out + "_metrics.json", "w") as f:
        json.dump(metrics, f)
    print("%d pairs in %.3f s (%.1f pairs/s incl. upload), %d failed; wrote %s_reference.csv, %s_tum.txt"
          % (len(poses), dt, len(poses) / dt, bad, a.out, a.out))


if __name__ == "__main__":
    main()
