"""Nothing written or read outside the extents: every entry point that takes caller DEVICE pointers, run on buffers cut out of a
guarded arena (tests/guard_bands.py) at exactly the alignment include/uwt.h states for the pointer, under two fills of everything the
call must not depend on.  Every guard byte is checked, every output byte must be the same under both fills, and the outputs must be the
bytes of the synchronous host form of the same call (which the other test files pin to the restatements).  The rows past a count must
hold what they held.  Frames are 165 x 99 with 3 levels (pitch 168, a masked last group, odd rows on every level) and 160 x 96 where a
whole-group level takes another kernel form; three pairs or frames in a context made for eight, so that the last pair's end is the
buffer's end and not the end of an allocation the library made."""
import importlib

import numpy as np
import pytest

import guard_bands as GB
import orb_cases
import ransac_cases
import surf_cases
import test_gpu_cloud as TC
import test_gpu_warp_image as TW

ARITH_INDEPENDENT = True   # where a store lands does not depend on the arithmetic set
OK, CAPACITY = 0, 5
SIZES = [(165, 99), (160, 96)]
REF, TGT = [0, 2, 0], [1, 3, 3]
ALIGN = dict(poses=4, stats=4, kp=4, match=4, counts=4, desc=16, desc_out=4, mask=1, ransac_info=8, track_info=4, plane=4, quality=8, cloud=16,
             cloud_info=8)   # include/uwt.h, "Alignment of device pointers"


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def backend():
    return GB.TorchBackend(importlib.import_module("torch"))


def tracker_ctx(capi, synth, w, h, **over):
    """the four frames of the warp tests with depth, pyramids and gradients, in a context for eight pairs; a fixed schedule"""
    ctx, gt = TW.make_ctx(capi, synth, w, h, True, max_pairs=8, gradients=True)
    ctx.update_params(max_iters=4, early_exit=0, **over)
    return ctx, gt


def stats_bytes(capi, stats):
    out = np.zeros(len(stats), capi.STATS)
    for i, s in enumerate(stats):
        for k in ("status", "iterations", "n_valid", "error"):
            out[i][k] = s[k]
    return out.tobytes()


def rows_and_rest(raw, dtype, P, cap, counts):
    """a P x cap record buffer as (the rows below each count, whether every byte past them still holds the output fill)"""
    a = np.frombuffer(raw, np.uint8).reshape(P, cap, np.dtype(dtype).itemsize)
    return [a[i, :counts[i]].tobytes() for i in range(P)], all((a[i, counts[i]:] == GB.OUT_FILL).all() for i in range(P))


def not_a_multiple_of_4(n):
    return n if n % 4 else n + 1


# ---- the trackers: poses and stats ------------------------------------------------------------------------------------------------------
def pose_specs():
    return [GB.Buf("poses", nbytes=3 * 28, align=ALIGN["poses"], stride=28), GB.Buf("stats", nbytes=3 * 16, align=ALIGN["stats"], stride=16)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_track_batch_async(capi, synth, backend, w, h):
    ctx, _ = tracker_ctx(capi, synth, w, h)
    want, wst = ctx.estimate_pose_batch(REF, TGT)
    outs = GB.run_twice(backend, pose_specs(), lambda a: (ctx.track_batch_async(0, 4, REF, TGT, a.ptr("poses"), a.ptr("stats"),
                                                                                grad_refs_only=False), ctx.sync()))
    assert outs["poses"] == want[:3].tobytes() and outs["stats"] == stats_bytes(capi, wst[:3])
    assert all(s["status"] == OK for s in wst[:3])
    ctx.close()


def feature_keypoints(w, h):
    rng = np.random.default_rng(3)
    kp = [rng.uniform([6, 6], [w - 7, h - 7], (n, 2)).astype(np.float32) for n in (60, 7, 200)]
    kp[2][:4] = np.array([[0, 0], [w - 1, h - 1], [2.5, h - 3.0], [w - 0.5, 4.0]], np.float32)   # patches cut by the image edge
    return kp


@pytest.mark.gpu
@pytest.mark.parametrize("weights,sampler", [(None, None), (2, 0), (2, 1)])
def test_gpu_track_features_batch_async_and_opt(capi, synth, backend, weights, sampler):
    w, h = 165, 99
    ctx, _ = tracker_ctx(capi, synth, w, h)
    kps = feature_keypoints(w, h)
    want, wst = ctx.estimate_pose_features_batch(REF, TGT, kps, weights=weights, sampler=sampler)
    outs = GB.run_twice(backend, pose_specs(), lambda a: (ctx.track_features_batch_async(REF, TGT, kps, a.ptr("poses"), a.ptr("stats"),
                                                                                         weights=weights, sampler=sampler), ctx.sync()))
    assert outs["poses"] == want[:3].tobytes() and outs["stats"] == stats_bytes(capi, wst[:3])
    assert all(s["status"] == OK and s["n_valid"] > 0 for s in wst[:3])
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("weights,sampler", [(None, None), (2, 0), (2, 1)])
def test_gpu_track_candidates_batch_async_and_opt(capi, synth, backend, w, h, weights, sampler):
    ctx, _ = tracker_ctx(capi, synth, w, h)
    want, wst = ctx.estimate_pose_candidates_batch(REF, TGT, threshold=5.0, weights=weights, sampler=sampler)
    outs = GB.run_twice(backend, pose_specs(), lambda a: (ctx.track_candidates_batch_async(REF, TGT, a.ptr("poses"), a.ptr("stats"),
                                                                                           threshold=5.0, weights=weights, sampler=sampler),
                                                          ctx.sync()))
    assert outs["poses"] == want[:3].tobytes() and outs["stats"] == stats_bytes(capi, wst[:3])
    assert all(s["status"] == OK and s["n_valid"] > 0 for s in wst[:3])
    ctx.close()


# ---- the chained tracking calls: all seven outputs, and the hand-over out of the arena -------------------------------------------------------
def tracking_specs(tag, P, cap):
    rec = lambda name, size, align: GB.Buf(tag + name, nbytes=P * cap * size, align=align, stride=cap * size)
    return [GB.Buf(tag + "poses", nbytes=P * 28, align=ALIGN["poses"], stride=28), GB.Buf(tag + "stats", nbytes=P * 16, align=ALIGN["stats"]),
            GB.Buf(tag + "info", nbytes=P * 32, align=ALIGN["track_info"]), rec("good", 12, ALIGN["match"]), rec("kept_prev", 32, ALIGN["kp"]),
            rec("kept_cur", 32, ALIGN["kp"]), GB.Buf(tag + "n_matches", nbytes=P * 4, align=ALIGN["counts"])]


def tracking_io(a, tag, prev=None):
    io = {k: a.ptr(tag + k) for k in ("poses", "stats", "info", "good", "kept_prev", "kept_cur", "n_matches")}
    if prev:
        io["prev_kp"], io["n_prev"] = a.ptr(prev + "kept_cur"), a.ptr(prev + "n_matches")
    return io


def check_tracking(capi, outs, tag, want, P, cap):
    cnt = [int(n) for n in want["info"]["n_matches"][:P]]
    assert outs[tag + "poses"] == want["poses"][:P].tobytes() and outs[tag + "stats"] == want["stats"][:P].tobytes()
    assert outs[tag + "info"] == want["info"][:P].tobytes() and np.frombuffer(outs[tag + "n_matches"], np.int32).tolist() == cnt
    for k, dt in (("good", capi.MATCH), ("kept_prev", capi.KEYPOINT), ("kept_cur", capi.KEYPOINT)):
        rows, rest = rows_and_rest(outs[tag + k], dt, P, cap, cnt)
        assert rows == [want[k][i].tobytes() for i in range(P)], (tag, k)
        assert rest, (tag, k, "rows past a pair's count were written")


def run_tracking_chain(capi, synth, backend, sync_form, async_form, params_of):
    """Two calls in one arena: pairs (0, 3), (0, 1), (2, 3) — the unrelated pair first, so that the LAST pair's lists are not empty —, then,
    from what the current frames kept, (3, 0), (1, 0), (3, 2) with the first call's d_kept_cur / d_n_matches as d_prev_kp / d_n_prev.
    Capacities, learnt from a run at 2048: the largest key-point count made no multiple of 4 (nothing is cut: the bytes are the large
    run's), then the last pair's key-point counts on either side and each of them minus 1 — detection has capacity cap (the header's step
    2), so the ordered cut runs on the last pair's frames inside the chain; the reference is the synchronous form at the same cap.
    At every capacity the second call also runs alone with d_prev_kp / d_n_prev as INPUTS of the arena, the rows past each d_n_prev
    under the two fills."""
    ctx, _ = tracker_ctx(capi, synth, 165, 99)
    tp = params_of(min_matches=3)
    REF, TGT = [0, 0, 2], [3, 1, 3]
    ref2, tgt2 = TGT, REF
    big = sync_form(ctx)(REF, TGT, params=tp, cap=2048)
    big2 = sync_form(ctx)(ref2, tgt2, prev=big["kept_cur"], params=tp, cap=2048)
    most = max(int(r["info"][k].max()) for r in (big, big2) for k in ("n_kp_prev", "n_kp_cur"))
    last = [int(big["info"][k][2]) for k in ("n_kp_prev", "n_kp_cur")]
    caps = sorted({not_a_multiple_of_4(most), last[0], last[0] - 1, last[1], last[1] - 1}, reverse=True)
    print("key points", big["info"]["n_kp_prev"], big["info"]["n_kp_cur"], "matches", big["info"]["n_matches"], big2["info"]["n_matches"],
          "used", big2["info"]["used_provided"], "caps", caps)
    assert big["info"]["n_matches"][2] > 0 and big2["info"]["n_matches"][2] > 0 and big2["info"]["used_provided"].any() and most < 2048
    assert min(last) > 8
    for cap in caps:
        want = sync_form(ctx)(REF, TGT, params=tp, cap=cap)
        want2 = sync_form(ctx)(ref2, tgt2, prev=want["kept_cur"], params=tp, cap=cap)
        if cap >= most:
            for a, b in ((want, big), (want2, big2)):
                assert a["info"].tobytes() == b["info"].tobytes() and a["poses"].tobytes() == b["poses"].tobytes()
                assert all(a[k][i].tobytes() == b[k][i].tobytes() for k in ("good", "kept_prev", "kept_cur") for i in range(3))
        else:   # below the last pair's larger count the cut ran there: that set holds cap rows, fewer than its frame has
            assert [int(want["info"][k][2]) for k in ("n_kp_prev", "n_kp_cur")] == [min(n, cap) for n in last]

        def call(a):
            async_form(ctx)(REF, TGT, tracking_io(a, "a_"), params=tp, cap=cap)
            async_form(ctx)(ref2, tgt2, tracking_io(a, "b_", prev="a_"), params=tp, cap=cap)
            ctx.sync()

        outs = GB.run_twice(backend, tracking_specs("a_", 3, cap) + tracking_specs("b_", 3, cap), call)
        check_tracking(capi, outs, "a_", want, 3, cap)
        check_tracking(capi, outs, "b_", want2, 3, cap)
        # the second call alone, its provided lists inputs: nothing may depend on the rows past d_n_prev
        n_prev = np.array([len(k) for k in want["kept_cur"]], np.int32)
        prev = np.zeros((3, cap), capi.KEYPOINT)
        for i, k in enumerate(want["kept_cur"]):
            prev[i, :len(k)] = k
        dead = [(i * cap * 32 + int(n_prev[i]) * 32, (i + 1) * cap * 32) for i in range(3)]
        specs = [GB.Buf("prev_kp", data=prev, align=ALIGN["kp"], stride=cap * 32, dead=dead), GB.Buf("n_prev", data=n_prev, align=ALIGN["counts"])]

        def second(a):
            io = tracking_io(a, "b_")
            io["prev_kp"], io["n_prev"] = a.ptr("prev_kp"), a.ptr("n_prev")
            async_form(ctx)(ref2, tgt2, io, params=tp, cap=cap)
            ctx.sync()

        outs = GB.run_twice(backend, specs + tracking_specs("b_", 3, cap), second)
        check_tracking(capi, outs, "b_", want2, 3, cap)
    ctx.close()


@pytest.mark.gpu
def test_gpu_tracking_batch_async(capi, synth, backend):
    run_tracking_chain(capi, synth, backend, lambda c: c.tracking_batch, lambda c: c.tracking_batch_async, capi.default_tracking_params)


@pytest.mark.gpu
def test_gpu_tracking_orb_batch_async(capi, synth, backend):
    run_tracking_chain(capi, synth, backend, lambda c: c.tracking_orb_batch, lambda c: c.tracking_orb_batch_async,
                       capi.default_tracking_orb_params)


# ---- descriptor matching ----------------------------------------------------------------------------------------------------------------------
MATCH_ROWS = [(63, 64), (65, 130), (130, 63)]   # 63, 64, 65 and 130 rows across the pairs; cap = the largest, on the last pair's query set


def match_pairs(synth, kind):
    dim = 64 if kind == "l2" else 32
    return [synth.descriptor_pair(70 + i, n, m, dim, kind)[:2] for i, (n, m) in enumerate(MATCH_ROWS)], dim


def check_matches(capi, outs, want, P, cap):
    cnt = [len(m) for m in want]
    assert np.frombuffer(outs["counts"], np.int32).tolist() == cnt and sum(cnt) > 20
    rows, rest = rows_and_rest(outs["matches"], capi.MATCH, P, cap, cnt)
    assert rows == [m.tobytes() for m in want] and rest


def match_out_specs(P, cap):
    return [GB.Buf("matches", nbytes=P * cap * 12, align=ALIGN["match"], stride=cap * 12), GB.Buf("counts", nbytes=P * 4, align=ALIGN["counts"])]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l2", "hamming"])
def test_gpu_match_descriptors_batch_async(capi, synth, backend, kind):
    ctx = capi.Context(capi.default_params(165, 99, *TW.INTR[(165, 99)], max_frames=2, max_pairs=8, n_levels=3, first_level=2, last_level=0))
    pairs, _ = match_pairs(synth, kind)
    cap = 130
    want = ctx.match_descriptors_batch(pairs, cap=cap)
    outs = GB.run_twice(backend, match_out_specs(3, cap),
                        lambda a: (ctx.match_descriptors_batch_async(a.ptr("matches"), a.ptr("counts"), pairs, cap=cap), ctx.sync()))
    check_matches(capi, outs, want, 3, cap)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l2", "hamming"])
def test_gpu_match_descriptors_device_async(capi, synth, backend, kind):
    ctx = capi.Context(capi.default_params(165, 99, *TW.INTR[(165, 99)], max_frames=2, max_pairs=8, n_levels=3, first_level=2, last_level=0))
    pairs, dim = match_pairs(synth, kind)
    cap = 130
    norm, dim, cap, q, nq, t, nt = ctx._descriptor_block(pairs, None, cap)
    row = dim * q.dtype.itemsize
    dead = lambda n: [(p * cap * row + int(n[p]) * row, (p + 1) * cap * row) for p in range(3)]
    specs = [GB.Buf("query", data=q, align=ALIGN["desc"], stride=cap * row, dead=dead(nq)), GB.Buf("n_query", data=nq, align=ALIGN["counts"]),
             GB.Buf("train", data=t, align=ALIGN["desc"], stride=cap * row, dead=dead(nt)), GB.Buf("n_train", data=nt, align=ALIGN["counts"])]
    want = ctx.match_descriptors_batch(pairs, cap=cap)
    outs = GB.run_twice(backend, specs + match_out_specs(3, cap), lambda a: (ctx.match_descriptors_device_async(
        3, dim, cap, a.ptr("query"), a.ptr("n_query"), a.ptr("train"), a.ptr("n_train"), a.ptr("matches"), a.ptr("counts"), norm=norm), ctx.sync()))
    check_matches(capi, outs, want, 3, cap)
    ctx.close()


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("counts,cap", [((0, 7, 8), 8), ((7, 0, 45), 45), ((8, 45, 44), 45), ((45, 8, 47), 47)])
def test_gpu_ransac_inliers_batch_async(capi, backend, counts, cap):
    """0, 7 (below the sample) and 8 matches, and a last pair that fills its cap; then the last pair one row short of a cap that is no
    multiple of 4, and filling one"""
    ctx = capi.Context(capi.default_params(165, 99, *TW.INTR[(165, 99)], max_frames=2, max_pairs=8, n_levels=3, first_level=2, last_level=0))
    pairs = [ransac_cases.scene(40 + i, n, 0.3 if n >= 30 else 0.0, 0.3)[:3] for i, n in enumerate(counts)]
    want = ctx.ransac_inliers_batch(pairs, cap=cap, kp_cap=cap)
    _, kp_cap, mt, nm, *_ = capi.Context._ransac_block(pairs, cap, cap)
    dead = [(p * cap * 12 + int(nm[p]) * 12, (p + 1) * cap * 12) for p in range(3)]
    specs = [GB.Buf("matches", data=mt, align=ALIGN["match"], stride=cap * 12, dead=dead), GB.Buf("n_matches", data=nm, align=ALIGN["counts"]),
             GB.Buf("mask", nbytes=3 * cap, align=ALIGN["mask"], stride=cap), GB.Buf("good", nbytes=3 * cap * 12, align=ALIGN["match"], stride=cap * 12),
             GB.Buf("counts", nbytes=12, align=ALIGN["counts"]), GB.Buf("info", nbytes=3 * 88, align=ALIGN["ransac_info"], stride=88)]
    outs = GB.run_twice(backend, specs, lambda a: (ctx.ransac_inliers_batch_async(
        a.ptr("matches"), a.ptr("n_matches"), cap, [p[1:] for p in pairs], a.ptr("mask"), a.ptr("good"), a.ptr("counts"), a.ptr("info"),
        kp_cap=kp_cap), ctx.sync()))
    kept = [len(w[1]) for w in want]
    assert np.frombuffer(outs["counts"], np.int32).tolist() == kept and (max(counts) < 30 or sum(kept) > 8)
    rows, rest = rows_and_rest(outs["mask"], np.uint8, 3, cap, list(counts))
    assert rows == [w[0].tobytes() for w in want] and rest
    rows, rest = rows_and_rest(outs["good"], capi.MATCH, 3, cap, kept)
    assert rows == [w[1].tobytes() for w in want] and rest
    assert outs["info"] == b"".join(w[2].tobytes() for w in want)
    ctx.close()


# ---- SURF and ORB ------------------------------------------------------------------------------------------------------------------------------
def run_detector(capi, backend, frames, sync_name, async_name, desc_row):
    w, h = 165, 99
    ctx = capi.Context(capi.default_params(w, h, *TW.INTR[(w, h)], max_frames=4, max_pairs=8, n_levels=3, first_level=2, last_level=0))
    ctx.upload_frames(0, np.stack(frames))
    slots = [0, 1, 2]
    full = getattr(ctx, sync_name)(slots, cap=2048)
    n = [len(kp) for kp, _ in full]
    print(sync_name, "key points", n)
    assert min(n) > 8 and max(n) < 2048
    last = n[2]
    caps = sorted({max(n), last, last - 1, not_a_multiple_of_4(last // 2)}, reverse=True)   # below last: the selection's cut runs on the last frame
    for cap in caps:
        want = getattr(ctx, sync_name)(slots, cap=cap)
        cnt = [len(kp) for kp, _ in want]
        assert cnt == [min(k, cap) for k in n]
        if cap >= max(n):   # nothing cut: the large-capacity run's bytes
            assert all(want[f][0].tobytes() == full[f][0].tobytes() and want[f][1].tobytes() == full[f][1].tobytes() for f in range(3))
        specs = [GB.Buf("kp", nbytes=3 * cap * 32, align=ALIGN["kp"], stride=cap * 32),
                 GB.Buf("desc", nbytes=3 * cap * desc_row, align=ALIGN["desc_out"], stride=cap * desc_row), GB.Buf("counts", nbytes=12, align=ALIGN["counts"])]
        outs = GB.run_twice(backend, specs, lambda a: (getattr(ctx, async_name)(slots, a.ptr("kp"), a.ptr("desc"), a.ptr("counts"), cap=cap),
                                                       ctx.sync()))
        assert np.frombuffer(outs["counts"], np.int32).tolist() == cnt, cap
        rows, rest = rows_and_rest(outs["kp"], capi.KEYPOINT, 3, cap, cnt)
        assert rows == [want[f][0].tobytes() for f in range(3)], cap
        assert rest, (cap, "key-point rows past a frame's count were written")
        rows, rest = rows_and_rest(outs["desc"], np.dtype((np.uint8, desc_row)), 3, cap, cnt)
        assert rows == [want[f][1].tobytes() for f in range(3)], cap
        assert rest, (cap, "descriptor rows past a frame's count were written")
    ctx.close()


@pytest.mark.gpu
def test_gpu_surf_detect_describe_batch_async(capi, backend):
    run_detector(capi, backend, [surf_cases.texture(165, 99, s) for s in (3, 4, 21)], "surf_detect_describe_batch",
                 "surf_detect_describe_batch_async", 256)


@pytest.mark.gpu
def test_gpu_orb_detect_describe_batch_async(capi, backend):
    run_detector(capi, backend, [orb_cases.frame_of(s, 165, 99) for s in ("t3", "t4", "t21")], "orb_detect_describe_batch",
                 "orb_detect_describe_batch_async", 32)


# ---- the image warp --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("lvl", [0, 2])
def test_gpu_warp_image_batch_async(capi, synth, backend, w, h, lvl):
    ctx, gt = tracker_ctx(capi, synth, w, h)
    poses = np.stack([gt, TW.ROLL, TW.CONTRACT])   # the contracting pose (many rows per pixel) on the last pair
    L = ctx.level_info(lvl)
    plane = L.pitch * L.img_h
    want = ctx.warp_image_batch(REF, TGT, poses, lvl=lvl)
    assert want["status"] == OK and (want["quality"]["n_landed"] > want["quality"]["n_covered"])[2]
    specs = [GB.Buf("poses", data=poses, align=ALIGN["poses"], stride=28)]
    specs += [GB.Buf(k, nbytes=3 * plane, align=ALIGN["plane"], stride=plane) for k in ("warped", "valid", "absdiff")]
    specs += [GB.Buf("quality", nbytes=3 * 48, align=ALIGN["quality"], stride=48)]
    outs = GB.run_twice(backend, specs, lambda a: (ctx.warp_image_batch_async(
        REF, TGT, a.ptr("poses"), {k: a.ptr(k) for k in ("warped", "valid", "absdiff", "quality")}, lvl=lvl), ctx.sync()))
    assert outs["quality"] == want["quality"].tobytes()
    for k in ("warped", "valid", "absdiff"):
        got = np.frombuffer(outs[k], np.uint8).reshape(3, L.img_h, L.pitch)
        assert got[:, :, :L.img_w].tobytes() == want[k].tobytes(), k
    ctx.close()


# ---- the cloud and the trajectory -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", [0, 1])
@pytest.mark.parametrize("skip", [0, 1])
def test_gpu_point_cloud_batch_async(capi, synth, backend, source, skip):
    w, h = 165, 99
    intr = TW.INTR[(w, h)]
    frames, depths = TC.scene(synth, w, h)   # zero-depth rows, blocks and corners cut into every frame's depth: rows to skip
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=4, max_pairs=8, n_levels=3, first_level=2, last_level=0, has_depth=1))
    ctx.upload_frames(0, np.stack(frames), np.stack(depths))
    ctx.build_pyramids(0, 4)
    ctx.apply_gradient(0, 4)
    slots = [0, 2, 3]
    traj = TC.poses_for(3)
    for stride in (1, 7):
        p = capi.default_cloud_params(mode=1, stride=stride, skip_invalid=skip, source=source, threshold=TC.THRESHOLD)
        full = ctx.point_cloud_batch(slots, traj, p)
        total = int(full["call"]["offset"])
        last = full["info"][2]
        assert full["status"] == OK and total == len(full["points"]) and int(last["n_points"]) > 8
        inside = int(last["offset"]) + 2 * int(last["n_points"]) // 3   # inside the last frame, inside a block; no multiple of 64
        inside += 1 if inside % 64 == 0 else 0
        assert inside % 64 and int(last["offset"]) < inside < total - 1
        for cap in (total, total - 1, inside, 0):
            want = ctx.point_cloud_batch(slots, traj, p, cap=cap)
            assert want["status"] == (OK if cap == total else CAPACITY) and want["points"].tobytes() == full["points"][:cap].tobytes()
            specs = [GB.Buf("traj", data=traj, align=ALIGN["poses"], stride=28),
                     GB.Buf("info", nbytes=4 * 32, align=ALIGN["cloud_info"], stride=32)]
            if cap:
                specs.append(GB.Buf("points", nbytes=cap * 16, align=ALIGN["cloud"], stride=cap * 16))
            outs = GB.run_twice(backend, specs, lambda a: (ctx.point_cloud_batch_async(
                slots, a.ptr("traj"), a.ptr("points") if cap else None, cap, a.ptr("info"), p), ctx.sync()))
            assert outs["info"] == want["info"].tobytes() + want["call"].tobytes(), (stride, cap)
            if cap:
                assert outs["points"] == full["points"][:cap].tobytes(), (stride, cap)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_gpu_accumulate_trajectory_device_async_and_from(capi, backend, n):
    ctx = capi.Context(capi.default_params(165, 99, *TW.INTR[(165, 99)], max_frames=2, max_pairs=8, n_levels=3, first_level=2, last_level=0))
    rng = np.random.default_rng(n)
    poses = np.concatenate([rng.normal(0, 0.05, (2 * n, 3)), 1 + rng.normal(0, 0.05, (2 * n, 1)), rng.normal(0, 0.01, (2 * n, 3))], 1).astype(np.float32)
    start = np.array([0.1, 0.2, -0.1, 0.9, 1.0, -2.0, 0.5], np.float32)
    want = ctx.accumulate_trajectory(poses, start=start, t_scale=40.0, reference_axes=False)
    specs = [GB.Buf("poses", data=poses[:n], align=ALIGN["poses"], stride=28), GB.Buf("more", data=poses[n:], align=ALIGN["poses"], stride=28),
             GB.Buf("traj", nbytes=n * 28, align=ALIGN["poses"], stride=28), GB.Buf("traj2", nbytes=n * 28, align=ALIGN["poses"], stride=28)]

    def call(a):   # the second call starts from the first call's last row, in the same arena
        ctx.accumulate_trajectory_device_async(a.ptr("poses"), n, a.ptr("traj"), start=start, t_scale=40.0)
        ctx.accumulate_trajectory_device_from_async(a.ptr("more"), n, a.ptr("traj", 28 * (n - 1)), a.ptr("traj2"), t_scale=40.0)
        ctx.sync()

    outs = GB.run_twice(backend, specs, call)
    assert outs["traj"] == want[:n].tobytes() and outs["traj2"] == want[n:].tobytes()
    ctx.close()


# ---- guards inside the context's own scratch (uwt_debug_guards / uwt_debug_check_guards) --------------------------------------------------
GUARD = 256


def frozen(x):
    """a result of any wrapper as nested tuples of bytes and plain values"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.generic):
        return x.tobytes()
    return x


def same_with_guards(ctx, run):
    """run() with the guards off, then on: no gap damaged, and every output bit for bit the same; the context is left with guards off"""
    ctx.debug_guards(0)
    off = frozen(run())
    ctx.debug_guards(GUARD)
    on = frozen(run())
    damaged, where = ctx.debug_check_guards()
    ctx.debug_guards(0)
    assert damaged == 0, where
    assert on == off
    assert ctx.debug_check_guards() == (0, "")   # guards off: nothing recorded, nothing to report


def jacobian_case(ctx, pose):
    r = ctx.residual_jacobian(0, 1, 1, pose)
    v = r["valid"] != 0
    return dict(A=r["A"], jtr=r["jtr"], sum_r2=r["sum_r2"], n_valid=r["n_valid"], valid=r["valid"], J=r["J"][v], r=r["r"][v])


def gn_update_case(ctx):
    """uwt_gn_update_records in both forms: 3 pairs behind a pair_base of 2, 17 records of a stride of 20"""
    import gn_update_cases as GC
    import gn_update_ref as GR
    recs = np.zeros((5, 20, GR.REC_WORDS), np.uint32)
    for p in range(5):
        recs[p, :17] = GC.fold_records(17, seed=p)
    states = np.array([GR.state(iters=p) for p in range(5)], GR.STATE_DTYPE)
    out = []
    for form in (0, 1):
        r = recs[:, :17] if form == 0 else recs
        st, active, tickets = ctx.gn_update_records(form, r, states, 17, pair_base=2, early_exit=0)
        out += [st.view(np.uint8), active, tickets]
    return out


def scratch_cases(capi, synth, ctx, gt):
    """name -> a call of one stage that owns a growable block (or carves the shared scratch), on the 165 x 99 frames"""
    w, h = 165, 99
    frames, depths, _ = TW.scene(synth, w, h, True)
    rng = np.random.default_rng(9)
    kps = feature_keypoints(w, h)
    l2, _ = match_pairs(synth, "l2")
    ham, _ = match_pairs(synth, "hamming")
    ransac = [ransac_cases.scene(40 + i, n, 0.3 if n >= 30 else 0.0, 0.3)[:3] for i, n in enumerate((8, 45, 44))]
    poses = np.stack([gt, TW.ROLL, TW.CONTRACT])
    L0 = ctx.level_info(0)
    table = np.stack([rng.uniform(0, w - 1, 500), rng.uniform(0, h - 1, 500), rng.uniform(0.5, 2, 500), np.ones(500)], 1).astype(np.float32)
    cand = ctx.obtain_candidate_points(0, 0, 5.0)[0]
    J, r, wt = rng.normal(0, 1, (64, 6)).astype(np.float32), rng.normal(0, 1, 64).astype(np.float32), rng.uniform(0, 1, 64).astype(np.float32)
    A = (J.T @ J).astype(np.float32)
    cloud = capi.default_cloud_params(mode=1, stride=7, skip_invalid=1, source=1, threshold=5.0)
    tp, tpo = capi.default_tracking_params(min_matches=3), capi.default_tracking_orb_params(min_matches=3)

    def match_device():
        return device_match_outputs(capi, ctx, l2)

    def cloud_async():
        torch = importlib.import_module("torch")
        d_traj = torch.from_numpy(TC.poses_for(3)).cuda()
        d_pts = torch.zeros((4096, 16), dtype=torch.uint8, device="cuda")
        d_info = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.point_cloud_batch_async([0, 2, 3], d_traj.data_ptr(), d_pts.data_ptr(), 4096, d_info.data_ptr(), cloud)
        ctx.sync()
        return d_pts.cpu().numpy(), d_info.cpu().numpy()

    return {
        "candidates_batch": lambda: ctx.estimate_pose_candidates_batch(REF, TGT, threshold=5.0),
        "candidates_batch_huber_bilinear": lambda: ctx.estimate_pose_candidates_batch(REF, TGT, threshold=5.0, weights=2, sampler=1),
        "features_batch_weights": lambda: ctx.estimate_pose_features_batch(REF, TGT, kps, weights=2, sampler=0),
        "dense_batch": lambda: ctx.estimate_pose_batch(REF, TGT),
        "knn_l2": lambda: ctx.knn_match_batch(l2, cap=130),
        "match_host_l2": lambda: ctx.match_descriptors_batch(l2, cap=130),
        "match_host_hamming": lambda: ctx.match_descriptors_batch(ham, cap=130),
        "match_device_l2": match_device,
        "ransac": lambda: ctx.ransac_inliers_batch(ransac, cap=45, kp_cap=45),
        "surf": lambda: ctx.surf_detect_describe_batch([0, 2, 3], cap=61),
        "surf_describe": lambda: ctx.surf_describe_batch([0, 2], [surf_cases.border_keypoints(w, h)] * 2),
        "surf_stages": lambda: (ctx.surf_integral(1), ctx.surf_response_layer(1, 0, 1)),
        "orb": lambda: ctx.orb_detect_describe_batch([0, 2, 3], cap=61),
        "orb_stages": lambda: (ctx.orb_layer(1, 1), ctx.orb_fast_scores(1, 0), ctx.orb_harris(1, 0, [[40, 40], [100, 50], [7, 90]])),
        "tracking_surf": lambda: ctx.tracking_batch(REF, TGT, params=tp, cap=61),
        "tracking_orb": lambda: ctx.tracking_orb_batch(REF, TGT, params=tpo, cap=61),
        "warp_explicit": lambda: ctx.obtain_image_transformed(0, 0, cand, ctx.warp(0, cand, gt)),
        "warp_batch": lambda: ctx.warp_image_batch(REF, TGT, poses, lvl=0),
        "warp_batch_level_2": lambda: ctx.warp_image_batch(REF, TGT, poses, lvl=2),
        "warp_mosaic": lambda: ctx.warp_mosaic(0, 1, 0, frames[0]),
        "cloud_batch": lambda: ctx.point_cloud_batch([0, 2, 3], TC.poses_for(3), cloud),
        "cloud_batch_cut": lambda: ctx.point_cloud_batch([0, 2, 3], TC.poses_for(3), cloud, cap=101),   # the cloud ends inside a frame
        "cloud_batch_async": cloud_async,
        "cloud_points": lambda: ctx.point_cloud_points(0, table, TC.poses_for(1)[0], capi.default_cloud_params(stride=3, skip_invalid=1)),
        "stage_resize": lambda: (ctx.resize_half_u8(frames[0]), ctx.resize_half_u16(depths[0]), ctx.halve_u8(frames[0][:98, :164]),
                                 ctx.halve_u16(depths[0][:98, :164])),
        "stage_scharr": lambda: ctx.scharr3(frames[1]),
        "stage_se3": lambda: (ctx.se3_exp(np.arange(6) * 0.01), ctx.se3_mul(gt, TW.ROLL), ctx.se3_matrix(gt), ctx.se3_handoff(gt, 1),
                              ctx.solve_delta(A + np.eye(6, dtype=np.float32), J[0])),
        "stage_warp": lambda: ctx.warp(1, table, gt),
        "stage_jacobian": lambda: jacobian_case(ctx, gt),
        "stage_ls": lambda: (ctx.ls_accumulate(J, r, wt), ctx.ls_accumulate_sse(J, r, wt)),
        "stage_robust_weights": lambda: ctx.robust_weights(np.linspace(-60, 60, 1000).astype(np.float32)),
        "stage_trajectory": lambda: (ctx.accumulate_trajectory(poses, t_scale=40.0), ctx.accumulate_trajectory(poses, scan=True)),
        "stage_gn_update": lambda: gn_update_case(ctx),
        "stage_gradient_and_candidates": lambda: (ctx.gradient_magnitude(2, 1), ctx.obtain_candidate_points(2, 1, 5.0),
                                                  ctx.obtain_candidate_points_batch(0, 3, 0, 5.0)),
        "stage_patches": lambda: (ctx.obtain_patch_points(0, kps[2]), ctx.obtain_patch_points_batch([0, 2, 3], kps),
                                  ctx.add_patch_points(1, table[:40] / 2)),
        "stage_pose_points": lambda: ctx.estimate_pose_points(0, 1, {l: ctx.obtain_candidate_points(0, l, 5.0)[0] for l in (0, 1, 2)}),
    }


def device_match_outputs(capi, ctx, pairs):
    torch = importlib.import_module("torch")
    norm, dim, cap, q, nq, t, nt = ctx._descriptor_block(pairs, None, 130)
    to = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    dq, dt, dnq, dnt = to(q), to(t), to(nq), to(nt)
    dm = torch.zeros((len(pairs), cap, 3), dtype=torch.int32, device="cuda")
    dc = torch.zeros((len(pairs),), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_descriptors_device_async(len(pairs), dim, cap, dq.data_ptr(), dnq.data_ptr(), dt.data_ptr(), dnt.data_ptr(), dm.data_ptr(),
                                       dc.data_ptr(), norm=norm)
    ctx.sync()
    return dm.cpu().numpy(), dc.cpu().numpy()


SCRATCH_CASES = ["candidates_batch", "candidates_batch_huber_bilinear", "features_batch_weights", "dense_batch", "knn_l2", "match_host_l2",
                 "match_host_hamming", "match_device_l2", "ransac", "surf", "surf_describe", "surf_stages", "orb", "orb_stages",
                 "tracking_surf", "tracking_orb", "warp_explicit", "warp_batch", "warp_batch_level_2", "warp_mosaic", "cloud_batch",
                 "cloud_batch_cut", "cloud_batch_async", "cloud_points", "stage_resize", "stage_scharr", "stage_se3", "stage_warp", "stage_jacobian", "stage_ls",
                 "stage_robust_weights", "stage_trajectory", "stage_gn_update", "stage_gradient_and_candidates", "stage_patches", "stage_pose_points"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCRATCH_CASES)
def test_gpu_scratch_guards(capi, synth, case):
    ctx, gt = tracker_ctx(capi, synth, 165, 99)
    cases = scratch_cases(capi, synth, ctx, gt)
    assert sorted(cases) == sorted(SCRATCH_CASES)
    same_with_guards(ctx, cases[case])
    ctx.close()


@pytest.mark.gpu
def test_gpu_scratch_guards_across_a_growth(capi, synth):
    """guards on, a small call and then a larger one of the same stage: the block is made again with its gaps, both calls leave every gap
    intact and give the bytes of the same calls without guards; then a smaller one again, in the block the larger one left"""
    ctx, gt = tracker_ctx(capi, synth, 165, 99)
    small = [synth.descriptor_pair(900, 40, 37, 64, "l2")[:2]]
    large = [synth.descriptor_pair(901 + i, 300, 281, 64, "l2")[:2] for i in range(3)]
    ransac_small = [ransac_cases.scene(60, 12, 0.0, 0.3)[:3]]
    ransac_large = [ransac_cases.scene(61 + i, 300 + i, 0.3, 0.3)[:3] for i in range(3)]
    steps = [lambda: ctx.match_descriptors_batch(small), lambda: ctx.match_descriptors_batch(large, cap=301),
             lambda: ctx.match_descriptors_batch(small), lambda: ctx.ransac_inliers_batch(ransac_small),
             lambda: ctx.ransac_inliers_batch(ransac_large), lambda: ctx.warp_image_batch(REF[:1], TGT[:1], gt[None], lvl=2),
             lambda: ctx.warp_image_batch(REF, TGT, np.stack([gt, TW.ROLL, TW.CONTRACT]), lvl=0)]
    want = [frozen(s()) for s in steps]
    ctx.debug_guards(GUARD)
    for i, s in enumerate(steps):
        assert frozen(s()) == want[i], i
        assert ctx.debug_check_guards() == (0, ""), i
    ctx.debug_guards(0)
    assert [frozen(s()) for s in steps] == want
    ctx.close()


@pytest.mark.gpu
def test_gpu_scratch_guards_carved_then_plain_use_of_one_block(capi, synth):
    """The shared scratch serves a carved call (uwt_scharr3: two arrays, the block ends with the carve's last gap) and then plain ones
    (uwt_robust_weights: 8 n + 64 bytes, one array with a tail gap) that fit the block it left: n walks the plain size up to the carved
    block's size and past it (165 x 99: 83 712 bytes with gaps of 256; n = 10 456 fills it), so the tail gap moves through the block's
    end.  Every gap of every use is intact, and so are the results."""
    ctx, _ = tracker_ctx(capi, synth, 165, 99)
    frames, _, _ = TW.scene(synth, 165, 99, True)
    sizes = list(range(10380, 10480, 4))
    r = np.linspace(-60, 60, 10480).astype(np.float32)
    want_g = frozen(ctx.scharr3(frames[1]))
    want = [frozen(ctx.robust_weights(r[:n])) for n in sizes]
    ctx.debug_guards(GUARD)
    assert frozen(ctx.scharr3(frames[1])) == want_g and ctx.debug_check_guards() == (0, "")
    for n, w in zip(sizes, want):
        assert frozen(ctx.robust_weights(r[:n])) == w, n
        assert ctx.debug_check_guards() == (0, ""), n
    assert frozen(ctx.scharr3(frames[1])) == want_g and ctx.debug_check_guards() == (0, "")   # and a carved use of the block a plain one grew
    ctx.debug_guards(0)
    ctx.close()


@pytest.mark.gpu
def test_gpu_debug_guards_refuses_a_size_out_of_range(capi, synth):
    ctx, _ = tracker_ctx(capi, synth, 165, 99)
    for bad in (-1, (1 << 24) + 1):
        with pytest.raises(capi.UwtError) as e:
            ctx.debug_guards(bad)
        assert e.value.status == 1
    assert ctx.estimate_pose_batch(REF, TGT)[1][0]["status"] == OK
    ctx.close()
