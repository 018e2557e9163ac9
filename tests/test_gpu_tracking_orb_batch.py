"""System::Tracking under RobustMatcher(1) for a batch of pairs in one device-resident call (uwt_tracking_orb_batch*): every output of
every pair compared AS INTEGERS / BYTES — no tolerance anywhere — with (a) the staged sequence of the existing entry points on the same
context (ORB -> Hamming matcher -> RANSAC -> getGoodKeypoints -> the live call), (b) the CPU restatement of the front end
(tests/tracking_orb_ref.py) and (c) the mirrors' Tracking loop with RobustMatcher(detector=1).  The counts asserted here are those
tests/test_tracking_orb_ref_cpu.py shows without a device.  Every call names its cap: 2048 unless the case is about another one."""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

import orb_cases
import surf_cases
import tracking_orb_ref as TO
from test_gpu_tracking_batch import (IDENTITY, device_set, differs, fetch, front_of, info_tuple, io_of, make_ctx, pair, result_of, seq, xy)

ARITH_INDEPENDENT = True   # the chain adds no arithmetic of its own: one arithmetic set shows everything
OK, INVALID_ARG, NO_VALID_POINTS, CAPACITY, PAIR_FAILED = 0, 1, 2, 5, 6   # uwt_status_code (include/uwt.h)
W, H = 256, 240
CAP = 2048


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def staged(ctx, capi, a, b, prev=None, tp=None, cap=CAP):
    """the staged sequence of the existing entry points for one pair, on the same context (and under its pattern in force)"""
    tp = tp or capi.default_tracking_orb_params()
    n_prev = 0 if prev is None else len(prev)
    use = n_prev >= 1 and n_prev >= tp.min_matches
    if use:
        kq, dq = ctx.orb_describe_batch([a], [prev], params=tp.orb, cap=cap)[0]
    else:
        kq, dq = ctx.orb_detect_describe_batch([a], params=tp.orb, cap=cap)[0]
    kt, dt = ctx.orb_detect_describe_batch([b], params=tp.orb, cap=cap)[0]
    sym = ctx.match_descriptors_batch([(dq, dt)], ratio=tp.ratio, cap=cap)[0]
    _, good, ri = ctx.ransac_inliers_batch([(sym, xy(kq), xy(kt))], params=tp.ransac, cap=cap, kp_cap=cap)[0]
    kept_prev, kept_cur = kq[good["query_idx"]], kt[good["train_idx"]]
    poses, stats = ctx.estimate_pose_features_batch([a], [b], [xy(kept_prev)[:200]])
    st = np.zeros(1, capi.STATS)
    for k in ("status", "iterations", "n_valid", "error"):
        st[k] = stats[0][k]
    info = (0, int(use), len(kq), len(kt), len(sym), len(good), int(ri["best_hypothesis"]), int(ri["hypotheses_run"]))
    return dict(info=info, good=good.tobytes(), kept_prev=kept_prev.tobytes(), kept_cur=kept_cur.tobytes(),
                pose=poses[0].view(np.uint32).tobytes(), stats=st[0].tobytes())


def same(got, want):
    d = differs(got, want)
    assert d is None, d


def ransac_over(distance):
    return dict(ransac=dict(distance=distance)) if distance else {}


# ---- 1. one pair, every stage -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance,counts", [(None, (471, 464, 270, 269)), (0.05, (471, 464, 270, 237))])
def test_gpu_one_pair_every_stage(capi, synth, distance, counts):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    tp = capi.default_tracking_orb_params(**ransac_over(distance))
    r = ctx.tracking_orb_batch([0], [1], params=tp, cap=CAP)
    got = result_of(r, 0)
    print("distance", distance, "info", got["info"], "stats", r["stats"][0])
    assert r["status"] == OK and got["info"][:2] == (OK, 0) and got["info"][2:6] == counts
    assert int(r["info"]["n_matches"][0]) == len(r["good"][0]) == len(r["kept_prev"][0]) == len(r["kept_cur"][0])
    assert np.count_nonzero(np.bincount(r["kept_prev"][0]["octave"], minlength=8)) == 8   # kept key points on every layer
    same(got, staged(ctx, capi, 0, 1, tp=tp))
    same(got, front_of(TO.front_end(ref, tgt, **ransac_over(distance))))
    ctx.close()


# ---- 2. hand-over without a wait ----------------------------------------------------------------------------------------------------
def chained_sequence(ctx, capi, torch, n_frames, tp, cap):
    """pair k = (slot k, slot k + 1) as successive one-pair asynchronous calls, kept_cur -> prev_kp on the device, ONE sync"""
    sets = [device_set(torch, 1, cap) for _ in range(n_frames - 1)]
    for k in range(n_frames - 1):
        ctx.tracking_orb_batch_async([k], [k + 1], io_of(sets[k], sets[k - 1] if k else None), params=tp, cap=cap)
    ctx.sync()
    return [result_of(fetch(capi, s), 0) for s in sets]


@pytest.mark.gpu
def test_gpu_handover_equals_the_tracking_loop(capi, synth, torch):
    T = importlib.import_module("uw-slam_amd.tracker")
    frames = seq(synth, 3)
    intr = TO.INTR[(W, H)]
    tracker = T.Tracker(False, max_frames=6)
    tracker.InitializePyramid(W, H, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    rm = T.RobustMatcher(tracker, detector=1)
    fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
    loop = []
    for k in range(4):
        st = T.Tracking(tracker, rm, fr[k], fr[k + 1])
        loop.append(dict(n=fr[k].n_matches_, kept_prev=fr[k].orb_keypoints_.tobytes(), kept_cur=fr[k + 1].orb_keypoints_.tobytes(),
                         xy_prev=fr[k].keypoints_.tobytes(), pose=np.asarray(fr[k].rigid_transformation_, np.float32).view(np.uint32).tobytes(),
                         stats=(st["status"], st["iterations"], st["n_valid"], np.float32(st["error"]).tobytes())))
    ctx = tracker._ctx   # the same context, the frames resident where the loop bound them
    assert [f._slot for f in fr] == [0, 1, 2, 3, 4]
    got = chained_sequence(ctx, capi, torch, 5, None, CAP)
    ref = TO.sequence(frames, min_matches=110)
    print("used_provided", [g["info"][1] for g in got], "n_matches", [g["info"][5] for g in got])
    assert [g["info"][1] for g in got] == [0, 1, 1, 0]            # both paths in one walk
    assert [g["info"][5] for g in got] == [262, 163, 108, 379]
    for k in range(4):
        assert differs(got[k], front_of(ref[k])) is None, (k, differs(got[k], front_of(ref[k])))
        st = np.frombuffer(got[k]["stats"], capi.STATS)[0]
        assert got[k]["info"][5] == loop[k]["n"]
        assert got[k]["kept_prev"] == loop[k]["kept_prev"] and got[k]["kept_cur"] == loop[k]["kept_cur"], k
        assert xy(np.frombuffer(got[k]["kept_prev"], capi.KEYPOINT)).tobytes() == loop[k]["xy_prev"]
        assert got[k]["pose"] == loop[k]["pose"], k
        assert (int(st["status"]), int(st["iterations"]), int(st["n_valid"]), st["error"].tobytes()) == loop[k]["stats"], k
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,min_matches,n_matches,used", [(3, 60, [262, 163, 108, 95], [0, 1, 1, 1]), (17, 110, [235, 168, 136, 96], [0, 1, 1, 1])])
def test_gpu_handover_equals_staged_and_restatement(capi, synth, torch, seed, min_matches, n_matches, used):
    frames = seq(synth, seed)
    ctx = make_ctx(capi, W, H, list(frames))
    tp = capi.default_tracking_orb_params(min_matches=min_matches)
    got = chained_sequence(ctx, capi, torch, 5, tp, CAP)
    ref = TO.sequence(frames, min_matches=min_matches)
    print("seed", seed, "min_matches", min_matches, "used_provided", [g["info"][1] for g in got], "n_matches", [g["info"][5] for g in got])
    assert [g["info"][1] for g in got] == used and [g["info"][5] for g in got] == n_matches
    prev = None
    for k in range(4):
        assert differs(got[k], front_of(ref[k])) is None, (k, differs(got[k], front_of(ref[k])))
        want = staged(ctx, capi, k, k + 1, prev=prev, tp=tp)
        assert differs(got[k], want) is None, (k, differs(got[k], want))
        prev = np.frombuffer(got[k]["kept_cur"], capi.KEYPOINT)
    ctx.close()


# ---- 3. batch independence --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_batch_independence(capi, synth):
    ref, tgt, _ = pair(synth, W, H, 31)
    s3 = seq(synth, 3)
    ctx = make_ctx(capi, W, H, [ref, tgt, surf_cases.flat(W, H), s3[0], s3[1], s3[2]], max_pairs=6)
    kept = ctx.tracking_orb_batch([3], [4], cap=CAP)["kept_cur"][0]   # what frame s3[1] kept as the current frame of pair (s3[0], s3[1])
    assert len(kept) == 262
    none = np.zeros(0, capi.KEYPOINT)
    pairs = [(0, 1, none), (0, 1, none), (0, 2, none), (2, 1, none), (4, 5, kept), (4, 5, kept[:40])]
    alone = [result_of(ctx.tracking_orb_batch([a], [b], prev=[p], cap=CAP), 0) for a, b, p in pairs]
    for order in (list(range(6)), list(range(5, -1, -1))):
        r = ctx.tracking_orb_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], prev=[pairs[i][2] for i in order], cap=CAP)
        assert r["status"] == PAIR_FAILED
        for place, i in enumerate(order):
            assert differs(result_of(r, place), alone[i]) is None, (order, i, differs(result_of(r, place), alone[i]))
    stats = [np.frombuffer(a["stats"], capi.STATS)[0] for a in alone]
    print("info", [a["info"] for a in alone])
    assert [int(s["status"]) for s in stats] == [OK, OK, NO_VALID_POINTS, NO_VALID_POINTS, OK, OK]
    assert [a["info"][0] for a in alone] == [OK] * 6                      # the front end of a flat pair is no error
    assert [a["info"][1] for a in alone] == [0, 0, 0, 0, 1, 0]            # 262 records are used, 40 are ignored
    assert alone[0] == alone[1] and alone[0]["info"][5] == 269
    assert alone[2]["info"][3] == 0 and alone[3]["info"][2] == 0 and alone[2]["info"][5] == alone[3]["info"][5] == 0
    assert alone[4]["info"][2] == 262 and alone[4]["info"][5] == 163
    same(alone[4], staged(ctx, capi, 4, 5, prev=kept))
    same(alone[5], staged(ctx, capi, 4, 5, prev=kept[:40]))
    assert alone[5]["info"][2] > 40                                       # the detection of s3[1]
    ctx.close()


# ---- 4. sizes, depth, capacity ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_small_frame_with_and_without_depth(capi, synth, depth):
    ref, tgt, dep = pair(synth, 160, 96, 5, depth)
    ctx = make_ctx(capi, 160, 96, [ref, tgt], [dep, dep] if depth else None)
    r = ctx.tracking_orb_batch([0], [1], cap=CAP)
    got = result_of(r, 0)
    print("depth", depth, "info", got["info"], "stats", r["stats"][0])
    assert got["info"][2:6] == (72, 69, 43, 43) and int(r["stats"]["status"][0]) == OK
    layers = np.bincount(np.concatenate([r["kept_prev"][0]["octave"], r["kept_cur"][0]["octave"]]), minlength=8)
    assert not layers[3:].any()                                           # the fourth layer is below the band
    same(got, staged(ctx, capi, 0, 1))
    same(got, front_of(TO.front_end(ref, tgt)))
    tp = capi.default_tracking_orb_params(ransac=dict(distance=0.05))
    got = result_of(ctx.tracking_orb_batch([0], [1], params=tp, cap=CAP), 0)
    assert got["info"][2:6] == (72, 69, 43, 36)
    same(got, staged(ctx, capi, 0, 1, tp=tp))
    ctx.close()


@pytest.mark.gpu
def test_gpu_capacity_cuts_both_sets(capi, synth):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    r = ctx.tracking_orb_batch([0], [1], cap=32)
    got = result_of(r, 0)
    print("cap 32 info", got["info"])
    assert got["info"][2:4] == (32, 32)
    same(got, staged(ctx, capi, 0, 1, cap=32))
    same(got, front_of(TO.front_end(ref, tgt, cap=32)))
    ctx.close()


@pytest.mark.gpu
def test_gpu_a_frame_without_a_band(capi, synth):
    ref, tgt, _ = pair(synth, 97, 61, 11)
    ctx = make_ctx(capi, 97, 61, [ref, tgt])
    r = ctx.tracking_orb_batch([0], [1], cap=CAP)
    got = result_of(r, 0)
    print("97 x 61 info", got["info"], "stats", r["stats"][0])
    assert r["status"] == PAIR_FAILED
    assert got["info"] == (OK, 0, 0, 0, 0, 0) + got["info"][6:] and int(r["stats"]["status"][0]) == NO_VALID_POINTS
    same(got, staged(ctx, capi, 0, 1))
    same(got, front_of(TO.front_end(ref, tgt)))
    ctx.close()


@pytest.mark.gpu
def test_gpu_more_than_200_kept(capi, synth):
    ref, tgt, _ = pair(synth, 640, 480, 31)
    ctx = make_ctx(capi, 640, 480, [ref, tgt])
    r = ctx.tracking_orb_batch([0], [1], cap=CAP)
    got = result_of(r, 0)
    print("640 x 480 info", got["info"], "stats", r["stats"][0])
    assert got["info"][5] > 200 and int(r["stats"]["status"][0]) == OK    # the live call takes the first 200
    same(got, staged(ctx, capi, 0, 1))
    ctx.close()


# ---- 5. what only the device can see ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("octave", [8, -1])
def test_gpu_device_side_errors(capi, synth, octave):
    s3 = seq(synth, 3)
    ctx = make_ctx(capi, W, H, [s3[0], s3[1], s3[2]], max_pairs=4)
    kept = ctx.tracking_orb_batch([0], [1], cap=CAP)["kept_cur"][0]
    assert len(kept) == 262
    good = result_of(ctx.tracking_orb_batch([1], [2], prev=[kept], cap=CAP), 0)
    assert good["info"][:2] == (OK, 1) and good["info"][5] == 163
    kp, n = np.zeros((4, CAP), capi.KEYPOINT), np.full(4, 262, np.int32)
    kp[:, :262] = kept
    kp["x"][0, 5] = np.nan
    kp["octave"][1, 7] = octave
    kp["octave"][2, 9], kp["x"][2, 9], kp["y"][2, 9] = 0, 5.0, 120.0      # inside the frame, outside layer 0's band
    r = ctx.tracking_orb_batch([1] * 4, [2] * 4, prev=(kp, n), cap=CAP)
    print("info", [info_tuple(r["info"][i]) for i in range(4)], "stats", r["stats"])
    assert r["status"] == PAIR_FAILED

    def refused(r, i):
        assert int(r["info"]["status"][i]) == INVALID_ARG and int(r["stats"]["status"][i]) == INVALID_ARG, i
        assert int(r["info"]["n_matches"][i]) == 0 and len(r["good"][i]) == 0, i
        assert info_tuple(r["info"][i])[1:3] == (0, 0) and info_tuple(r["info"][i])[4] == 0 and info_tuple(r["info"][i])[6] == -1, i
        assert r["poses"][i].tobytes() == IDENTITY.tobytes(), i

    for i in range(3):
        refused(r, i)
    same(result_of(r, 3), good)
    # a count outside 0..cap
    kp[:, :262] = kept
    n[2] = CAP + 1
    r = ctx.tracking_orb_batch([1] * 4, [2] * 4, prev=(kp, n), cap=CAP)
    assert r["status"] == PAIR_FAILED
    refused(r, 2)
    for i in (0, 1, 3):
        same(result_of(r, i), good)
    # the context still works
    same(result_of(ctx.tracking_orb_batch([1], [2], prev=[kept], cap=CAP), 0), good)
    ctx.close()


# ---- 6. what the host refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_host_side_errors_leave_outputs_untouched(capi, synth, torch):
    ref, tgt, _ = pair(synth, 160, 96, 5)
    ctx = make_ctx(capi, 160, 96, [ref, tgt])
    cap = 64   # (of the output arrays the refusals must leave alone; no refused call depends on it)
    L = capi.lib()

    def fresh():
        out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, cap), capi.MATCH),
               np.zeros((1, cap), capi.KEYPOINT), np.zeros((1, cap), capi.KEYPOINT))
        for a in out:
            a.view(np.uint8)[...] = 0x5A
        return out

    def untouched(out):
        return all((a.view(np.uint8) == 0x5A).all() for a in out)

    P = capi.default_tracking_orb_params
    bad = [(dict(ref=[2]), INVALID_ARG), (dict(tgt=[-1]), INVALID_ARG), (dict(ref=[], tgt=[]), INVALID_ARG),
           (dict(ref=[0, 0], tgt=[1, 1]), INVALID_ARG),                                    # n_pairs above max_pairs
           (dict(cap=0), INVALID_ARG), (dict(cap=capi.UWT_MATCH_MAX_ROWS + 1), CAPACITY),
           (dict(params=P(orb=dict(n_features=0))), INVALID_ARG), (dict(params=P(orb=dict(n_features=65537))), INVALID_ARG),
           (dict(params=P(orb=dict(n_levels=0))), INVALID_ARG), (dict(params=P(orb=dict(n_levels=9))), INVALID_ARG),
           (dict(params=P(orb=dict(edge_threshold=15))), INVALID_ARG), (dict(params=P(orb=dict(edge_threshold=1025))), INVALID_ARG),
           (dict(params=P(orb=dict(fast_threshold=-1))), INVALID_ARG), (dict(params=P(orb=dict(fast_threshold=256))), INVALID_ARG),
           (dict(params=P(ransac=dict(distance=-1.0))), INVALID_ARG), (dict(params=P(ransac=dict(confidence=0.0))), INVALID_ARG),
           (dict(params=P(ransac=dict(max_hypotheses=0))), INVALID_ARG),
           (dict(params=P(ratio=float("nan"))), INVALID_ARG), (dict(params=P(ratio=float("inf"))), INVALID_ARG),
           (dict(params=P(min_matches=-1)), INVALID_ARG)]
    for kw, status in bad:
        out = fresh()
        with pytest.raises(capi.UwtError) as e:
            ctx.tracking_orb_batch(kw.get("ref", [0]), kw.get("tgt", [1]), params=kw.get("params"), cap=kw.get("cap", cap), out=out)
        assert e.value.status == status, (kw, e.value.status)
        assert untouched(out) and L.uwt_last_error(ctx._h), kw

    # null lists, null required outputs, and exactly one of the provided list and its counts: the raw entry point
    one = np.array([0], np.int32)
    two = np.array([1], np.int32)
    kp, n = np.zeros((1, cap), capi.KEYPOINT), np.zeros(1, np.int32)
    for hole in ("ref", "tgt", "poses", "info", "good", "kept_prev", "kept_cur", "only_kp", "only_n"):
        out = fresh()
        a = dict(ref=one.ctypes.data, tgt=two.ctypes.data, kp=None, n=None, poses=out[0].ctypes.data, stats=out[1].ctypes.data,
                 info=out[2].ctypes.data, good=out[3].ctypes.data, kept_prev=out[4].ctypes.data, kept_cur=out[5].ctypes.data)
        if hole == "only_kp":
            a["kp"] = kp.ctypes.data
        elif hole == "only_n":
            a["n"] = n.ctypes.data
        else:
            a[hole] = None
        st = L.uwt_tracking_orb_batch(ctx._h, 1, *[C.c_void_p(a[k]) for k in ("ref", "tgt")], None, cap,
                                      *[C.c_void_p(a[k]) for k in ("kp", "n", "poses", "stats", "info", "good", "kept_prev", "kept_cur")])
        assert st == INVALID_ARG and untouched(out) and L.uwt_last_error(ctx._h), hole

    # the asynchronous form: an input that is also an output of the same call
    s = device_set(torch, 1, cap, fill=0x5A5A5A5A)
    for alias in ("kept_prev", "kept_cur", "n_matches"):
        io = io_of(s)
        io["prev_kp"], io["n_prev"] = s["good"].data_ptr(), s["poses"].data_ptr()   # (never read: the call is refused)
        io["prev_kp" if alias != "n_matches" else "n_prev"] = s[alias].data_ptr()
        with pytest.raises(capi.UwtError) as e:
            ctx.tracking_orb_batch_async([0], [1], io, cap=cap)
        assert e.value.status == INVALID_ARG, alias
    for hole in ("poses", "info", "good", "kept_prev", "kept_cur", "n_matches"):
        io = io_of(s)
        io[hole] = None
        with pytest.raises(capi.UwtError) as e:
            ctx.tracking_orb_batch_async([0], [1], io, cap=cap)
        assert e.value.status == INVALID_ARG, hole
    ctx.sync()
    assert all(bool((v == 0x5A5A5A5A).all()) for v in s.values())
    assert ctx.tracking_orb_batch([0], [1], cap=CAP)["status"] == OK   # the context still works
    ctx.close()


@pytest.mark.gpu
def test_gpu_a_frame_higher_than_the_pyramid_allows_is_refused(capi):
    # (16385 rows of 16 pixels: a context that wide cannot be created, the tracker's own index arithmetic refuses it)
    ctx = capi.Context(capi.default_params(16, 16385, 525.0, 525.0, 7.5, 8192.0, n_levels=1, first_level=0, last_level=0, max_frames=2, max_pairs=1))
    out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, 8), capi.MATCH),
           np.zeros((1, 8), capi.KEYPOINT), np.zeros((1, 8), capi.KEYPOINT))
    for a in out:
        a.view(np.uint8)[...] = 0x5A
    with pytest.raises(capi.UwtError) as e:
        ctx.tracking_orb_batch([0], [1], cap=8, out=out)   # nothing is enqueued: the slots need not hold frames
    assert e.value.status == CAPACITY and capi.lib().uwt_last_error(ctx._h)
    assert all((a.view(np.uint8) == 0x5A).all() for a in out)
    ctx.close()


# ---- 7. forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_async_equals_sync_and_rows_past_a_count_stay(capi, synth, torch):
    ref, tgt, _ = pair(synth, 160, 96, 5)
    ctx = make_ctx(capi, 160, 96, [ref, tgt])
    out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, CAP), capi.MATCH),
           np.zeros((1, CAP), capi.KEYPOINT), np.zeros((1, CAP), capi.KEYPOINT))
    for a in out[3:]:
        a.view(np.uint8)[...] = 0x5A
    sync = ctx.tracking_orb_batch([0], [1], cap=CAP, out=out)
    n = int(sync["info"]["n_matches"][0])
    assert n == 43
    for a in out[3:]:
        assert (a[0, n:].view(np.uint8) == 0x5A).all() and not (a[0, :n].view(np.uint8) == 0x5A).all()
    s = device_set(torch, 1, CAP, fill=0x5A5A5A5A)
    ctx.tracking_orb_batch_async([0], [1], io_of(s), cap=CAP)
    ctx.sync()
    got = fetch(capi, s)
    same(result_of(got, 0), result_of(sync, 0))
    for k in ("good", "kept_prev", "kept_cur"):
        assert (got["raw"][k][0, n:] == 0x5A5A5A5A).all(), k
    # stats may be left out
    s2 = device_set(torch, 1, CAP)
    io = io_of(s2)
    io["stats"] = None
    ctx.tracking_orb_batch_async([0], [1], io, cap=CAP)
    ctx.sync()
    got2 = result_of(fetch(capi, s2), 0)
    assert got2["pose"] == result_of(sync, 0)["pose"] and got2["info"] == result_of(sync, 0)["info"]
    assert not s2["stats"].cpu().numpy().any()
    ctx.close()


@pytest.mark.gpu
def test_gpu_growth_under_a_queued_async_call(capi, synth, torch):
    """a one-pair asynchronous call is still queued when a call of the same context needs the scratch larger (two pairs): both give,
    as bytes, what the same two calls give on fresh contexts"""
    ref, tgt, _ = pair(synth, 160, 96, 5)

    def run(ctx_small, ctx_large):
        s = device_set(torch, 1, CAP)
        ctx_small.tracking_orb_batch_async([0], [1], io_of(s), cap=CAP)
        r = ctx_large.tracking_orb_batch([0, 0], [1, 1], cap=CAP)                 # no sync in between
        ctx_small.sync()
        return result_of(fetch(capi, s), 0), result_of(r, 0), result_of(r, 1)

    ctxs = [make_ctx(capi, 160, 96, [ref, tgt], max_pairs=2) for _ in range(3)]
    got = run(ctxs[0], ctxs[0])
    want = run(ctxs[1], ctxs[2])
    for c in ctxs:
        c.close()
    assert got[0]["info"][5] == got[1]["info"][5] == 43 and got[0] == got[1] == got[2]
    assert got == want


@pytest.mark.gpu
def test_gpu_tuning_does_not_show(capi, synth):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    first = result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0)
    ctx.set_tuning(split=2, tail_update=2, first_poll=1, typed_loads=0, target_blocks=256)
    second = result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0)
    ctx.close()
    assert first["info"][5] == 269 and first == second


# ---- 8. a pattern of the caller's -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_pattern_of_the_callers(capi, synth):
    ref, tgt, _ = pair(synth, 160, 96, 5)
    ctx = make_ctx(capi, 160, 96, [ref, tgt])
    default = result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0)
    p = orb_cases.second_pattern()
    ctx.orb_set_pattern(p)
    got = result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0)
    same(got, staged(ctx, capi, 0, 1))
    same(got, front_of(TO.front_end(ref, tgt, pattern=p)))
    assert got["info"][2:4] == default["info"][2:4] == (72, 69)           # the same key points,
    assert got["info"][4] >= 8 and got["good"] != default["good"]         # other descriptors: other matches
    ctx.orb_set_pattern(None)
    same(result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0), default)
    ctx.close()


# ---- 9. mirrors and tool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_tracking_batch_mirror_equals_the_tracking_loop(capi, synth):
    T = importlib.import_module("uw-slam_amd.tracker")
    frames = seq(synth, 3)
    intr = TO.INTR[(W, H)]
    Kmat = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32)

    def fields(run):
        tracker = T.Tracker(False, max_frames=6)
        tracker.InitializePyramid(W, H, Kmat)
        rm = T.RobustMatcher(tracker, detector=1)
        fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
        stats = run(tracker, rm, fr)
        tracker._ctx.close()
        assert all(len(f.surf_keypoints_) == 0 for f in fr)
        return ([(f.n_matches_, np.asarray(f.keypoints_, np.float32).tobytes(), np.asarray(f.orb_keypoints_, capi.KEYPOINT).tobytes(),
                  np.asarray(f.rigid_transformation_, np.float32).view(np.uint32).tobytes()) for f in fr],
                [(s["status"], s["iterations"], s["n_valid"], np.float32(s["error"]).tobytes()) for s in stats])

    loop = fields(lambda tr, rm, fr: [T.Tracking(tr, rm, fr[k], fr[k + 1]) for k in range(4)])
    batch = fields(lambda tr, rm, fr: T.TrackingBatch(tr, rm, [(fr[k], fr[k + 1]) for k in range(4)], cap=CAP))
    assert [f[0] for f in loop[0]] == [262, 163, 108, 379, 379]
    assert batch == loop


@pytest.mark.gpu
def test_gpu_track_sequence_chained_equals_live(capi, synth, torch):
    """tools/track_sequence.py --live --chained --detector orb walks the sequence without a wait and gives the trajectory of --live"""
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "track_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    frames = list(seq(synth, 3))
    live = tool.track_live(W, H, TO.INTR[(W, H)], frames, None, detector=1)
    chained = tool.track_live_chained(W, H, TO.INTR[(W, H)], frames, None, cap=CAP, detector=1)
    assert live[2] == chained[2] == [262, 163, 108, 379]
    assert live[0].view(np.uint32).tobytes() == chained[0].view(np.uint32).tobytes()
    assert [(s["status"], s["iterations"], s["n_valid"]) for s in live[1]] == [(s["status"], s["iterations"], s["n_valid"]) for s in chained[1]]


# ---- 10. SURF unchanged ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_surf_chain_unchanged_beside_the_orb_chain(capi, synth):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    first = result_of(ctx.tracking_batch([0], [1], cap=CAP), 0)
    assert first["info"][5] == 174
    orb = result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0)   # the scratch is shared
    assert orb["info"][5] == 269
    assert result_of(ctx.tracking_batch([0], [1], cap=CAP), 0) == first
    assert result_of(ctx.tracking_orb_batch([0], [1], cap=CAP), 0) == orb
    ctx.close()
