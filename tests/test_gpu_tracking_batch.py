"""System::Tracking for a batch of pairs in one device-resident call (uwt_tracking_batch*, uwt_match_descriptors_device_async): every
output of every pair compared AS INTEGERS / BYTES — no tolerance anywhere — with the staged sequence of the existing entry points on
the same context (SURF -> matcher -> RANSAC -> getGoodKeypoints -> the live call), and the front end with its CPU restatement
(tests/tracking_ref.py)."""
import ctypes as C
import importlib
import importlib.util

import numpy as np
import pytest

import match_cases
import surf_cases as K
import tracking_ref as TR

ARITH_INDEPENDENT = True   # the chain adds no arithmetic of its own: one arithmetic set shows everything
OK, INVALID_ARG, NO_VALID_POINTS, CAPACITY, PAIR_FAILED = 0, 1, 2, 5, 6   # uwt_status_code (include/uwt.h)
W, H = 256, 240
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)   # qx qy qz qw tx ty tz
INFO_FIELDS = ("status", "used_provided", "n_kp_prev", "n_kp_cur", "n_symmetric", "n_matches", "best_hypothesis", "hypotheses_run")


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def make_ctx(capi, w, h, frames, depths=None, max_pairs=1, **over):
    """a context with `frames` resident from slot 0 on, in the state the live call expects"""
    if w < 200:   # a small frame has fewer levels than the default schedule names (the live call runs on level 0 alone)
        over.setdefault("n_levels", 3)
        over.setdefault("first_level", 2)
        over.setdefault("last_level", 1)
    if depths is not None:
        over["has_depth"] = 1
    ctx = capi.Context(capi.default_params(w, h, *TR.INTR[(w, h)], max_frames=max(2, len(frames)), max_pairs=max_pairs, **over))
    ctx.upload_frames(0, np.stack(frames), np.stack(depths) if depths is not None else None)
    ctx.build_pyramids(0, len(frames))
    ctx.apply_gradient(0, len(frames))
    return ctx


_rendered = {}


def pair(synth, w, h, seed, depth=False):
    key = ("pair", w, h, seed, depth)
    if key not in _rendered:
        _rendered[key] = synth.render_pair(w, h, *TR.INTR[(w, h)], seed=seed, with_depth=depth)[:3]
    return _rendered[key]


def seq(synth, seed):
    key = ("seq", seed)
    if key not in _rendered:
        _rendered[key] = synth.render_sequence(W, H, *TR.INTR[(W, H)], 5, seed=seed)[0]
    return _rendered[key]


def xy(kp):
    return np.stack([kp["x"], kp["y"]], 1).astype(np.float32).reshape(-1, 2)


def info_tuple(rec):
    return tuple(int(rec[k]) for k in INFO_FIELDS)


def result_of(r, i):
    """pair i of a tracking_batch result in the form every comparison uses"""
    return dict(info=info_tuple(r["info"][i]), good=r["good"][i].tobytes(), kept_prev=r["kept_prev"][i].tobytes(),
                kept_cur=r["kept_cur"][i].tobytes(), pose=r["poses"][i].view(np.uint32).tobytes(), stats=r["stats"][i].tobytes())


def staged(ctx, capi, a, b, prev=None, tp=None, cap=2048):
    """the staged sequence of the existing entry points for one pair, on the same context"""
    tp = tp or capi.default_tracking_params()
    n_prev = 0 if prev is None else len(prev)
    use = n_prev >= 1 and n_prev >= tp.min_matches
    if use:
        kq, dq = ctx.surf_describe_batch([a], [prev], params=tp.surf, cap=cap)[0]
    else:
        kq, dq = ctx.surf_detect_describe_batch([a], params=tp.surf, cap=cap)[0]
    kt, dt = ctx.surf_detect_describe_batch([b], params=tp.surf, cap=cap)[0]
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


def front_of(ref):
    """a tracking_ref.front_end result in the same form (the front end: no pose, no stats)"""
    return dict(info=tuple(int(ref["info"][k]) for k in INFO_FIELDS), good=ref["good"].tobytes(), kept_prev=ref["kept_prev"].tobytes(),
                kept_cur=ref["kept_cur"].tobytes())


def differs(got, want):
    """the first field of `want` that `got` does not have bit for bit, or None"""
    for k, v in want.items():
        if got[k] != v:
            return "%s: %r against %r" % (k, got[k] if k == "info" else len(got[k]), v if k == "info" else len(v))
    return None


def ransac_over(distance):
    return dict(ransac=dict(distance=distance)) if distance else {}


# ---- device buffers of the asynchronous form ------------------------------------------------------------------------------------
def device_set(torch, P, cap, fill=0):
    i32 = dict(dtype=torch.int32, device="cuda")
    s = dict(poses=torch.full((P, 7), fill, **i32), stats=torch.full((P, 4), fill, **i32), info=torch.full((P, 8), fill, **i32),
             good=torch.full((P, cap, 3), fill, **i32), kept_prev=torch.full((P, cap, 8), fill, **i32),
             kept_cur=torch.full((P, cap, 8), fill, **i32), n_matches=torch.full((P,), fill, **i32))
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    return s


def io_of(s, prev=None):
    io = {k: v.data_ptr() for k, v in s.items()}
    if prev is not None:
        io["prev_kp"], io["n_prev"] = prev["kept_cur"].data_ptr(), prev["n_matches"].data_ptr()
    return io


def fetch(capi, s):
    """a device set as tracking_batch returns its results"""
    host = {k: v.cpu().numpy() for k, v in s.items()}
    info = host["info"].view(capi.TRACKING_INFO).reshape(-1)
    cnt = host["n_matches"]
    P = len(cnt)
    good = host["good"].view(capi.MATCH).reshape(P, -1)
    kp, kc = host["kept_prev"].view(capi.KEYPOINT).reshape(P, -1), host["kept_cur"].view(capi.KEYPOINT).reshape(P, -1)
    return dict(poses=host["poses"].view(np.float32), stats=host["stats"].view(capi.STATS).reshape(-1), info=info,
                good=[good[i, :cnt[i]] for i in range(P)], kept_prev=[kp[i, :cnt[i]] for i in range(P)],
                kept_cur=[kc[i, :cnt[i]] for i in range(P)], raw=host)


# ---- 1. one pair, every stage -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance,inliers", [(None, 174), (0.05, 144), (0.02, 98)])
def test_gpu_one_pair_every_stage(capi, synth, distance, inliers):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    tp = capi.default_tracking_params(**ransac_over(distance))
    r = ctx.tracking_batch([0], [1], params=tp)
    got = result_of(r, 0)
    print("distance", distance, "info", got["info"], "stats", r["stats"][0])
    assert r["status"] == OK and got["info"][5] == inliers
    assert int(r["info"]["n_matches"][0]) == len(r["good"][0]) == len(r["kept_prev"][0])
    assert differs(got, staged(ctx, capi, 0, 1, tp=tp)) is None, differs(got, staged(ctx, capi, 0, 1, tp=tp))
    want = front_of(TR.front_end(ref, tgt, **ransac_over(distance)))
    assert differs(got, want) is None, differs(got, want)
    ctx.close()


# ---- 2. hand-over without a wait ----------------------------------------------------------------------------------------------------
def chained_sequence(ctx, capi, torch, n_frames, tp, cap):
    """pair k = (slot k, slot k + 1) as successive one-pair asynchronous calls, kept_cur -> prev_kp on the device, ONE sync"""
    sets = [device_set(torch, 1, cap) for _ in range(n_frames - 1)]   # (two would do for the hand-over; one per call keeps every result)
    for k in range(n_frames - 1):
        ctx.tracking_batch_async([k], [k + 1], io_of(sets[k], sets[k - 1] if k else None), params=tp, cap=cap)
    ctx.sync()
    return [result_of(fetch(capi, s), 0) for s in sets]


@pytest.mark.gpu
def test_gpu_handover_equals_the_tracking_loop(capi, synth, torch):
    T = importlib.import_module("uw-slam_amd.tracker")
    frames = seq(synth, 3)
    intr = TR.INTR[(W, H)]
    tracker = T.Tracker(False, max_frames=6)
    tracker.InitializePyramid(W, H, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    rm = T.RobustMatcher(tracker)
    fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
    loop = []
    for k in range(4):
        st = T.Tracking(tracker, rm, fr[k], fr[k + 1])
        loop.append(dict(n=fr[k].n_matches_, kept_prev=fr[k].surf_keypoints_.tobytes(), kept_cur=fr[k + 1].surf_keypoints_.tobytes(),
                         xy_prev=fr[k].keypoints_.tobytes(), pose=np.asarray(fr[k].rigid_transformation_, np.float32).view(np.uint32).tobytes(),
                         stats=(st["status"], st["iterations"], st["n_valid"], np.float32(st["error"]).tobytes())))
    ctx = tracker._ctx   # the same context, the frames resident where the loop bound them
    assert [f._slot for f in fr] == [0, 1, 2, 3, 4]
    got = chained_sequence(ctx, capi, torch, 5, None, 2048)
    ref = TR.sequence(frames, min_matches=110)
    print("used_provided", [g["info"][1] for g in got], "n_matches", [g["info"][5] for g in got])
    assert [g["info"][1] for g in got] == [0, 1, 1, 1]
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
@pytest.mark.parametrize("min_matches,used", [(90, [0, 1, 0, 0]), (110, [0, 0, 0, 0])])
def test_gpu_handover_mixed_paths(capi, synth, torch, min_matches, used):
    frames = seq(synth, 17)
    ctx = make_ctx(capi, W, H, list(frames))
    tp = capi.default_tracking_params(min_matches=min_matches)
    got = chained_sequence(ctx, capi, torch, 5, tp, 2048)
    ref = TR.sequence(frames, min_matches=min_matches)
    print("min_matches", min_matches, "used_provided", [g["info"][1] for g in got], "n_matches", [g["info"][5] for g in got])
    assert [g["info"][1] for g in got] == used
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
    ctx = make_ctx(capi, W, H, [ref, tgt, K.flat(W, H), s3[0], s3[1], s3[2]], max_pairs=6)
    kept = ctx.tracking_batch([3], [4])["kept_cur"][0]   # what frame s3[1] kept as the current frame of pair (s3[0], s3[1])
    assert len(kept) == 149
    none = np.zeros(0, capi.KEYPOINT)
    pairs = [(0, 1, none), (0, 1, none), (0, 2, none), (2, 1, none), (4, 5, kept), (4, 5, kept[:40])]
    alone = [result_of(ctx.tracking_batch([a], [b], prev=[p]), 0) for a, b, p in pairs]
    for order in (list(range(6)), list(range(5, -1, -1))):
        r = ctx.tracking_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], prev=[pairs[i][2] for i in order])
        assert r["status"] == PAIR_FAILED
        for place, i in enumerate(order):
            assert differs(result_of(r, place), alone[i]) is None, (order, i, differs(result_of(r, place), alone[i]))
    stats = [np.frombuffer(a["stats"], capi.STATS)[0] for a in alone]
    print("info", [a["info"] for a in alone])
    assert [int(s["status"]) for s in stats] == [OK, OK, NO_VALID_POINTS, NO_VALID_POINTS, OK, OK]
    assert [a["info"][0] for a in alone] == [OK] * 6                      # the front end of a flat pair is no error
    assert [a["info"][1] for a in alone] == [0, 0, 0, 0, 1, 0]            # 149 records are used, 40 are ignored
    assert alone[0] == alone[1]
    assert alone[2]["info"][3] == 0 and alone[3]["info"][2] == 0 and alone[2]["info"][5] == alone[3]["info"][5] == 0
    assert alone[4]["info"][2] == 149 and alone[5]["info"][2] == 193      # 193: the detection of s3[1]
    want = staged(ctx, capi, 4, 5, prev=kept)
    assert differs(alone[4], want) is None, differs(alone[4], want)
    ctx.close()


# ---- 4. sizes and depth -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,depth,cap,n_matches", [(97, 61, 11, False, 2048, 14), (160, 96, 5, False, 2048, 49),
                                                         (160, 96, 5, True, 2048, 49), (640, 480, 31, False, 2048, 528),
                                                         (735, 479, 12, False, 2048, 616), (256, 240, 31, False, 32, 21)])
def test_gpu_sizes_depth_and_capacity(capi, synth, w, h, seed, depth, cap, n_matches):
    ref, tgt, dep = pair(synth, w, h, seed, depth)
    ctx = make_ctx(capi, w, h, [ref, tgt], [dep, dep] if depth else None)
    r = ctx.tracking_batch([0], [1], cap=cap)
    got = result_of(r, 0)
    print(w, h, "depth", depth, "cap", cap, "info", got["info"], "stats", r["stats"][0])
    assert got["info"][5] == n_matches          # (640 x 480 and 735 x 479: more than 200, the live call takes the first 200)
    want = staged(ctx, capi, 0, 1, cap=cap)
    assert differs(got, want) is None, differs(got, want)
    want = front_of(TR.front_end(ref, tgt, cap=cap))
    assert differs(got, want) is None, differs(got, want)
    assert int(r["stats"]["status"][0]) == OK
    ctx.close()


# ---- 5. what only the device can see ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_device_side_errors(capi, synth):
    s3 = seq(synth, 3)
    cap = 256
    ctx = make_ctx(capi, W, H, [s3[0], s3[1], s3[2]], max_pairs=4)
    kept = ctx.tracking_batch([0], [1], cap=cap)["kept_cur"][0]
    assert len(kept) == 149
    good = result_of(ctx.tracking_batch([1], [2], prev=[kept], cap=cap), 0)
    assert good["info"][:2] == (OK, 1)
    kp, n = np.zeros((4, cap), capi.KEYPOINT), np.array([149, 149, cap + 1, 149], np.int32)
    kp[:, :149] = kept
    kp["x"][0, 5] = np.nan
    kp["size"][1, 7] = 0.0
    r = ctx.tracking_batch([1] * 4, [2] * 4, prev=(kp, n), cap=cap)
    print("info", [info_tuple(r["info"][i]) for i in range(4)], "stats", r["stats"])
    assert r["status"] == PAIR_FAILED
    for i in range(3):
        assert int(r["info"]["status"][i]) == INVALID_ARG and int(r["stats"]["status"][i]) == INVALID_ARG, i
        assert int(r["info"]["n_matches"][i]) == 0 and len(r["good"][i]) == 0, i
        assert r["poses"][i].tobytes() == IDENTITY.tobytes(), i
    assert differs(result_of(r, 3), good) is None, differs(result_of(r, 3), good)
    # the context still works
    again = result_of(ctx.tracking_batch([1], [2], prev=[kept], cap=cap), 0)
    assert differs(again, good) is None, differs(again, good)
    ctx.close()


# ---- 6. what the host refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_host_side_errors_leave_outputs_untouched(capi, synth, torch):
    ref, tgt, _ = pair(synth, 160, 96, 5)
    ctx = make_ctx(capi, 160, 96, [ref, tgt])
    cap = 64
    L = capi.lib()

    def fresh():
        out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, cap), capi.MATCH),
               np.zeros((1, cap), capi.KEYPOINT), np.zeros((1, cap), capi.KEYPOINT))
        for a in out:
            a.view(np.uint8)[...] = 0x5A
        return out

    def untouched(out):
        return all((a.view(np.uint8) == 0x5A).all() for a in out)

    P = capi.default_tracking_params
    bad = [(dict(ref=[2]), INVALID_ARG), (dict(tgt=[-1]), INVALID_ARG), (dict(ref=[], tgt=[]), INVALID_ARG),
           (dict(ref=[0, 0], tgt=[1, 1]), INVALID_ARG),                                    # n_pairs above max_pairs
           (dict(cap=0), INVALID_ARG), (dict(cap=capi.UWT_MATCH_MAX_ROWS + 1), CAPACITY),
           (dict(params=P(surf=dict(n_octaves=0))), INVALID_ARG), (dict(params=P(surf=dict(n_octave_layers=5))), INVALID_ARG),
           (dict(params=P(surf=dict(hessian_threshold=float("nan")))), INVALID_ARG),
           (dict(params=P(ransac=dict(distance=-1.0))), INVALID_ARG), (dict(params=P(ransac=dict(confidence=0.0))), INVALID_ARG),
           (dict(params=P(ransac=dict(max_hypotheses=0))), INVALID_ARG),
           (dict(params=P(ratio=float("nan"))), INVALID_ARG), (dict(params=P(ratio=float("inf"))), INVALID_ARG),
           (dict(params=P(min_matches=-1)), INVALID_ARG)]
    for kw, status in bad:
        out = fresh()
        with pytest.raises(capi.UwtError) as e:
            ctx.tracking_batch(kw.get("ref", [0]), kw.get("tgt", [1]), params=kw.get("params"), cap=kw.get("cap", cap), out=out)
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
        st = L.uwt_tracking_batch(ctx._h, 1, *[C.c_void_p(a[k]) for k in ("ref", "tgt")], None, cap,
                                  *[C.c_void_p(a[k]) for k in ("kp", "n", "poses", "stats", "info", "good", "kept_prev", "kept_cur")])
        assert st == INVALID_ARG and untouched(out) and L.uwt_last_error(ctx._h), hole

    # the asynchronous form: an input that is also an output of the same call
    s = device_set(torch, 1, cap, fill=0x5A5A5A5A)
    for alias in ("kept_prev", "kept_cur", "n_matches"):
        io = io_of(s)
        io["prev_kp"], io["n_prev"] = s["good"].data_ptr(), s["poses"].data_ptr()   # (never read: the call is refused)
        io["prev_kp" if alias != "n_matches" else "n_prev"] = s[alias].data_ptr()
        with pytest.raises(capi.UwtError) as e:
            ctx.tracking_batch_async([0], [1], io, cap=cap)
        assert e.value.status == INVALID_ARG, alias
    ctx.sync()
    assert all(bool((v == 0x5A5A5A5A).all()) for v in s.values())
    assert ctx.tracking_batch([0], [1], cap=cap)["status"] == OK   # the context still works
    ctx.close()


# ---- 7. forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_async_equals_sync_and_rows_past_a_count_stay(capi, synth, torch):
    ref, tgt, _ = pair(synth, 160, 96, 5)
    ctx = make_ctx(capi, 160, 96, [ref, tgt])
    cap = 128
    out = (np.zeros((1, 7), np.float32), np.zeros(1, capi.STATS), np.zeros(1, capi.TRACKING_INFO), np.zeros((1, cap), capi.MATCH),
           np.zeros((1, cap), capi.KEYPOINT), np.zeros((1, cap), capi.KEYPOINT))
    for a in out[3:]:
        a.view(np.uint8)[...] = 0x5A
    sync = ctx.tracking_batch([0], [1], cap=cap, out=out)
    n = int(sync["info"]["n_matches"][0])
    assert n == 49
    for a in out[3:]:
        assert (a[0, n:].view(np.uint8) == 0x5A).all() and not (a[0, :n].view(np.uint8) == 0x5A).all()
    s = device_set(torch, 1, cap, fill=0x5A5A5A5A)
    ctx.tracking_batch_async([0], [1], io_of(s), cap=cap)
    ctx.sync()
    got = fetch(capi, s)
    assert differs(result_of(got, 0), result_of(sync, 0)) is None, differs(result_of(got, 0), result_of(sync, 0))
    for k in ("good", "kept_prev", "kept_cur"):
        assert (got["raw"][k][0, n:] == 0x5A5A5A5A).all(), k
    # stats may be left out
    s2 = device_set(torch, 1, cap)
    io = io_of(s2)
    io["stats"] = None
    ctx.tracking_batch_async([0], [1], io, cap=cap)
    ctx.sync()
    got2 = result_of(fetch(capi, s2), 0)
    assert got2["pose"] == result_of(sync, 0)["pose"] and got2["info"] == result_of(sync, 0)["info"]
    assert not s2["stats"].cpu().numpy().any()
    ctx.close()


@pytest.mark.gpu
def test_gpu_growth_under_a_queued_async_call(capi, synth, torch):
    """a small asynchronous call is still queued when a call of the same context needs the scratch larger: both give, as bytes,
    what the same two calls give on fresh contexts"""
    ref, tgt, _ = pair(synth, 160, 96, 5)

    def run(ctx_small, ctx_large):
        s = device_set(torch, 1, 64)
        ctx_small.tracking_batch_async([0], [1], io_of(s), cap=64)
        large = result_of(ctx_large.tracking_batch([0], [1], cap=2048), 0)     # no sync in between
        ctx_small.sync()
        return result_of(fetch(capi, s), 0), large

    ctxs = [make_ctx(capi, 160, 96, [ref, tgt]) for _ in range(3)]
    got = run(ctxs[0], ctxs[0])
    want = run(ctxs[1], ctxs[2])
    for c in ctxs:
        c.close()
    assert got[0]["info"][5] == got[1]["info"][5] == 49
    assert got == want


@pytest.mark.gpu
def test_gpu_tuning_does_not_show(capi, synth):
    ref, tgt, _ = pair(synth, W, H, 31)
    ctx = make_ctx(capi, W, H, [ref, tgt])
    first = result_of(ctx.tracking_batch([0], [1]), 0)
    ctx.set_tuning(split=2, tail_update=2, first_poll=1, typed_loads=0, target_blocks=256)
    second = result_of(ctx.tracking_batch([0], [1]), 0)
    ctx.close()
    assert first["info"][5] == 174 and first == second


# ---- 8. the matcher over device descriptors -----------------------------------------------------------------------------------------
def device_match(ctx, capi, torch, pairs, cap, ratio, counts=None):
    """uwt_match_descriptors_device_async over `pairs` packed at stride cap; counts: the device counts when they are not the true ones"""
    norm, dim, cap, q, nq, t, nt = ctx._descriptor_block(pairs, None, cap)
    if counts is not None:
        nq, nt = (np.asarray(c, np.int32) for c in counts)
    to = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    dq, dt, dnq, dnt = to(q), to(t), to(nq), to(nt)
    P = len(pairs)
    dm = torch.full((P, cap, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dc = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_descriptors_device_async(P, dim, cap, dq.data_ptr(), dnq.data_ptr(), dt.data_ptr(), dnt.data_ptr(), dm.data_ptr(),
                                       dc.data_ptr(), ratio=ratio, norm=norm)
    ctx.sync()
    cnt = dc.cpu().numpy()
    raw = dm.cpu().numpy()
    m = raw.view(capi.MATCH).reshape(P, cap)
    for i in range(P):
        assert 0 <= cnt[i] <= cap and (raw[i, cnt[i]:] == 0x5A5A5A5A).all()   # the rows past a count are not written
    return [m[i, :cnt[i]].copy() for i in range(P)]


@pytest.mark.gpu
def test_gpu_match_device_equals_host_form(capi, synth, torch):
    ctx = capi.Context(capi.default_params(64, 48, 64.0, 64.0, 31.5, 23.5, n_levels=1, first_level=0, last_level=0, max_frames=2, max_pairs=1))
    for name, A, B, ratio, _, matches in match_cases.CASES:   # the hand-written cases: counts of 1 and 2, ties, both norms
        got = device_match(ctx, capi, torch, [(A, B)], 8, ratio)[0]
        assert got.tobytes() == np.array(matches, capi.MATCH).reshape(-1).tobytes(), name
        assert got.tobytes() == ctx.match_descriptors_batch([(A, B)], ratio=ratio, cap=8)[0].tobytes(), name
    for kind, dim in (("l2", 64), ("hamming", 32)):
        sets = [synth.descriptor_pair(50 + i, n, m, dim, kind)[:2] for i, (n, m) in enumerate([(130, 97), (0, 40), (40, 0), (1, 1), (1, 70),
                                                                                              (70, 1), (200, 65), (64, 64)])]
        for cap in (200, 333):   # 4 and 6 tiles: another cut of the train range, the same records
            want = ctx.match_descriptors_batch(sets, cap=cap)
            got = device_match(ctx, capi, torch, sets, cap, 0.65)
            assert sum(len(w) for w in want) > 100
            for i in range(len(sets)):
                assert got[i].tobytes() == want[i].tobytes(), (kind, cap, i)
        # cap 4096 with 3 rows
        small = [(sets[0][0][:3], sets[0][1][:3])]
        assert device_match(ctx, capi, torch, small, 4096, 0.65)[0].tobytes() == ctx.match_descriptors_batch(small, cap=4096)[0].tobytes()
        # a device count outside 0..cap gives that pair count 0; its neighbours are unaffected
        three = [sets[0], sets[6], sets[7]]
        want = ctx.match_descriptors_batch(three, cap=200)
        for counts in (([130, 201, 64], [97, 65, 64]), ([130, 200, 64], [97, -1, 64])):
            got = device_match(ctx, capi, torch, three, 200, 0.65, counts=counts)
            assert len(got[1]) == 0 and got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes(), (kind, counts)
    # host-side errors: nothing enqueued
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for kw, status in ((dict(n_pairs=0), INVALID_ARG), (dict(dim=6), INVALID_ARG), (dict(cap=0), INVALID_ARG), (dict(cap=4097), CAPACITY),
                       (dict(ratio=float("nan")), INVALID_ARG), (dict(norm=2), INVALID_ARG), (dict(dim=1024), CAPACITY)):
        a = dict(n_pairs=1, dim=4, cap=4, ratio=0.65, norm=0)
        a.update(kw)
        with pytest.raises(capi.UwtError) as e:
            ctx.match_descriptors_device_async(a["n_pairs"], a["dim"], a["cap"], *([z.data_ptr()] * 6), ratio=a["ratio"], norm=a["norm"])
        assert e.value.status == status, kw
    ctx.close()


@pytest.mark.gpu
def test_gpu_match_device_every_count_zero(capi, torch):
    """Two pairs, dim 64, cap 8, every device count 0, then one of them cap + 1 (taken as 0): the device form sizes k_knn2 by cap and
    launches it all the same; counts 0 and no match row written (device_match looks), which is what the host form gives, whose
    batch has no row and which launches no k_knn2 at all"""
    ctx = capi.Context(capi.default_params(64, 48, 64.0, 64.0, 31.5, 23.5, n_levels=1, first_level=0, last_level=0, max_frames=2, max_pairs=1))
    P, cap, dim = 2, 8, 64
    rows = np.random.default_rng(21).normal(size=(P, cap, dim)).astype(np.float32)
    none = np.zeros(P, np.int32)
    want = ctx.match_descriptors_batch(packed=(rows, none, rows, none))
    assert [len(w) for w in want] == [0, 0]
    pairs = [(rows[i], rows[i]) for i in range(P)]
    for counts in (([0, 0], [0, 0]), ([0, cap + 1], [0, 0])):
        got = device_match(ctx, capi, torch, pairs, cap, 0.65, counts=counts)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], counts
    ctx.close()


@pytest.mark.gpu
def test_gpu_track_sequence_chained_equals_live(capi, synth, torch):
    """tools/track_sequence.py --live --chained walks the sequence without a wait and gives the trajectory of --live"""
    import os
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "track_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    frames = list(seq(synth, 3))
    live = tool.track_live(W, H, TR.INTR[(W, H)], frames, None)
    chained = tool.track_live_chained(W, H, TR.INTR[(W, H)], frames, None)
    assert live[2] == chained[2] == [149, 131, 120, 119]
    assert live[0].view(np.uint32).tobytes() == chained[0].view(np.uint32).tobytes()
    assert [(s["status"], s["iterations"], s["n_valid"]) for s in live[1]] == [(s["status"], s["iterations"], s["n_valid"]) for s in chained[1]]


# ---- 9. the Python mirror -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_tracking_batch_mirror_equals_the_tracking_loop(capi, synth):
    T = importlib.import_module("uw-slam_amd.tracker")
    frames = seq(synth, 3)
    intr = TR.INTR[(W, H)]
    Kmat = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32)

    def fields(run):
        tracker = T.Tracker(False, max_frames=6)
        tracker.InitializePyramid(W, H, Kmat)
        rm = T.RobustMatcher(tracker)
        fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
        stats = run(tracker, rm, fr)
        tracker._ctx.close()
        return ([(f.n_matches_, np.asarray(f.keypoints_, np.float32).tobytes(), np.asarray(f.surf_keypoints_, capi.KEYPOINT).tobytes(),
                  np.asarray(f.rigid_transformation_, np.float32).view(np.uint32).tobytes()) for f in fr],
                [(s["status"], s["iterations"], s["n_valid"], np.float32(s["error"]).tobytes()) for s in stats])

    loop = fields(lambda tr, rm, fr: [T.Tracking(tr, rm, fr[k], fr[k + 1]) for k in range(4)])
    batch = fields(lambda tr, rm, fr: T.TrackingBatch(tr, rm, [(fr[k], fr[k + 1]) for k in range(4)]))
    assert [f[0] for f in loop[0]] == [149, 131, 120, 119, 119]
    assert batch == loop
