"""Robust weights and the bilinear sampler in the batched table calls (uwt_table_options; uwt_estimate_pose_candidates_batch_opt,
uwt_track_candidates_batch_opt_async, uwt_estimate_pose_features_batch_opt, uwt_track_features_batch_opt_async and the options
overloads of uw::Tracker): bit for bit against the oracle (candidate_points / patch_points + align_pair_points under the same
weights and sampler, one pair at a time) and against the per-pair path (uwt_obtain_*_points + uwt_estimate_pose_points) on a
context created with those weights and sampler.

Tukey over the bilinear sampler, (1, 1), is a mode only the options have: uwt_create and uwt_update_params refuse it, so no context
can run the per-pair path under it.  That mode is held to the oracle alone, and the refusal is asserted where the comparison with the
per-pair path is left out.

Every scene below ends with status 0 in the oracle under every mode, schedule and arithmetic set, so equality is strict for every
pair that is not built to fail; no seed had to be replaced for the f64-sum-at-an-f32-midpoint event (README "Parity")."""
import ctypes
import hashlib
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"160x96": (160, 96, (131.25, 131.25, 79.5, 47.5)),
         "165x99": (165, 99, (131.25, 130.0, 82.0, 49.0))}     # pitch 168, fx != fy: the general Jacobian form
MODES = [(1, 0), (2, 0), (0, 1), (2, 1), (1, 1)]               # (weights, sampler)
SCHEDULES = {"fixed": dict(max_iters=6, early_exit=0), "early": dict(max_iters=50, early_exit=1)}
LEVELS = dict(n_levels=4, first_level=2, last_level=0)
# EstimatePoseFeatures' locals (src/Tracker.cpp:633-640, 834, 856): what the oracle and the per-pair path are run with
FEATURES = dict(n_levels=4, first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002, handoff_scale_t=1)
N_SCENES = 6
# scene j's reference is slot 2j, its target slot 2j + 1: repeated reference slots, two pairs to another scene's target, one pair
# (slot, same slot)
CAND_REF = np.array([0, 2, 4, 6, 8, 10, 0, 4, 2, 6], np.int32)
CAND_TGT = np.array([1, 3, 5, 7, 9, 11, 3, 9, 2, 7], np.int32)
FEAT_REF = np.array([0, 2, 4, 6, 8, 10], np.int32)
FEAT_TGT = np.array([1, 3, 5, 7, 9, 11], np.int32)
FEAT_COUNTS = [60, 7, 1, 25, 0, 40]                             # 8, 1, 1, 3, 1 (fails) slices; the last pair has cut patches


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


_scenes = {}
_oracle = {}


def scenes(synth, size, depth):
    """N_SCENES rendered (ref, tgt, depth) pairs of one size, cached across the tests and the arithmetic sets."""
    key = (size[0], size[1], depth)
    if key not in _scenes:
        w, h, intr = size
        _scenes[key] = [synth.render_pair(w, h, *intr, seed=7300 + 17 * s, z=1.1 + 0.05 * s, max_t=0.01 + 0.002 * s,
                                          max_deg=0.3 + 0.1 * s, with_depth=depth)[:3] for s in range(N_SCENES)]
    return _scenes[key]


def frame(sc, slot):
    return sc[slot // 2][slot % 2]


def pair_digest(sc, depth, ref_slot, tgt_slot):
    """what an oracle result of one pair depends on beside its params: the two frames and the reference's depth"""
    h = hashlib.sha1(frame(sc, ref_slot).tobytes() + frame(sc, tgt_slot).tobytes())
    if depth:
        h.update(sc[ref_slot // 2][2].tobytes())
    return h.hexdigest()


def make_ctx(capi, size, depth, max_pairs, **over):
    w, h, intr = size
    if depth:
        over["has_depth"] = 1
    return capi.Context(capi.default_params(w, h, *intr, max_frames=2 * N_SCENES, max_pairs=max_pairs, **over))


def load(ctx, sc, depth):
    frames = np.stack([f for r, t, _ in sc for f in (r, t)])
    deps = np.stack([d for _, _, d in sc for _ in (0, 1)]) if depth else None
    ctx.upload_frames(0, frames, deps)
    ctx.build_pyramids(0, len(frames))
    ctx.apply_gradient(0, len(frames))


def feature_keypoints(w, h):
    rng = np.random.default_rng(31)
    kps = [rng.uniform([6, 6], [w - 7, h - 7], (n, 2)).astype(np.float32) for n in FEAT_COUNTS]
    kps[-1][:4] = np.array([[0, 0], [w - 1, h - 1], [2.5, h - 3.0], [w - 0.5, 4.0]], np.float32)   # patches cut by the border
    return kps


def oracle_candidates(O, arith, size, sc, depth, over, ref_slot, tgt_slot, threshold=20.0):
    """candidate_points on the iterated levels of the oracle's own pyramid + align_pair_points under `over`; computed once per
    (arithmetic set, size, depth, params, pair) and shared."""
    key = ("cand", arith, size[:2], depth, tuple(sorted(over.items())), pair_digest(sc, depth, ref_slot, tgt_slot))
    if key not in _oracle:
        w, h, intr = size
        p = O.default_params(w, h, *intr, **over)
        if depth:
            p.has_depth = 1
        r, d = frame(sc, ref_slot), sc[ref_slot // 2][2] if depth else None
        imgs = O.pyramid(r, p.n_levels)
        deps = O.pyramid(d, p.n_levels) if d is not None else None
        tables = {}
        for l in range(p.last_level, p.first_level + 1):
            L = O.level_intrinsics(p, l)
            mag = O.gradient_mag(*O.scharr3(imgs[l]))
            tables[l] = O.candidate_points(mag, deps[l] if deps is not None else None, threshold, grid=(L.w, L.h))[0]
        _oracle[key] = O.align_pair_points(p, r, frame(sc, tgt_slot), tables, ref_depth=d, want_trace=True)
    return _oracle[key]


def oracle_features(O, arith, size, sc, depth, over, ref_slot, tgt_slot, kp):
    key = ("feat", arith, size[:2], depth, tuple(sorted(over.items())), kp.tobytes(), pair_digest(sc, depth, ref_slot, tgt_slot))
    if key not in _oracle:
        w, h, intr = size
        p = O.default_params(w, h, *intr, **over)
        if depth:
            p.has_depth = 1
        d = sc[ref_slot // 2][2] if depth else None
        pts, _ = O.patch_points(kp, d, w, h)
        _oracle[key] = O.align_pair_points(p, frame(sc, ref_slot), frame(sc, tgt_slot), {0: pts}, ref_depth=d, want_trace=True)
    return _oracle[key]


def assert_is_oracle(i, oracle_result, pose, st, must_succeed=True):
    so, pose_cpu, tr = oracle_result
    assert st["status"] == so, (i, so, st)
    if must_succeed:
        assert so == 0, (i, so)
    if so == 0:
        assert st["iterations"] == len(tr) and st["n_valid"] == tr[-1]["n_valid"], (i, st, len(tr), tr[-1]["n_valid"])
        assert np.array_equal(pose, pose_cpu), (i, pose, pose_cpu)


def same_stats(a, b):
    return (a["status"], a["iterations"], a["n_valid"]) == (b["status"], b["iterations"], b["n_valid"]) and \
        np.float32(a["error"]).tobytes() == np.float32(b["error"]).tobytes()


def result_bytes(poses, stats):
    return np.ascontiguousarray(poses).tobytes() + b"".join(
        np.array([s["status"], s["iterations"], s["n_valid"]], np.int32).tobytes() + np.float32(s["error"]).tobytes() for s in stats)


def per_pair_candidates(ctx, ref_slot, tgt_slot, threshold=20.0):
    """uwt_obtain_candidate_points on every iterated level, then uwt_estimate_pose_points, under the context's weights and sampler"""
    p = ctx.params
    tables = {l: ctx.obtain_candidate_points(int(ref_slot), l, threshold)[0] for l in range(p.last_level, p.first_level + 1)}
    return ctx.estimate_pose_points(int(ref_slot), int(tgt_slot), tables)


def per_pair_context(capi, size, depth, over, weights, sampler):
    """A context whose params carry the mode, for the per-pair path; None for Tukey over the bilinear sampler, which uwt_create
    refuses (asserted)."""
    if (weights, sampler) == (1, 1):
        with pytest.raises(capi.UwtError) as e:
            make_ctx(capi, size, depth, 1, weights=1, sampler=1, **over)
        assert e.value.status == capi.ERR_INVALID_ARG
        return None
    return make_ctx(capi, size, depth, 1, weights=weights, sampler=sampler, **over)


def get_params(capi, c):
    p = capi.Params()
    assert capi.lib().uwt_get_params(c._h, ctypes.byref(p)) == 0
    return bytes(p)


def raw_opt_call(capi, ctx, kind, ref, tgt, opt, kp_block=None, threshold=20.0):
    """The synchronous _opt entries with `opt` a TableOptions or None (a null pointer).  Returns (status, poses, stats list)."""
    lib = capi.lib()
    i32, f32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    ref = np.ascontiguousarray(ref, np.int32)
    tgt = np.ascontiguousarray(tgt, np.int32)
    poses = np.zeros((max(ref.size, 1), 7), np.float32)
    stats = (capi.Stats * max(ref.size, 1))()
    o = ctypes.byref(opt) if opt is not None else None
    if kind == "candidates":
        st = lib.uwt_estimate_pose_candidates_batch_opt(ctx._h, ref.size, ref.ctypes.data_as(i32), tgt.ctypes.data_as(i32),
                                                        ctypes.c_double(threshold), o, poses.ctypes.data_as(f32), stats)
    else:
        kp, n = kp_block
        st = lib.uwt_estimate_pose_features_batch_opt(ctx._h, ref.size, ref.ctypes.data_as(i32), tgt.ctypes.data_as(i32),
                                                      kp.ctypes.data_as(f32), n.ctypes.data_as(i32), o, poses.ctypes.data_as(f32), stats)
    return st, poses[:ref.size], [dict(status=s.status, iterations=s.iterations, n_valid=s.n_valid, error=s.error)
                                  for s in stats[:ref.size]]


# ---- 1. candidates against the oracle and the per-pair path ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("depth", [False, True], ids=["none", "depth"])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("mode", MODES, ids=["tukey", "huber", "bilinear", "huber_bilinear", "tukey_bilinear"])
def test_gpu_candidates_opt_matches_oracle_and_per_pair_path(capi, O, synth, arith, size, depth, schedule, mode):
    size = SIZES[size]
    weights, sampler = mode
    over = dict(LEVELS, **SCHEDULES[schedule])
    sc = scenes(synth, size, depth)
    ctx = make_ctx(capi, size, depth, len(CAND_REF), **over)
    load(ctx, sc, depth)
    poses, stats = ctx.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, raise_on_pair_failure=True, weights=weights, sampler=sampler)
    mover = dict(over, weights=weights, sampler=sampler)
    for i in range(len(CAND_REF)):
        assert_is_oracle(i, oracle_candidates(O, arith, size, sc, depth, mover, CAND_REF[i], CAND_TGT[i]), poses[i], stats[i])
    pp = per_pair_context(capi, size, depth, over, weights, sampler)
    if pp is not None:
        load(pp, sc, depth)
        for i in range(len(CAND_REF)):
            pose, st = per_pair_candidates(pp, CAND_REF[i], CAND_TGT[i])
            assert np.array_equal(pose, poses[i]) and same_stats(st, stats[i]), (i, pose, poses[i], st, stats[i])
        pp.close()
    ctx.close()


# ---- 2. features likewise --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("depth", [False, True], ids=["none", "depth"])
def test_gpu_features_opt_matches_oracle_and_per_pair_path(capi, O, synth, arith, size, depth):
    size = SIZES[size]
    w, h, _ = size
    sc = scenes(synth, size, depth)
    kps = feature_keypoints(w, h)
    ctx = make_ctx(capi, size, depth, len(FEAT_REF), weights=2, **LEVELS)   # the context's own weights: ignored, as ever
    load(ctx, sc, depth)
    seen = {}
    for weights, sampler in [(0, 0)] + MODES:
        poses, stats = ctx.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps, weights=weights, sampler=sampler)
        mover = dict(FEATURES, weights=weights, sampler=sampler)
        for i in range(len(FEAT_REF)):
            res = oracle_features(O, arith, size, sc, depth, mover, FEAT_REF[i], FEAT_TGT[i], kps[i])
            assert_is_oracle(i, res, poses[i], stats[i], must_succeed=FEAT_COUNTS[i] > 0)
        assert stats[4]["status"] == capi.ERR_NO_VALID_POINTS and stats[4]["n_valid"] == 0
        pp = per_pair_context(capi, size, depth, FEATURES, weights, sampler)
        if pp is not None:
            load(pp, sc, depth)
            for i in range(len(FEAT_REF)):
                pts, _ = pp.obtain_patch_points(int(FEAT_REF[i]), kps[i])
                pose, st = pp.estimate_pose_points(int(FEAT_REF[i]), int(FEAT_TGT[i]), {0: pts})
                assert st["status"] == stats[i]["status"], (i, st, stats[i])
                if st["status"] == 0:
                    assert np.array_equal(pose, poses[i]) and same_stats(st, stats[i]), (weights, sampler, i, st, stats[i])
            pp.close()
        seen[(weights, sampler)] = poses[0].tobytes()
    assert len(set(seen.values())) == 6, "an option was ignored"
    plain, pst = ctx.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps)
    assert plain[0].tobytes() == seen[(0, 0)]
    ctx.close()


# ---- 3. identity options are the existing call ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_gpu_identity_options_are_the_existing_calls(capi, synth, schedule):
    size = SIZES["165x99"]
    w, h, _ = size
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, len(CAND_REF), **dict(LEVELS, **SCHEDULES[schedule]))
    load(ctx, sc, True)
    want = result_bytes(*ctx.estimate_pose_candidates_batch(CAND_REF, CAND_TGT))
    for opt in (None, capi.TableOptions()):
        st, poses, stats = raw_opt_call(capi, ctx, "candidates", CAND_REF, CAND_TGT, opt)
        assert st == 0 and result_bytes(poses, stats) == want
    assert result_bytes(*ctx.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=0, sampler=0)) == want
    kps = feature_keypoints(w, h)
    block = ctx._keypoint_block(kps)
    want = result_bytes(*ctx.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps))
    for opt in (None, capi.TableOptions()):
        st, poses, stats = raw_opt_call(capi, ctx, "features", FEAT_REF, FEAT_TGT, opt, kp_block=block)
        assert st == capi.ERR_PAIR_FAILED and result_bytes(poses, stats) == want   # (the pair without key points)
    ctx.close()


# ---- 4. independence ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("mode", [(1, 0), (2, 1)], ids=["tukey", "huber_bilinear"])
def test_gpu_candidates_opt_independent_of_batch_place_and_tuning(capi, synth, schedule, mode):
    """Each pair alone gives the bits it has in the batch and in a shuffled batch; uwt_tuning moves nothing; a second call gives
    the same bytes (the histograms were left clear)."""
    size = SIZES["165x99"]
    weights, sampler = mode
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, len(CAND_REF), **dict(LEVELS, **SCHEDULES[schedule]))
    load(ctx, sc, True)
    run = lambda r, t: ctx.estimate_pose_candidates_batch(r, t, raise_on_pair_failure=True, weights=weights, sampler=sampler)
    poses, stats = run(CAND_REF, CAND_TGT)
    assert result_bytes(*run(CAND_REF, CAND_TGT)) == result_bytes(poses, stats)
    for i in range(len(CAND_REF)):
        alone, st = run(CAND_REF[i:i + 1], CAND_TGT[i:i + 1])
        assert np.array_equal(alone[0], poses[i]) and same_stats(st[0], stats[i]), i
    perm = np.random.default_rng(2).permutation(len(CAND_REF))
    shuffled, sst = run(CAND_REF[perm], CAND_TGT[perm])
    assert result_bytes(shuffled, sst) == result_bytes(poses[perm], [stats[i] for i in perm])
    for tune in (dict(first_poll=1), dict(first_poll=64), dict(first_poll=3, target_blocks=256)):
        ctx.set_tuning(**tune)
        assert result_bytes(*run(CAND_REF, CAND_TGT)) == result_bytes(poses, stats), tune
    ctx.close()


@pytest.mark.gpu
def test_gpu_features_opt_independent_of_batch_and_place(capi, synth):
    size = SIZES["160x96"]
    w, h, _ = size
    sc = scenes(synth, size, True)
    kps = feature_keypoints(w, h)
    ctx = make_ctx(capi, size, True, len(FEAT_REF), **LEVELS)
    load(ctx, sc, True)
    run = lambda r, t, k: ctx.estimate_pose_features_batch(r, t, k, weights=2, sampler=1)
    poses, stats = run(FEAT_REF, FEAT_TGT, kps)
    assert result_bytes(*run(FEAT_REF, FEAT_TGT, kps)) == result_bytes(poses, stats)
    for i in range(len(FEAT_REF)):
        alone, st = run(FEAT_REF[i:i + 1], FEAT_TGT[i:i + 1], kps[i:i + 1])
        assert np.array_equal(alone[0], poses[i]) and same_stats(st[0], stats[i]), i
    perm = [3, 0, 5, 4, 1, 2]
    shuffled, sst = run(FEAT_REF[perm], FEAT_TGT[perm], [kps[i] for i in perm])
    assert result_bytes(shuffled, sst) == result_bytes(poses[perm], [stats[i] for i in perm])
    ctx.close()


@pytest.mark.gpu
def test_gpu_robust_tables_then_dense_robust_batch_share_the_histograms(capi, synth):
    """A robust table call followed by the dense robust batch (uwt_estimate_pose_batch under weights = 2) on the same context gives
    what a fresh context gives: both use the context's per-pair histograms, and each leaves them all-zero."""
    size = SIZES["160x96"]
    sc = scenes(synth, size, True)
    over = dict(LEVELS, max_iters=6, early_exit=0, weights=2)
    used, fresh = make_ctx(capi, size, True, len(CAND_REF), **over), make_ctx(capi, size, True, len(CAND_REF), **over)
    load(used, sc, True)
    load(fresh, sc, True)
    _, stats = used.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=1, sampler=0)
    assert all(s["status"] == 0 for s in stats)
    want = result_bytes(*fresh.estimate_pose_batch(CAND_REF, CAND_TGT))
    assert result_bytes(*used.estimate_pose_batch(CAND_REF, CAND_TGT)) == want
    again, astats = used.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=1, sampler=0)   # and the other way round
    first, fstats = fresh.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=1, sampler=0)
    assert result_bytes(again, astats) == result_bytes(first, fstats)
    used.close()
    fresh.close()


# ---- 5. options do not touch the context ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_options_neither_read_nor_change_the_context(capi, synth):
    size = SIZES["160x96"]
    w, h, _ = size
    sc = scenes(synth, size, False)
    over = dict(LEVELS, max_iters=6, early_exit=0)
    robust = make_ctx(capi, size, False, len(CAND_REF), weights=2, **over)
    plain = make_ctx(capi, size, False, len(CAND_REF), **over)
    load(robust, sc, False)
    load(plain, sc, False)
    before = get_params(capi, robust), get_params(capi, plain)
    with pytest.raises(capi.UwtError):                                    # the existing entry still refuses
        robust.estimate_pose_candidates_batch(CAND_REF, CAND_TGT)
    want = result_bytes(*plain.estimate_pose_candidates_batch(CAND_REF, CAND_TGT))
    assert result_bytes(*robust.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=0, sampler=0)) == want
    st, poses, stats = raw_opt_call(capi, robust, "candidates", CAND_REF, CAND_TGT, None)
    assert st == 0 and result_bytes(poses, stats) == want
    huber = result_bytes(*plain.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=2, sampler=1))   # a context created without
    assert result_bytes(*robust.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=2, sampler=1)) == huber and huber != want
    kps = feature_keypoints(w, h)
    plain.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps, weights=1, sampler=1)
    assert (get_params(capi, robust), get_params(capi, plain)) == before
    robust.close()
    plain.close()


# ---- 6. failure stays per pair ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True], ids=["none", "depth"])
@pytest.mark.parametrize("mode", [(1, 0), (2, 1)], ids=["tukey", "huber_bilinear"])
def test_gpu_candidates_opt_per_pair_failure(capi, O, synth, arith, depth, mode):
    size = SIZES["160x96"]
    w, h, _ = size
    weights, sampler = mode
    sc = list(scenes(synth, size, depth))
    sc[1] = (np.full((h, w), 128, np.uint8), sc[1][1], sc[1][2])            # a flat reference: no candidate anywhere
    if depth:
        sc[2] = (sc[2][0], sc[2][1], np.zeros((h, w), np.uint16))           # every candidate on zero depth
    over = dict(LEVELS, **SCHEDULES["early"])
    ctx = make_ctx(capi, size, depth, 8, **over)
    load(ctx, sc, depth)
    ref = np.array([2, 4, 6, 8, 10, 4, 2, 0], np.int32)
    tgt = ref + 1
    with pytest.raises(capi.UwtError) as e:
        ctx.estimate_pose_candidates_batch(ref, tgt, raise_on_pair_failure=True, weights=weights, sampler=sampler)
    assert e.value.status == capi.ERR_PAIR_FAILED
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt, weights=weights, sampler=sampler)
    bad = {2, 4} if depth else {2}
    mover = dict(over, weights=weights, sampler=sampler)
    good = make_ctx(capi, size, depth, 8, **over)                             # the same pairs where nothing fails beside them
    load(good, list(scenes(synth, size, depth)), depth)
    gposes, gstats = good.estimate_pose_candidates_batch(ref, tgt, weights=weights, sampler=sampler)
    for i in range(len(ref)):
        if int(ref[i]) in bad:
            assert stats[i]["status"] == capi.ERR_NO_VALID_POINTS and stats[i]["n_valid"] == 0, (i, stats[i])
            assert oracle_candidates(O, arith, size, sc, depth, mover, ref[i], tgt[i])[0] == capi.ERR_NO_VALID_POINTS
        else:
            assert np.array_equal(poses[i], gposes[i]) and same_stats(stats[i], gstats[i]), i
            assert_is_oracle(i, oracle_candidates(O, arith, size, sc, depth, mover, ref[i], tgt[i]), poses[i], stats[i])
    good.close()
    ctx.close()


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_opt_argument_errors(capi, synth):
    import torch
    size = SIZES["160x96"]
    w, h, _ = size
    sc = scenes(synth, size, False)
    ctx = make_ctx(capi, size, False, 4, **dict(LEVELS, **SCHEDULES["fixed"]))
    load(ctx, sc, False)
    lib = capi.lib()
    i32, f32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    r4, t4 = CAND_REF[:4].copy(), CAND_TGT[:4].copy()
    kps = feature_keypoints(w, h)[:4]
    block = ctx._keypoint_block(kps)
    d_poses = torch.zeros((8, 7), dtype=torch.float32, device="cuda")   # a real target, should a bad call be enqueued after all
    torch.cuda.synchronize()
    bad_opts = []
    for field, value in (("weights", -1), ("weights", 3), ("sampler", -1), ("sampler", 2)):
        o = capi.TableOptions()
        setattr(o, field, value)
        bad_opts.append(o)
    for k in (0, 5):
        o = capi.TableOptions(weights=2)
        o.reserved[k] = 1
        bad_opts.append(o)
    for o in bad_opts:
        assert raw_opt_call(capi, ctx, "candidates", r4, t4, o)[0] == capi.ERR_INVALID_ARG
        assert raw_opt_call(capi, ctx, "features", r4, t4, o, kp_block=block)[0] == capi.ERR_INVALID_ARG
        assert lib.uwt_track_candidates_batch_opt_async(ctx._h, 4, r4.ctypes.data_as(i32), t4.ctypes.data_as(i32), ctypes.c_double(20.0),
                                                        ctypes.byref(o), ctypes.c_void_p(d_poses.data_ptr()), None) == capi.ERR_INVALID_ARG
        assert lib.uwt_track_features_batch_opt_async(ctx._h, 4, r4.ctypes.data_as(i32), t4.ctypes.data_as(i32), block[0].ctypes.data_as(f32),
                                                      block[1].ctypes.data_as(i32), ctypes.byref(o), ctypes.c_void_p(d_poses.data_ptr()),
                                                      None) == capi.ERR_INVALID_ARG
    good = capi.TableOptions(weights=2, sampler=1)
    poses = np.zeros((8, 7), np.float32)
    for a, b in ((None, t4), (r4, None)):
        pa = a.ctypes.data_as(i32) if a is not None else None
        pb = b.ctypes.data_as(i32) if b is not None else None
        assert lib.uwt_estimate_pose_candidates_batch_opt(ctx._h, 4, pa, pb, ctypes.c_double(20.0), ctypes.byref(good),
                                                          poses.ctypes.data_as(f32), None) == capi.ERR_INVALID_ARG
        assert lib.uwt_estimate_pose_features_batch_opt(ctx._h, 4, pa, pb, block[0].ctypes.data_as(f32), block[1].ctypes.data_as(i32),
                                                        ctypes.byref(good), poses.ctypes.data_as(f32), None) == capi.ERR_INVALID_ARG
    assert lib.uwt_estimate_pose_candidates_batch_opt(ctx._h, 4, r4.ctypes.data_as(i32), t4.ctypes.data_as(i32), ctypes.c_double(20.0),
                                                      ctypes.byref(good), None, None) == capi.ERR_INVALID_ARG
    assert lib.uwt_track_candidates_batch_opt_async(ctx._h, 4, r4.ctypes.data_as(i32), t4.ctypes.data_as(i32), ctypes.c_double(20.0),
                                                    ctypes.byref(good), None, None) == capi.ERR_INVALID_ARG
    cases = [(CAND_REF[:5], CAND_TGT[:5]),                                           # n_pairs > max_pairs
             (np.zeros(0, np.int32), np.zeros(0, np.int32)),                         # n_pairs = 0
             (np.array([0, 2 * N_SCENES], np.int32), t4[:2]),                        # a slot out of range
             (r4[:2], np.array([1, -1], np.int32))]
    for r, t in cases:
        for call in (lambda: ctx.estimate_pose_candidates_batch(r, t, weights=2, sampler=1),
                     lambda: ctx.track_candidates_batch_async(r, t, d_poses.data_ptr(), weights=2, sampler=1),
                     lambda: ctx.estimate_pose_features_batch(r, t, kps[:len(r)], weights=2, sampler=1),
                     lambda: ctx.track_features_batch_async(r, t, kps[:len(r)], d_poses.data_ptr(), weights=2, sampler=1)):
            with pytest.raises(capi.UwtError) as e:
                call()
            assert e.value.status == capi.ERR_INVALID_ARG
    ctx.sync()
    assert not d_poses.cpu().numpy().any()                                           # nothing was enqueued
    # the context is usable afterwards
    poses, stats = ctx.estimate_pose_candidates_batch(r4, t4, raise_on_pair_failure=True, weights=2, sampler=1)
    fresh = make_ctx(capi, size, False, 4, **dict(LEVELS, **SCHEDULES["fixed"]))
    load(fresh, sc, False)
    assert result_bytes(poses, stats) == result_bytes(*fresh.estimate_pose_candidates_batch(r4, t4, weights=2, sampler=1))
    fresh.close()
    ctx.close()


# ---- 8. async equals sync -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_gpu_opt_async_equals_sync(capi, synth, schedule):
    """Into device buffers the asynchronous forms equal the synchronous ones, two calls queued without a wait."""
    import torch
    size = SIZES["165x99"]
    w, h, _ = size
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, len(CAND_REF), **dict(LEVELS, **SCHEDULES[schedule]))
    load(ctx, sc, True)
    n = len(CAND_REF)
    want, wst = ctx.estimate_pose_candidates_batch(CAND_REF, CAND_TGT, weights=1, sampler=0)
    want2, _ = ctx.estimate_pose_candidates_batch(CAND_REF[::-1].copy(), CAND_TGT[::-1].copy(), weights=2, sampler=1)
    d_poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    d_stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # torch's fill kernels run on torch's stream, not on the context's
    ctx.track_candidates_batch_async(CAND_REF, CAND_TGT, d_poses.data_ptr(), d_stats.data_ptr(), weights=1, sampler=0)
    ctx.track_candidates_batch_async(CAND_REF[::-1].copy(), CAND_TGT[::-1].copy(), d2.data_ptr(), weights=2, sampler=1)
    ctx.sync()
    st = d_stats.cpu().numpy()
    assert np.array_equal(d_poses.cpu().numpy(), want) and np.array_equal(d2.cpu().numpy(), want2)
    assert [tuple(r[:3]) for r in st] == [(s["status"], s["iterations"], s["n_valid"]) for s in wst]
    assert st[:, 3].astype(np.int32).tobytes() == np.array([s["error"] for s in wst], np.float32).tobytes()
    kps = feature_keypoints(w, h)
    m = len(FEAT_REF)
    fwant, fst = ctx.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps, weights=2, sampler=0)
    fwant2, _ = ctx.estimate_pose_features_batch(FEAT_REF, FEAT_TGT, kps, weights=0, sampler=1)
    f1 = torch.zeros((m, 7), dtype=torch.float32, device="cuda")
    s1 = torch.zeros((m, 4), dtype=torch.int32, device="cuda")
    f2 = torch.zeros((m, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.track_features_batch_async(FEAT_REF, FEAT_TGT, kps, f1.data_ptr(), s1.data_ptr(), weights=2, sampler=0)
    ctx.track_features_batch_async(FEAT_REF, FEAT_TGT, kps, f2.data_ptr(), weights=0, sampler=1)
    ctx.sync()
    assert np.array_equal(f1.cpu().numpy(), fwant) and np.array_equal(f2.cpu().numpy(), fwant2)
    assert [tuple(r[:3]) for r in s1.cpu().numpy()] == [(s["status"], s["iterations"], s["n_valid"]) for s in fst]
    ctx.close()


# ---- 9. the C++ mirror --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_tables_robust_cpp_mirror_matches_oracle(capi, O, synth, tmp_path, arith):
    """uw::Tracker::EstimatePoseCandidatesBatch / ::EstimatePoseFeaturesBatch with uwt_table_options {Huber, bilinear} on three
    160 x 96 pairs against the oracle."""
    w, h, intr = SIZES["160x96"]
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_tables_robust")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_tables_robust.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    sc = scenes(synth, SIZES["160x96"], False)[:3]
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(r.tobytes() + t.tobytes() for r, t, _ in sc))
    out = subprocess.run([exe, str(raw), str(w), str(h), "3", "2", "1", arith], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    kp = np.array([[10.0 + (k % 10) * 14.5, 10.0 + (k // 10) * 30.25] for k in range(30)], np.float32)
    for tag, over in (("CAND", dict(n_levels=5, first_level=2, last_level=0, max_iters=6, early_exit=0)), ("FEAT", dict(FEATURES, n_levels=5))):
        lines = [ln.split() for ln in out.stdout.strip().splitlines() if ln.startswith(tag)]
        assert len(lines) == 3
        for i, ln in enumerate(lines):
            pose = np.array([float(v) for v in ln[2:9]], np.float32)
            mover = dict(over, weights=2, sampler=1)
            if tag == "CAND":
                so, pose_cpu, tr = oracle_candidates(O, arith, SIZES["160x96"], sc, False, mover, 2 * i, 2 * i + 1)
            else:
                so, pose_cpu, tr = oracle_features(O, arith, SIZES["160x96"], sc, False, mover, 2 * i, 2 * i + 1, kp)
            assert so == 0 and int(ln[10]) == 0 and int(ln[9]) == len(tr) and int(ln[11]) == tr[-1]["n_valid"], (tag, i, ln)
            assert np.array_equal(pose, pose_cpu), (tag, i, pose, pose_cpu)
