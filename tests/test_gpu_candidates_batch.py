"""Semi-dense tracking for a batch of pairs (Tracker::ObtainCandidatePoints(previous), src/Tracker.cpp:1314-1362, then
EstimatePose(previous, current), :362-597, over those tables) with device-resident candidate tables:
uwt_estimate_pose_candidates_batch, uwt_track_candidates_batch_async and uw::Tracker::EstimatePoseCandidatesBatch, bit for bit
against the oracle's candidate_points per level + align_pair_points one pair at a time, and against the per-pair path
(uwt_obtain_candidate_points per level + uwt_estimate_pose_points) on the same context."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGA = (640, 480, (525.0, 525.0, 319.5, 239.5))
EUROC = (736, 480, (458.654, 457.296, 367.215, 248.375))      # fx != fy
ODD = (733, 471, (458.654, 457.296, 366.0, 235.0))
SCHEDULES = {"reference": {},                                   # the context's defaults: levels 4 -> 1, 50 iterations, early exit
             "fixed4x10": dict(max_iters=10, early_exit=0)}
N_SCENES = 6


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


_scenes = {}


def scenes(synth, size, depth):
    """N_SCENES rendered (ref, tgt, depth) pairs of one size, cached across the arithmetic sets."""
    key = (size[0], size[1], depth)
    if key not in _scenes:
        w, h, intr = size
        _scenes[key] = [synth.render_pair(w, h, *intr, seed=6300 + 17 * s, z=1.1 + 0.05 * s, max_t=0.01 + 0.002 * s,
                                          max_deg=0.3 + 0.1 * s, with_depth=depth)[:3] for s in range(N_SCENES)]
    return _scenes[key]


def make_ctx(capi, size, depth, max_frames, max_pairs, **over):
    w, h, intr = size
    if depth:
        over["has_depth"] = 1
    return capi.Context(capi.default_params(w, h, *intr, max_frames=max_frames, max_pairs=max_pairs, **over))


def load(ctx, sc, depth):
    frames = np.stack([f for r, t, _ in sc for f in (r, t)])
    deps = np.stack([d for _, _, d in sc for _ in (0, 1)]) if depth else None
    ctx.upload_frames(0, frames, deps)
    ctx.build_pyramids(0, len(frames))
    ctx.apply_gradient(0, len(frames))


def pair_list(n, seed):
    """n pairs over the scenes in a seeded order: scene j's reference (slot 2j) to its own target (slot 2j + 1) or, every fifth
    pair, to the next scene's target; reference slots repeat."""
    rng = np.random.default_rng(seed)
    js = rng.integers(0, N_SCENES, n)
    ref = (2 * js).astype(np.int32)
    tgt = np.array([2 * ((j + 1) % N_SCENES) + 1 if i % 5 == 4 else 2 * j + 1 for i, j in enumerate(js)], np.int32)
    return ref, tgt


def oracle_params(O, size, depth, over):
    w, h, intr = size
    p = O.default_params(w, h, *intr, **over)
    if depth:
        p.has_depth = 1
    return p


def oracle_tables(O, p, img, dep, threshold=20.0):
    """ObtainCandidatePoints on the iterated levels of the oracle's own pyramid, on each level's point grid."""
    imgs = O.pyramid(img, p.n_levels)
    deps = O.pyramid(dep, p.n_levels) if dep is not None else None
    tables = {}
    for l in range(p.last_level, p.first_level + 1):
        L = O.level_intrinsics(p, l)
        mag = O.gradient_mag(*O.scharr3(imgs[l]))
        tables[l] = O.candidate_points(mag, deps[l] if deps is not None else None, threshold, grid=(L.w, L.h))[0]
    return tables


def oracle_pair(O, size, sc, depth, over, ref_slot, tgt_slot, threshold=20.0):
    r, _, d = sc[ref_slot // 2]
    t = sc[tgt_slot // 2][1]
    p = oracle_params(O, size, depth, over)
    tables = oracle_tables(O, p, r, d if depth else None, threshold)
    return O.align_pair_points(p, r, t, tables, ref_depth=d if depth else None, want_trace=True)


def assert_matches_oracle(O, size, sc, depth, over, ref, tgt, poses, stats):
    """Every pair's status as the oracle's; where the oracle succeeds, the pose bit for bit and iterations / n_valid as its
    trace.  Returns how many pairs succeeded.  (The synthetic texture saturates gradient_: its mean is ~230, and on some
    scenes no cell of level 2 exceeds mean + 20, so those pairs fail with ERR_NO_VALID_POINTS in the oracle and here alike.)"""
    ok = 0
    for i in range(len(ref)):
        so, pose_cpu, tr = oracle_pair(O, size, sc, depth, over, ref[i], tgt[i])
        assert stats[i]["status"] == so, (i, so, stats[i])
        if so == 0:
            assert stats[i]["iterations"] == len(tr) and stats[i]["n_valid"] == tr[-1]["n_valid"], (i, stats[i], len(tr))
            assert np.array_equal(poses[i], pose_cpu), (i, poses[i], pose_cpu)
            ok += 1
    return ok


def per_pair_path(ctx, ref_slot, tgt_slot, threshold=20.0):
    """uwt_obtain_candidate_points on every iterated level, then uwt_estimate_pose_points over those tables."""
    p = ctx.params
    tables = {l: ctx.obtain_candidate_points(int(ref_slot), l, threshold)[0] for l in range(p.last_level, p.first_level + 1)}
    return ctx.estimate_pose_points(int(ref_slot), int(tgt_slot), tables)


def get_params(capi, c):
    p = capi.Params()
    assert capi.lib().uwt_get_params(c._h, ctypes.byref(p)) == 0
    return bytes(p)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("size,depth", [(VGA, False), (VGA, True), (EUROC, False), (ODD, False)],
                         ids=["640x480", "640x480_depth", "736x480", "733x471"])
def test_gpu_candidates_batch_matches_oracle(capi, O, synth, size, depth, schedule):
    over = SCHEDULES[schedule]
    sc = scenes(synth, size, depth)
    ctx = make_ctx(capi, size, depth, 2 * N_SCENES, 8, **over)
    load(ctx, sc, depth)
    ref, tgt = pair_list(8, seed=3)
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt)
    assert assert_matches_oracle(O, size, sc, depth, over, ref, tgt, poses, stats) >= len(ref) // 2
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_candidates_batch_equals_per_pair_path(capi, synth, depth, schedule):
    """Poses and every uwt_stats field, bit for bit, against the per-pair path on the same context."""
    size = VGA
    sc = scenes(synth, size, depth)
    ctx = make_ctx(capi, size, depth, 2 * N_SCENES, 8, **SCHEDULES[schedule])
    load(ctx, sc, depth)
    ref, tgt = pair_list(8, seed=4)
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt)
    assert sum(s["status"] == 0 for s in stats) >= len(ref) // 2
    for i in range(len(ref)):
        pose, st = per_pair_path(ctx, ref[i], tgt[i])
        assert np.array_equal(pose, poses[i]), i
        assert st["status"] == stats[i]["status"] and st["iterations"] == stats[i]["iterations"], (i, st, stats[i])
        assert st["n_valid"] == stats[i]["n_valid"] and np.float32(st["error"]).tobytes() == np.float32(stats[i]["error"]).tobytes()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_gpu_candidates_batch_independent_of_batch_and_tuning(capi, synth, schedule):
    """Each pair alone gives the bits it gets in a batch of 16 in shuffled order with repeated slots, and uwt_tuning
    (first_poll 1 / 3 / 64, target_blocks) does not move any pose."""
    size = VGA
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, 2 * N_SCENES, 16, **SCHEDULES[schedule])
    load(ctx, sc, True)
    ref, tgt = pair_list(16, seed=8)
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt)
    assert sum(s["status"] == 0 for s in stats) >= len(ref) // 2
    assert len(set(ref.tolist())) < len(ref)
    for i in range(len(ref)):
        alone, st = ctx.estimate_pose_candidates_batch(ref[i:i + 1], tgt[i:i + 1])
        assert np.array_equal(alone[0], poses[i]) and st[0] == stats[i], i
    perm = np.random.default_rng(2).permutation(len(ref))
    shuffled, sst = ctx.estimate_pose_candidates_batch(ref[perm], tgt[perm])
    assert np.array_equal(shuffled, poses[perm]) and sst == [stats[i] for i in perm]
    for over in (dict(first_poll=1), dict(first_poll=64), dict(first_poll=3, target_blocks=256)):
        ctx.set_tuning(**over)
        again, ast = ctx.estimate_pose_candidates_batch(ref, tgt)
        assert np.array_equal(again, poses) and ast == stats, over
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("over", [dict(first_level=3, last_level=0, max_iters=8),
                                  dict(first_level=2, last_level=2, max_iters=30, gain=20.0),
                                  dict(first_level=4, last_level=1, max_iters=6, early_exit=0, handoff_scale_t=1, gain=35.0,
                                       epsilon=0.01, initial_error=1e5)],
                         ids=["levels3to0", "level2_gain", "handoff_scale_t"])
def test_gpu_candidates_batch_honours_params(capi, O, synth, over):
    """The context's schedule and solver constants are the call's (against the oracle under the same params); the params are
    read, not changed."""
    size = VGA
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, 2 * N_SCENES, 6, **over)
    load(ctx, sc, True)
    before = get_params(capi, ctx)
    ref, tgt = pair_list(6, seed=12)
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt)
    assert get_params(capi, ctx) == before
    assert assert_matches_oracle(O, size, sc, True, over, ref, tgt, poses, stats) >= len(ref) // 2
    default = make_ctx(capi, size, True, 2 * N_SCENES, 6)
    load(default, sc, True)
    dp, _ = default.estimate_pose_candidates_batch(ref, tgt)
    assert not np.array_equal(dp, poses)
    default.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("over", [dict(weights=1), dict(sampler=1), dict(weights=2, sampler=1)])
def test_gpu_candidates_batch_refuses_weights_and_sampler(capi, synth, over):
    size = VGA
    sc = scenes(synth, size, False)
    ctx = make_ctx(capi, size, False, 2 * N_SCENES, 4, **over)
    load(ctx, sc, False)
    with pytest.raises(capi.UwtError) as e:
        ctx.estimate_pose_candidates_batch([0], [1])
    assert e.value.status == capi.ERR_INVALID_ARG and "uwt_estimate_pose_points" in str(e.value)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_candidates_batch_per_pair_failure(capi, O, synth, depth):
    """A flat reference frame (and, with depth, a reference whose depth bytes are all zero) fails on its own:
    ERR_NO_VALID_POINTS in its stats, ERR_PAIR_FAILED from the synchronous call, the other pairs' bits unchanged."""
    size = VGA
    w, h, _ = size
    sc = list(scenes(synth, size, depth))
    flat = np.full((h, w), 128, np.uint8)
    sc[1] = (flat, sc[1][1], sc[1][2])
    if depth:
        sc[2] = (sc[2][0], sc[2][1], np.zeros((h, w), np.uint16))
    ctx = make_ctx(capi, size, depth, 2 * N_SCENES, 8)
    load(ctx, sc, depth)
    ref = np.array([2, 4, 6, 8, 10, 4, 2], np.int32)
    tgt = ref + 1
    with pytest.raises(capi.UwtError) as e:
        ctx.estimate_pose_candidates_batch(ref, tgt, raise_on_pair_failure=True)
    assert e.value.status == capi.ERR_PAIR_FAILED
    poses, stats = ctx.estimate_pose_candidates_batch(ref, tgt)
    bad = {2, 4} if depth else {2}
    for i in range(len(ref)):
        if ref[i] in bad:
            assert stats[i]["status"] == capi.ERR_NO_VALID_POINTS and stats[i]["n_valid"] == 0, (i, stats[i])
            pose, st = per_pair_path(ctx, ref[i], tgt[i])
            assert st["status"] == stats[i]["status"]
        else:
            alone, ast = ctx.estimate_pose_candidates_batch(ref[i:i + 1], tgt[i:i + 1])
            assert np.array_equal(alone[0], poses[i]) and ast[0] == stats[i], i
    assert assert_matches_oracle(O, size, sc, depth, {}, ref, tgt, poses, stats) >= 3
    ctx.close()


@pytest.mark.gpu
def test_gpu_candidates_batch_argument_errors(capi, O, synth):
    import torch
    size = VGA
    sc = scenes(synth, size, False)
    ctx = make_ctx(capi, size, False, 2 * N_SCENES, 4)
    load(ctx, sc, False)
    ref, tgt = pair_list(5, seed=14)
    lib = capi.lib()
    i32 = ctypes.POINTER(ctypes.c_int32)
    poses = np.zeros((8, 7), np.float32)
    pp = poses.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    r4, t4 = np.array([2, 4, 6, 8], np.int32), np.array([3, 5, 7, 9], np.int32)
    for a, b in ((None, t4), (r4, None)):
        st = lib.uwt_estimate_pose_candidates_batch(ctx._h, 4, a.ctypes.data_as(i32) if a is not None else None,
                                                    b.ctypes.data_as(i32) if b is not None else None, ctypes.c_double(20.0), pp, None)
        assert st == capi.ERR_INVALID_ARG
        st = lib.uwt_track_candidates_batch_async(ctx._h, 4, a.ctypes.data_as(i32) if a is not None else None,
                                                  b.ctypes.data_as(i32) if b is not None else None, ctypes.c_double(20.0), None, None)
        assert st == capi.ERR_INVALID_ARG
    st = lib.uwt_estimate_pose_candidates_batch(ctx._h, 0, r4.ctypes.data_as(i32), t4.ctypes.data_as(i32), ctypes.c_double(20.0), pp, None)
    assert st == capi.ERR_INVALID_ARG
    d_poses = torch.zeros((8, 7), dtype=torch.float32, device="cuda")   # a real target, should a bad call be enqueued after all
    torch.cuda.synchronize()
    cases = [(ref, tgt, 20.0),                                                  # n_pairs > max_pairs
             (np.array([0, 2 * N_SCENES], np.int32), tgt[:2], 20.0),            # a slot out of range
             (ref[:2], np.array([1, -1], np.int32), 20.0),
             (ref[:2], tgt[:2], float("nan")),                                  # a non-finite threshold
             (ref[:2], tgt[:2], float("inf"))]
    for r, t, thr in cases:
        with pytest.raises(capi.UwtError) as e:
            ctx.estimate_pose_candidates_batch(r, t, threshold=thr)
        assert e.value.status == capi.ERR_INVALID_ARG
        with pytest.raises(capi.UwtError) as e:
            ctx.track_candidates_batch_async(r, t, d_poses.data_ptr(), threshold=thr)
        assert e.value.status == capi.ERR_INVALID_ARG
    # the context is usable afterwards
    poses, stats = ctx.estimate_pose_candidates_batch(r4, t4, raise_on_pair_failure=True)
    assert assert_matches_oracle(O, size, sc, False, {}, r4, t4, poses, stats) == 4
    ctx.close()


@pytest.mark.gpu
def test_gpu_track_candidates_batch_async_equals_sync(capi, synth):
    """Into device buffers the asynchronous form equals the synchronous one, twice in a row without a wait; behind
    upload_frames_async into the very slots it read, the next call sees the new frames."""
    import torch
    size = VGA
    w, h, _ = size
    sc = scenes(synth, size, True)
    ctx = make_ctx(capi, size, True, 2 * N_SCENES, 16)
    load(ctx, sc, True)
    ref, tgt = pair_list(16, seed=21)
    want, wst = ctx.estimate_pose_candidates_batch(ref, tgt)
    d_poses = torch.zeros((16, 7), dtype=torch.float32, device="cuda")
    d_stats = torch.zeros((16, 4), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((16, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # torch's fill kernels run on torch's stream, not on the context's
    ctx.track_candidates_batch_async(ref, tgt, d_poses.data_ptr(), d_stats.data_ptr())
    ctx.track_candidates_batch_async(ref[::-1].copy(), tgt[::-1].copy(), d2.data_ptr())
    ctx.sync()
    st = d_stats.cpu().numpy()
    assert np.array_equal(d_poses.cpu().numpy(), want) and np.array_equal(d2.cpu().numpy(), want[::-1])
    assert [tuple(r[:3]) for r in st] == [(s["status"], s["iterations"], s["n_valid"]) for s in wst]
    # new frames land in every slot the batch read while it may still run
    new = scenes(synth, size, True)[::-1]
    pg = capi.pinned_empty((2 * N_SCENES, h, w), np.uint8)
    pd = capi.pinned_empty((2 * N_SCENES, h, w), np.uint16)
    pg[:] = np.stack([f for r, t, _ in new for f in (r, t)])
    pd[:] = np.stack([d for _, _, d in new for _ in (0, 1)])
    ctx.track_candidates_batch_async(ref, tgt, d_poses.data_ptr())
    ctx.upload_frames_async(0, pg, pd)
    ctx.build_pyramids(0, 2 * N_SCENES)
    ctx.apply_gradient(0, 2 * N_SCENES)
    ctx.track_candidates_batch_async(ref, tgt, d2.data_ptr())
    ctx.sync()
    assert np.array_equal(d_poses.cpu().numpy(), want)
    fresh = make_ctx(capi, size, True, 2 * N_SCENES, 16)
    load(fresh, new, True)
    want_new, _ = fresh.estimate_pose_candidates_batch(ref, tgt)
    assert np.array_equal(d2.cpu().numpy(), want_new) and not np.array_equal(want_new, want)
    fresh.close()
    ctx.close()


@pytest.mark.gpu
def test_gpu_candidates_growth_under_a_queued_async_call(capi, synth):
    """A one-pair asynchronous call is still queued when a synchronous call of the same context for four pairs needs every buffer
    of the stage larger: both give, as bytes, what the same two calls give on fresh contexts."""
    import torch
    size = (160, 96, (131.25, 131.25, 79.5, 47.5))
    sc = scenes(synth, size, True)
    ref, tgt = pair_list(4, seed=33)

    def run(ctx_small, ctx_large):
        d_poses = torch.zeros((1, 7), dtype=torch.float32, device="cuda")
        d_stats = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # torch's fill kernels run on torch's stream, not on the context's
        ctx_small.track_candidates_batch_async(ref[:1], tgt[:1], d_poses.data_ptr(), d_stats.data_ptr())
        poses, stats = ctx_large.estimate_pose_candidates_batch(ref, tgt)     # no sync in between
        ctx_small.sync()
        assert d_stats.cpu().numpy()[0, 0] == 0 and all(s["status"] == 0 for s in stats)   # every alignment ran to its end
        return (d_poses.cpu().numpy().tobytes() + d_stats.cpu().numpy().tobytes(),
                poses.tobytes() + repr([sorted(s.items()) for s in stats]).encode())

    ctxs = [make_ctx(capi, size, True, 2 * N_SCENES, 4) for _ in range(3)]
    for c in ctxs:
        load(c, sc, True)
    got = run(ctxs[0], ctxs[0])
    want = run(ctxs[1], ctxs[2])
    for c in ctxs:
        c.close()
    assert got == want


@pytest.mark.gpu
def test_gpu_candidates_batch_cpp_mirror_matches_oracle(capi, O, synth, tmp_path, arith):
    """uw::Tracker::EstimatePoseCandidatesBatch at 640 x 480 on three pairs against the oracle (the tracker's defaults: the
    reference schedule)."""
    w, h = 640, 480
    f = 525.0 * w / 640.0
    intr = (f, f, w / 2 - 0.5, h / 2 - 0.5)
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_candidates_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_candidates_batch.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pairs = [synth.render_pair(w, h, *intr, seed=s, z=1.2)[:2] for s in (5400, 5401, 5403)]   # candidates on every level
    raw = tmp_path / "frames.raw"
    raw.write_bytes(b"".join(r.tobytes() + t.tobytes() for r, t in pairs))
    out = subprocess.run([exe, str(raw), str(w), str(h), "3", arith], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines() if ln.startswith("PAIR")]
    assert len(lines) == 3
    for i, ln in enumerate(lines):
        pose = np.array([float(v) for v in ln[2:9]], np.float32)
        p = O.default_params(w, h, *intr)
        tables = oracle_tables(O, p, pairs[i][0], None)
        so, pose_cpu, tr = O.align_pair_points(p, pairs[i][0], pairs[i][1], tables, want_trace=True)
        assert so == 0 and int(ln[10]) == 0 and int(ln[9]) == len(tr) and int(ln[11]) == tr[-1]["n_valid"]
        assert np.array_equal(pose, pose_cpu), (i, pose, pose_cpu)
