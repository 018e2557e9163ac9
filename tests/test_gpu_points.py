"""The sparse point producers on the device — k_grad_mag_slots, k_candidates_slots<false / true> with k_scan_counts, k_patch_points_batch,
k_add_patch_points and the sweep's copy of the candidate selection — on the designed cases of tests/points_cases.py, in every form that
contains them, bit for bit against the numpy restatement (tests/points_ref.py; tests/seeded_ref.py's loop over the restatement's tables for
the alignments, tests/cloud_ref.py over them for the cloud).  tests/test_points_cpu.py shows, without a GPU, which classes each case
reaches and that each of 22 plausible mistakes changes the expectation of a named case.  Every comparison is one of bytes or integers.

Every input is inside the contract include/uwt.h states, or is refused on the host with nothing enqueued."""
import importlib

import numpy as np
import pytest

import cloud_ref as CR
import guard_bands as GB
import points_cases as PC
import points_ref as PR
import seeded_ref as SR

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, NO_VALID_POINTS = 0, 1, 2
W0, H0 = 64, 48
PATCHES = PC.patch_sets(W0, H0)
PATCH_BY_NAME = {p.name: p for p in PATCHES}
# EstimatePoseFeatures' locals (src/Tracker.cpp:633-640, 834, 856): what the live call runs under
FEATURES = dict(first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002, handoff_scale_t=1)
SCHEDULE = dict(first_level=2, last_level=0, max_iters=3, early_exit=0)
GUARD = 256


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def make_ctx(capi, geom, max_pairs=8, depth=None, **over):
    """a context of a geometry with its designed frames (and depth planes) resident in every slot, pyramids built, gradients applied"""
    w, h, nl, slots, has = PC.GEOMS[geom]
    has = has if depth is None else depth
    params = dict(dict(n_levels=nl, first_level=nl - 1, last_level=0), **over)
    ctx = capi.Context(capi.default_params(w, h, *PC.intr(w, h), max_frames=slots, max_pairs=max_pairs, has_depth=int(has), **params))
    ctx.upload_frames(0, np.stack(PC.frames_of(geom)), np.stack(PC.depths_of(geom)) if has else None)
    ctx.build_pyramids(0, slots)
    ctx.apply_gradient(0, slots)
    return ctx


def same_rows(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- 1. the staged entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.one_arith
@pytest.mark.parametrize("geom", list(PC.GEOMS))
def test_staged_gradient_magnitude_and_candidates(capi, O, geom):
    """uwt_gradient_magnitude on every level of every slot; uwt_obtain_candidate_points_batch (and the one-frame entry) on every case of
    the geometry: rows, order and full counts; cap truncation; the level's pitch and grid are what the restatement assumes"""
    w, h, nl, slots, has = PC.GEOMS[geom]
    ctx = make_ctx(capi, geom)
    for l in range(nl):
        L = ctx.level_info(l)
        for s in range(slots):
            mag, _, grid = PC.level_planes(O, geom, s)[l]
            assert (L.w, L.h) == grid and (L.img_h, L.img_w) == mag.shape and L.pitch == PR.pitch_of(L.img_w)
            assert ctx.gradient_magnitude(s, l).tobytes() == mag.tobytes(), (geom, s, l)
    cases = [c for c in PC.CANDIDATES if c.geom == geom]
    for case in sorted(cases, key=lambda c: bool(PC.level0_depths(O, c))):      # the case that replaces a depth plane goes last
        for slot, dep in PC.level0_depths(O, case).items():
            ctx.upload_frames(slot, PC.frames_of(geom)[slot][None], dep[None])
            ctx.build_pyramids(slot, 1)
            ctx.apply_gradient(slot, 1)
        frames, t = PC.candidate_inputs(O, case)
        want = [PR.candidate_points(mag, dep, t, grid, case.lvl, case.n) for mag, dep, grid in frames]
        got, cnt = ctx.obtain_candidate_points_batch(case.first, case.n, case.lvl, t)
        print(case.name, "t = %r" % t, "counts", [int(c) for c in cnt], "want", [n for _, n in want])
        for f in range(case.n):
            assert int(cnt[f]) == want[f][1] and same_rows(got[f], want[f][0]), (case.name, f)
        if case.n == 1:
            rows, n = ctx.obtain_candidate_points(case.first, case.lvl, t)
            assert n == want[0][1] and same_rows(rows, want[0][0]), case.name
        full = max(n for _, n in want)
        for cap in sorted({0, 1, full // 2, full, full + 5}):                    # below, at and above the full count
            got, cnt2 = ctx.obtain_candidate_points_batch(case.first, case.n, case.lvl, t, cap=cap)
            assert np.array_equal(cnt2, cnt), (case.name, cap)
            for f in range(case.n):
                assert same_rows(got[f], want[f][0][:cap]), (case.name, cap, f)
    ctx.close()


@pytest.mark.one_arith
def test_non_finite_threshold_is_refused_by_every_entry(capi, O, torch):
    """NaN and the infinities: UWT_ERR_INVALID_ARG from the staged entries as from the batched tracking calls, nothing enqueued, and the
    context gives the restatement's rows afterwards; +-1e300 is finite and served"""
    geom = "g128x64"
    ctx = make_ctx(capi, geom, **dict(SCHEDULE, first_level=1))
    d_poses = torch.zeros((2, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for call in (lambda: ctx.obtain_candidate_points(0, 0, bad), lambda: ctx.obtain_candidate_points_batch(0, 2, 1, bad),
                     lambda: ctx.estimate_pose_candidates_batch([0], [1], threshold=bad),
                     lambda: ctx.estimate_pose_candidates_batch([0], [1], threshold=bad, weights=2, sampler=1),
                     lambda: ctx.estimate_pose_candidates_batch_seeded([0], [1], threshold=bad),
                     lambda: ctx.track_candidates_batch_async([0], [1], d_poses.data_ptr(), threshold=bad),
                     lambda: ctx.track_candidates_batch_seeded_async([0], [1], d_poses.data_ptr(), threshold=bad)):
            with pytest.raises(capi.UwtError) as e:
                call()
            assert e.value.status == INVALID_ARG
    ctx.sync()
    assert not d_poses.cpu().numpy().any()
    mag, dep, grid = PC.level_planes(O, geom, 0)[0]
    for t in (20.0, 1e300, -1e300):
        rows, n = ctx.obtain_candidate_points(0, 0, t)
        want, nw = PR.candidate_points(mag, dep, t, grid)
        assert n == nw and same_rows(rows, want)
    ctx.close()


def patch_want(kp, dep, cap=None):
    return PR.patch_points(kp, dep, W0, H0, cap)


@pytest.mark.one_arith
@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
def test_staged_patch_points(capi, O, depth):
    """uwt_obtain_patch_points on every key-point set (caps below, at and above the count) and uwt_obtain_patch_points_batch over all of
    them in one call, on slots whose depth planes differ; what is outside the key-point domain is refused and nothing is enqueued"""
    ctx = make_ctx(capi, "g64x48", max_pairs=16, depth=depth)
    deps = PC.depths_of("g64x48")
    for ps in PATCHES:
        want, n = patch_want(ps.kp, deps[0] if depth else None)
        rows, cnt = ctx.obtain_patch_points(0, ps.kp)
        print(ps.name, "count", cnt, "want", n)
        assert cnt == n and same_rows(rows, want), ps.name
        for cap in sorted({0, 1, max(n - 1, 0), n, n + 7}):
            rows, cnt = ctx.obtain_patch_points(0, ps.kp, cap=cap)
            assert cnt == n and same_rows(rows, want[:cap]), (ps.name, cap)
    slots = [(3 * i) % 10 for i in range(len(PATCHES))]                          # 0, 3, 6, 9, 2, ...: every kind of depth plane
    slots[[p.name for p in PATCHES].index("on_depths")] = 0
    got, cnt = ctx.obtain_patch_points_batch(slots, [p.kp for p in PATCHES])
    for f, ps in enumerate(PATCHES):
        want, n = patch_want(ps.kp, deps[slots[f]] if depth else None)
        assert int(cnt[f]) == n and same_rows(got[f], want), (ps.name, slots[f])
    capped, cnt2 = ctx.obtain_patch_points_batch(slots, [p.kp for p in PATCHES], cap=100)
    assert np.array_equal(cnt, cnt2) and all(same_rows(capped[f], got[f][:100]) for f in range(len(PATCHES)))
    for name, make in PC.REFUSED_KEYPOINTS.items():
        bad = np.array(make(W0, H0), np.float32)
        for call in (lambda: ctx.obtain_patch_points(0, bad), lambda: ctx.obtain_patch_points_batch([1, 0], [PATCHES[0].kp, bad]),
                     lambda: ctx.estimate_pose_features_batch([1, 0], [2, 3], [PATCHES[0].kp, bad])):
            with pytest.raises(capi.UwtError) as e:
                call()
            assert e.value.status == INVALID_ARG, name
    ps = PATCH_BY_NAME["edges"]                                                  # the context is usable afterwards
    want, n = patch_want(ps.kp, deps[0] if depth else None)
    rows, cnt = ctx.obtain_patch_points(0, ps.kp)
    assert cnt == n and same_rows(rows, want)
    ctx.close()


@pytest.mark.one_arith
def test_staged_add_patch_points(capi, O):
    """uwt_add_patch_points on levels 0 and 2 of 64 x 48: ties, borders, patch sizes 1, 3, 5, 11, 0 .. 600 points, caps inside the cloned
    part and inside the cells"""
    ctx = make_ctx(capi, "g64x48")
    for lvl in (0, 2):
        L = ctx.level_info(lvl)
        for tb in PC.table_sets(L.w, L.h):
            for ps in tb.patch_sizes:
                want, n = PR.add_patch_points(tb.pts, L.w, L.h, ps)
                rows, cnt = ctx.add_patch_points(lvl, tb.pts, patch_size=ps)
                print(lvl, tb.name, ps, "count", cnt, "want", n)
                assert cnt == n and same_rows(rows, want), (lvl, tb.name, ps)
                for cap in sorted({0, len(tb.pts) // 2, len(tb.pts), (len(tb.pts) + n) // 2, n, n + 3}):
                    rows, cnt = ctx.add_patch_points(lvl, tb.pts, patch_size=ps, cap=cap)
                    assert cnt == n and same_rows(rows, want[:cap]), (lvl, tb.name, ps, cap)
    ctx.close()


# ---- 2. the batched table calls ------------------------------------------------------------------------------------------------------------
# a small start: with a depth plane a candidate's z is byte * 0.0002 <= 0.051, and a larger translation would carry every point out
SEED = np.array([4e-5, -2e-5, 3e-5, 0.0, 3e-6, -2e-6, 1e-6], np.float32)
SEED[3] = np.sqrt(np.float32(1) - (SEED[:3] ** 2).sum(dtype=np.float32))
# (weights, sampler, seeded): plain, _opt (Huber, bilinear), _seeded — each as the synchronous and the _async entry
FORMS = {"plain": (None, None, False), "opt_huber_bilinear": (2, 1, False), "seeded": (None, None, True)}


def bits(poses, stats):
    return [(np.asarray(poses[i], np.float32).tobytes(), int(s["status"]), int(s["iterations"]), int(s["n_valid"]),
             int(np.float32(s["error"]).view(np.uint32))) for i, s in enumerate(stats)]


def device_bits(capi, torch, P, enqueue, ctx, seeds):
    """an _async entry into device buffers (seeds from device memory), as bits()"""
    d_poses = torch.zeros((P, 7), dtype=torch.float32, device="cuda")
    d_stats = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds)).cuda() if seeds is not None else None
    torch.cuda.synchronize()   # torch's fills and copies run on torch's stream, not on the context's
    enqueue(d_poses.data_ptr(), d_stats.data_ptr(), d_seeds.data_ptr() if seeds is not None else None)
    ctx.sync()
    st = d_stats.cpu().numpy().view(np.uint32)
    return [(d_poses.cpu().numpy()[i].tobytes(), int(st[i, 0]), int(st[i, 1]), int(st[i, 2]), int(st[i, 3])) for i in range(P)]


def check_pairs(got, want, what):
    """where the reference succeeds, the pose and every field of uwt_stats; where it runs out of valid points, the status, the unchanged
    pose, the evaluations and n_valid = 0"""
    for i, (g, (st, pose, tr)) in enumerate(zip(got, want)):
        assert g[1] == st, (what, i, g[1:], st)
        if st == OK:
            assert g == (pose.tobytes(),) + SR.stats_of(st, tr), (what, i, g[1:], SR.stats_of(st, tr))
        else:   # the pose in front of the evaluation that found no valid point, `iterations` counting it, n_valid = 0
            assert g[:4] == (pose.tobytes(), st, len(tr) + 1, 0), (what, i, g[1:], len(tr))


def lone_failure_depth(O, geom, slot, t):
    """the slot's depth plane with whole rows cleared: every cell level 2 selects at t reads a zero byte (rows 4y .. 4y + 3 of level 0 halve
    twice into row y of level 2), while most of the plane stays non-zero"""
    w, h = PC.GEOMS[geom][:2]
    mag2, _, grid2 = PC.level_planes(O, geom, slot)[2]
    sel, _ = PR.candidate_points(mag2, None, t, grid2)
    by = np.ascontiguousarray(PC.depths_of(geom)[slot]).view(np.uint8).reshape(h, 2 * w).copy()
    for y in sorted(set(sel[:, 1].astype(int))):
        by[4 * y:4 * y + 4, :] = 0
    return np.ascontiguousarray(by).view("<u2").reshape(h, w).astype(np.uint16)


def candidate_wants(O, geom, pairs, form, kind):
    """(threshold, the reference's (status, pose, trace) per pair, {slot: replaced depth plane}) of one batched candidates call.  With a
    depth plane and kind `eq`, the last pair's reference gets lone_failure_depth: it fails alone."""
    weights, sampler, seeded = FORMS[form]
    w, h, nl, slots, has = PC.GEOMS[geom]
    frames, deps = PC.frames_of(geom), PC.depths_of(geom)
    p = PC.oracle_params(O, geom, weights=weights or 0, sampler=sampler or 0, **SCHEDULE)
    t = PC.threshold_of(O, PC.Cand("pivot", geom, 0, pairs[0][0], 1, pairs[0][0], kind, ()))
    replaced = {pairs[-1][0]: lone_failure_depth(O, geom, pairs[-1][0], t)} if has and kind == "eq" else {}
    want = []
    for r, s in pairs:
        dp = replaced.get(r, deps[r]) if has else None
        dl = O.pyramid(dp, nl) if has else [None] * nl
        tables = {}
        for l in range(SCHEDULE["first_level"] + 1):
            mag, _, grid = PC.level_planes(O, geom, r)[l]
            tables[l] = PR.candidate_points(mag, dl[l], t, grid, l)[0]
        want.append(SR.align(O, p, frames[r], frames[s], dp, seed=SEED if seeded else None, tables=tables))
    return t, want, replaced


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geom,pairs", [("g64x48", [(2, 3), (5, 4), (3, 2), (1, 6)]), ("g46x35", [(0, 1), (1, 0)])], ids=["g64x48", "g46x35"])
def test_batched_candidate_calls(capi, torch, O, arith, geom, pairs, form):
    """uwt_estimate_pose_candidates_batch / uwt_track_candidates_batch_async, their _opt and _seeded forms, at the `eq` and the `below`
    threshold of pair 0's reference frame: a cell with magnitude == fl(mean + t) gained or lost changes n_valid and the pose.  On 64 x 48
    the last pair fails alone at `eq`: its reference's depth plane reads a zero byte under every cell level 2 selects."""
    weights, sampler, seeded = FORMS[form]
    frames, deps = PC.frames_of(geom), PC.depths_of(geom)
    ref, tgt = [r for r, _ in pairs], [t for _, t in pairs]
    P = len(pairs)
    seeds = np.tile(SEED, (P, 1)) if seeded else None
    ctx = make_ctx(capi, geom, **SCHEDULE)
    n_valid = {}
    for kind in ("eq", "below"):
        t, want, replaced = candidate_wants(O, geom, pairs, form, kind)
        for slot, dep in replaced.items():
            ctx.upload_frames(slot, frames[slot][None], dep[None])
            ctx.build_pyramids(slot, 1)
            ctx.apply_gradient(slot, 1)
        assert [wt[0] for wt in want] == [OK] * (P - 1) + [NO_VALID_POINTS if replaced else OK]
        n_valid[kind] = want[0][2][-1]["n_valid"]
        if seeded:
            got = bits(*ctx.estimate_pose_candidates_batch_seeded(ref, tgt, seeds, 0, threshold=t, weights=weights, sampler=sampler))
            dev = device_bits(capi, torch, P, lambda dp_, ds_, dz_: ctx.track_candidates_batch_seeded_async(
                ref, tgt, dp_, ds_, dz_, 0, threshold=t, weights=weights, sampler=sampler), ctx, seeds)
        else:
            got = bits(*ctx.estimate_pose_candidates_batch(ref, tgt, threshold=t, weights=weights, sampler=sampler))
            dev = device_bits(capi, torch, P, lambda dp_, ds_, dz_: ctx.track_candidates_batch_async(
                ref, tgt, dp_, ds_, threshold=t, weights=weights, sampler=sampler), ctx, None)
        print(geom, form, kind, "t = %r" % t, [g[1:4] for g in got], [SR.stats_of(wt[0], wt[2])[:3] for wt in want])
        check_pairs(got, want, (kind, "sync"))
        check_pairs(dev, want, (kind, "async"))
        for slot in replaced:   # the plane goes back for the other threshold
            ctx.upload_frames(slot, frames[slot][None], deps[slot][None])
            ctx.build_pyramids(slot, 1)
            ctx.apply_gradient(slot, 1)
    assert n_valid["below"] > n_valid["eq"]       # the cells holding the magnitude itself
    ctx.close()


def feature_pairs():
    """one pair per key-point set: reference slots over every kind of depth plane, `on_depths` on slot 0, the target the next slot"""
    ref = [(3 * i) % 10 for i in range(len(PATCHES))]
    ref[[p_.name for p_ in PATCHES].index("on_depths")] = 0
    return ref, [(r + 1) % 10 for r in ref], [p_.kp for p_ in PATCHES]


def feature_wants(O, depth, form):
    weights, sampler, seeded = FORMS[form]
    geom = "g64x48"
    frames, deps = PC.frames_of(geom), PC.depths_of(geom)
    ref, tgt, kps = feature_pairs()
    p = PC.oracle_params(O, geom, weights=weights or 0, sampler=sampler or 0, **FEATURES)
    p.has_depth = int(depth)
    want = []
    for i in range(len(ref)):
        dp = deps[ref[i]] if depth else None
        pts, _ = PR.patch_points(kps[i], dp, W0, H0)
        want.append(SR.align(O, p, frames[ref[i]], frames[tgt[i]], dp, seed=SEED if seeded else None, tables={0: pts}))
    return want


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
def test_batched_feature_calls(capi, torch, O, arith, depth, form):
    """uwt_estimate_pose_features_batch / uwt_track_features_batch_async, their _opt and _seeded forms, one pair per key-point set: patches
    over every border, key points on the five depths, 199 / 200 / 201 / 256 key points, none (the pair fails alone)"""
    weights, sampler, seeded = FORMS[form]
    ref, tgt, kps = feature_pairs()
    P = len(ref)
    seeds = np.tile(SEED, (P, 1)) if seeded else None
    want = feature_wants(O, depth, form)
    assert want[[p_.name for p_ in PATCHES].index("none")][0] == NO_VALID_POINTS and sum(wt[0] == OK for wt in want) >= P - 3
    ctx = make_ctx(capi, "g64x48", max_pairs=16, depth=depth)
    if seeded:
        got = bits(*ctx.estimate_pose_features_batch_seeded(ref, tgt, kps, seeds, 0, weights=weights, sampler=sampler))
        dev = device_bits(capi, torch, P, lambda dp_, ds_, dz_: ctx.track_features_batch_seeded_async(
            ref, tgt, kps, dp_, ds_, dz_, 0, weights=weights, sampler=sampler), ctx, seeds)
    else:
        got = bits(*ctx.estimate_pose_features_batch(ref, tgt, kps, weights=weights, sampler=sampler))
        dev = device_bits(capi, torch, P, lambda dp_, ds_, dz_: ctx.track_features_batch_async(
            ref, tgt, kps, dp_, ds_, weights=weights, sampler=sampler), ctx, None)
    print(form, depth, [g[1:4] for g in got], [SR.stats_of(wt[0], wt[2])[:3] for wt in want])
    check_pairs(got, want, "sync")
    check_pairs(dev, want, "async")
    ctx.close()


# ---- 3. the cloud and the sweep over the candidate selection ---------------------------------------------------------------------------------
def cloud_poses(n):
    out = []
    for f in range(n):
        a = np.deg2rad(3.0 + 2.0 * f)
        out.append([0.1 * np.sin(a / 2), -0.2 * np.sin(a / 2), np.sqrt(0.95) * np.sin(a / 2), np.cos(a / 2), 0.3 * f - 0.2, 0.05 * f, -0.1 * f + 0.4])
    return np.array(out, np.float32)


@pytest.mark.parametrize("geom,slots", [("g64x48", [4, 1, 3, 2]), ("g46x35", [1, 0]), ("g128x64", [0, 1])], ids=["g64x48", "g46x35", "g128x64"])
def test_cloud_from_candidates(capi, O, arith, geom, slots):
    """uwt_point_cloud_batch with source = 1 at the three equality thresholds of the first frame and at the one that selects every cell:
    the cloud's rows are the restatement's selection, record for record"""
    w, h, nl, _, has = PC.GEOMS[geom]
    frames = PC.frames_of(geom)
    ctx = make_ctx(capi, geom)
    L = O.level_intrinsics(PC.oracle_params(O, geom), 0)
    traj = cloud_poses(len(slots))
    for kind in ("eq", "below", "above", "all"):
        t = PC.threshold_of(O, PC.Cand("pivot", geom, 0, slots[0], 1, slots[0], kind, ()))
        tabs = [PR.candidate_points(*PC.level_planes(O, geom, s)[0][:2], t, PC.level_planes(O, geom, s)[0][2])[0] for s in slots]
        for mode, stride, skip in ((1, 1, 0), (0, 3, 1)):
            pts, info, call = CR.batch_cloud(O, [(tabs[f], traj[f], frames[s]) for f, s in enumerate(slots)], L, arith, mode, stride, skip)
            r = ctx.point_cloud_batch(slots, traj, capi.default_cloud_params(mode=mode, stride=stride, skip_invalid=skip, source=1, threshold=t))
            print(geom, kind, mode, stride, "rows", [int(i["n_rows"]) for i in r["info"]], "want", [len(tb) for tb in tabs])
            assert r["status"] == OK
            assert [tuple(int(i[k]) for k in CR.INFO_FIELDS) for i in r["info"]] == info
            assert tuple(int(r["call"][k]) for k in CR.INFO_FIELDS) == call
            assert r["points"].tobytes() == pts[:call[5]].tobytes()
        if kind == "all" and not has:
            assert [len(tb) for tb in tabs] == [w * h] * len(slots)
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("geom,lvl", [("g128x64", 0), ("g46x35", 0), ("g46x35", 1), ("g46x35", 2), ("g272x24", 0)])
def test_sweep_selects_the_complement_of_not_selected(capi, O, geom, lvl):
    """uwt_sweep_depth_batch with source = 1 at the equality thresholds: the pixels whose outcome is 0 (not selected) are exactly those the
    restatement does not select — image columns and rows beyond the point grid included — and n_selected is its count"""
    w, h, nl, slots, _ = PC.GEOMS[geom]
    ctx = make_ctx(capi, geom, depth=False)
    mag, _, grid = PC.level_planes(O, geom, 0)[lvl]
    codes = capi.sweep_hypotheses(0.6, 3.0, ctx.params.depth_scale, 17)
    pose = np.array([[0, 0, 0, 1, 0.05, 0.0, 0.0]], np.float32)
    for kind in ("eq", "below", "above", "all", "none"):
        t = PC.threshold_of(O, PC.Cand("pivot", geom, lvl, 0, 1, 0, kind, ()))
        rows, n = PR.candidate_points(mag, None, t, grid)
        sel = np.zeros(mag.shape, bool)
        sel[rows[:, 1].astype(int), rows[:, 0].astype(int)] = True
        r = ctx.sweep_depth([0], [[1]], pose, codes, capi.default_sweep_params(lvl=lvl, source=1, threshold=t, n_views=1, n_hyp=len(codes)))
        print(geom, lvl, kind, "selected", int(r["info"][0]["n_selected"]), "want", n)
        assert r["status"] == OK and int(r["info"][0]["status"]) == OK
        assert np.array_equal(r["outcome"][0] != 0, sel) and int(r["info"][0]["n_selected"]) == n
        assert not r["depth"][0][~sel].any()
    ctx.close()


# ---- 4. guard bands: the full table and 256 key points ---------------------------------------------------------------------------------------
def frozen(x):
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    return x


def same_with_guards(ctx, run):
    """run() with guard gaps between the arrays of the context's scratch off, then on: no gap damaged, every output the same"""
    ctx.debug_guards(0)
    off = frozen(run())
    ctx.debug_guards(GUARD)
    on = frozen(run())
    damaged, where = ctx.debug_check_guards()
    ctx.debug_guards(0)
    assert damaged == 0, where
    assert on == off


@pytest.mark.one_arith
@pytest.mark.parametrize("name", ["g128x64_l0_all", "g46x35_l2_all", "g46x35_l1_all", "g40x90_l0_all", "g272x24_l0_all", "g163x99_l1_all_n3"])
def test_guards_around_the_full_candidate_table(capi, O, name):
    """every cell selected: each frame's table holds exactly gw * gh rows, its last row the last of its room ("the bound is never reached")
    — nothing is written past it, into the next frame's table or the gap behind the last"""
    case = PC.CAND_BY_NAME[name]
    ctx = make_ctx(capi, case.geom, depth=False)
    t = PC.threshold_of(O, case)
    L = ctx.level_info(case.lvl)
    same_with_guards(ctx, lambda: ctx.obtain_candidate_points_batch(case.first, case.n, case.lvl, t))
    got, cnt = ctx.obtain_candidate_points_batch(case.first, case.n, case.lvl, t)
    assert [int(c) for c in cnt] == [L.w * L.h] * case.n
    for f in range(case.n):
        mag, _, grid = PC.level_planes(O, case.geom, case.first + f)[case.lvl]
        assert same_rows(got[f], PR.candidate_points(mag, None, t, grid)[0])
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
def test_guards_around_256_key_points(capi, torch, O, depth):
    """256 key points of which 200 are used: the staged entries under scratch guards, and the live call's poses and stats in a guarded
    arena of caller memory, equal to the synchronous entry's"""
    ctx = make_ctx(capi, "g64x48", max_pairs=8, depth=depth)
    kp = PATCH_BY_NAME["n256"].kp
    same_with_guards(ctx, lambda: ctx.obtain_patch_points(0, kp))
    same_with_guards(ctx, lambda: ctx.obtain_patch_points_batch([0, 3, 2], [kp, kp[::-1].copy(), PATCH_BY_NAME["edges"].kp]))
    ref, tgt, kps = [0, 3, 2], [1, 2, 3], [kp, kp[::-1].copy(), PATCH_BY_NAME["edges"].kp]
    want, wst = ctx.estimate_pose_features_batch(ref, tgt, kps)
    specs = [GB.Buf("poses", nbytes=3 * 28, align=4, stride=28), GB.Buf("stats", nbytes=3 * 16, align=4, stride=16)]
    outs = GB.run_twice(GB.TorchBackend(torch), specs, lambda a: (ctx.track_features_batch_async(ref, tgt, kps, a.ptr("poses"), a.ptr("stats")), ctx.sync()))
    st = np.zeros(3, capi.STATS)
    for i, s in enumerate(wst):
        for k in ("status", "iterations", "n_valid", "error"):
            st[i][k] = s[k]
    assert outs["poses"] == want[:3].tobytes() and outs["stats"] == st.tobytes() and all(s["status"] == OK for s in wst)
    ctx.close()


@pytest.mark.one_arith
def test_guards_around_the_candidates_call_with_full_tables(capi, torch, O):
    """the batched candidates call at a threshold that selects every cell of every iterated level (46 x 35, levels 2 .. 0: grids below
    their images), poses and stats in a guarded arena, equal to the synchronous entry's; the context's scratch under guards as well"""
    geom = "g46x35"
    ctx = make_ctx(capi, geom, **SCHEDULE)
    ref, tgt = [0, 1, 0], [1, 0, 0]
    want, wst = ctx.estimate_pose_candidates_batch(ref, tgt, threshold=-300.0)
    assert all(s["status"] == OK and s["n_valid"] > 0 for s in wst)
    for l in range(SCHEDULE["first_level"] + 1):   # every iterated level's table is full: one row per cell of its grid
        L = ctx.level_info(l)
        assert [int(c) for c in ctx.obtain_candidate_points_batch(0, 2, l, -300.0)[1]] == [L.w * L.h] * 2
    frames = PC.frames_of(geom)
    p = PC.oracle_params(O, geom, **SCHEDULE)
    for i in range(3):
        tables = {l: PR.candidate_points(*PC.level_planes(O, geom, ref[i])[l][:2], -300.0, PC.level_planes(O, geom, ref[i])[l][2])[0]
                  for l in range(SCHEDULE["first_level"] + 1)}
        st, pose, tr = SR.align(O, p, frames[ref[i]], frames[tgt[i]], None, tables=tables)
        assert (want[i].tobytes(), wst[i]["status"], wst[i]["iterations"], wst[i]["n_valid"]) == (pose.tobytes(),) + SR.stats_of(st, tr)[:3]
    same_with_guards(ctx, lambda: ctx.estimate_pose_candidates_batch(ref, tgt, threshold=-300.0))
    specs = [GB.Buf("poses", nbytes=3 * 28, align=4, stride=28), GB.Buf("stats", nbytes=3 * 16, align=4, stride=16)]
    outs = GB.run_twice(GB.TorchBackend(torch), specs, lambda a: (ctx.track_candidates_batch_async(ref, tgt, a.ptr("poses"), a.ptr("stats"), threshold=-300.0),
                                                                   ctx.sync()))
    st = np.zeros(3, capi.STATS)
    for i, s in enumerate(wst):
        for k in ("status", "iterations", "n_valid", "error"):
            st[i][k] = s[k]
    assert outs["poses"] == want[:3].tobytes() and outs["stats"] == st.tobytes()
    ctx.close()
