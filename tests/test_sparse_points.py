"""explicit point tables (candidatePoints_) and their producers
(ObtainPatchesPoints, ObtainCandidatePoints), CPU oracle checks + GPU parity."""
import importlib

import numpy as np
import pytest

MID = (131.25, 131.25, 79.5, 47.5)
FEATURES = dict(n_levels=5, first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002,
                handoff_scale_t=1)   # EstimatePoseFeatures locals, src/Tracker.cpp:634-640, 834, 856


def test_oracle_patch_points_semantics(O):
    w, h = 64, 48
    kp = np.array([[20.0, 20.0], [2.5, 3.0], [62.9, 46.2], [30.7, 10.2]], np.float32)
    pts, n = O.patch_points(kp, None, w, h)
    exp = []
    for x, y in kp:
        i = int(np.float32(x) - np.float32(5))
        while np.float32(i) <= np.float32(x) + np.float32(5):
            j = int(np.float32(y) - np.float32(5))
            while np.float32(j) <= np.float32(y) + np.float32(5):
                if 0 < i < w and 0 < j < h:
                    exp.append([i, j, 1, 1])
                j += 1
            i += 1
    assert n == len(exp) and np.array_equal(pts, np.array(exp, np.float32))
    assert (pts[:121, 0] == np.repeat(np.arange(15, 26), 11)).all()       # 11x11, x-major (src/Tracker.cpp:1204-1206)
    dep = np.zeros((h, w), np.uint16)
    dep[20, 20] = 5000
    dep[10, 30] = 40000                                                    # negative as short, still != 0
    pts, n = O.patch_points(kp, dep, w, h)
    assert n == 121 + 121 and pts[0, 2] == np.float32(5000) * np.float32(0.0002) * np.float32(1.0)
    assert pts[121, 2] == np.float32(np.int16(40000 - 65536)) * np.float32(0.0002)
    many = np.tile(np.array([[20.0, 20.0]], np.float32), (250, 1))
    assert O.patch_points(many, None, w, h)[1] == 200 * 121               # min(num_max_keypoints, 200)


def test_oracle_candidate_points_semantics(O, synth):
    img = synth.texture(64, 48, seed=4)
    gx, gy = O.scharr3(img)
    mag = O.gradient_mag(gx, gy)
    pts, n = O.candidate_points(mag, None, 20.0)
    thres = mag.astype(np.float64).mean() + 20.0
    ys, xs = np.nonzero(mag.T > thres)  # transposed => x-major order
    assert n == len(xs) and np.array_equal(pts[:, 0], ys) and np.array_equal(pts[:, 1], xs)
    assert (pts[:, 2] == 1).all() and (pts[:, 3] == 1).all() and 0 < n < mag.size
    dep = np.full((48, 64), 0x0100, np.uint16)  # bytes: 00 01 00 01 ... => at<uchar>(y, x) is zero for even x
    ptsd, nd = O.candidate_points(mag, dep, 20.0)
    assert nd > 0 and (ptsd[:, 0] % 2 == 1).all() and (ptsd[:, 2] == np.float32(1) * np.float32(0.0002)).all()


def test_oracle_dense_table_equals_dense_path(O, synth):
    w, h = 160, 96
    ref, tgt, _, _, _ = synth.render_pair(w, h, *MID, seed=61)
    p = O.default_params(w, h, *MID)
    st0, pose0, tr0 = O.align_pair(p, ref, tgt, want_trace=True)
    tables = {l: O.dense_points(None, w >> l, h >> l, l) for l in range(1, 5)}
    st1, pose1, tr1 = O.align_pair_points(p, ref, tgt, tables, want_trace=True)
    assert st0 == st1 == 0 and np.array_equal(pose0, pose1) and len(tr0) == len(tr1)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def test_oracle_drops_table_rows_outside_the_level(O, synth):
    """The oracle's own definition of the undefined case: a row whose reference position is outside the level (the reference's
    Mat::at would read outside the image, src/Tracker.cpp:474-477) is dropped — a table with such rows aligns like the table
    without them, and a table of nothing else has no valid point."""
    w, h = 160, 96
    ref, tgt, _, _, _ = synth.render_pair(w, h, *MID, seed=66, z=1.1)
    p = O.default_params(w, h, *MID, n_levels=4, first_level=0, last_level=0, max_iters=4, early_exit=0)
    rng = np.random.default_rng(12)
    inside = np.empty((2000, 4), np.float32)
    inside[:, 0] = rng.uniform(0, w - 0.01, 2000); inside[:, 1] = rng.uniform(0, h - 0.01, 2000); inside[:, 2:] = 1.0
    outside = np.array([[-1.5, 4, 1, 1], [w, 4, 1, 1], [5, -1.0, 1, 1], [5, h, 1, 1], [-2, h + 9, 1, 1]], np.float32)
    s0, p0, t0 = O.align_pair_points(p, ref, tgt, {0: inside}, want_trace=True)
    s1, p1, t1 = O.align_pair_points(p, ref, tgt, {0: np.concatenate([outside, inside])}, want_trace=True)
    assert s0 == 0 and s1 == 0 and np.array_equal(p0, p1) and [q["n_valid"] for q in t0] == [q["n_valid"] for q in t1]
    assert O.align_pair_points(p, ref, tgt, {0: outside})[0] != 0


def _ctx_pair(capi, synth, w, h, seed, depth=False, **over):
    ref, tgt, dep, _, _ = synth.render_pair(w, h, *MID, seed=seed, with_depth=depth, z=1.1)
    if depth:
        over["has_depth"] = 1
    ctx = capi.Context(capi.default_params(w, h, *MID, max_frames=2, max_pairs=1, **over))
    ctx.upload_frames(0, np.stack([ref, tgt]), np.stack([dep, dep]) if depth else None)
    ctx.build_pyramids(0, 2)
    ctx.apply_gradient(0, 2)
    return ctx, ref, tgt, dep


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_producers_bit_exact(capi, O, synth, depth):
    w, h = 160, 96
    ctx, ref, tgt, dep = _ctx_pair(capi, synth, w, h, 62, depth)
    tdep = None
    if depth:   # the target frame gets a depth plane of its own (holes elsewhere): a wrong slot offset shows
        tdep = np.roll(dep, (3, 5), axis=(0, 1))
        ctx.upload_frames(1, tgt[None], tdep[None])
        ctx.build_pyramids(1, 1)
        ctx.apply_gradient(1, 1)
    rng = np.random.default_rng(5)
    kp = np.concatenate([rng.uniform(0, [w - 0.01, h - 0.01], (230, 2)),
                         [[0, 0], [w - 1, h - 1], [4.5, 4.5], [5, 5], [w - 5.5, h - 5.5]]]).astype(np.float32)
    for slot, img, dp in ((0, ref, dep), (1, tgt, tdep)):
        dp0 = dp
        for lvl in range(5):
            if lvl:
                img = O.halve_u8(img)
                dp = O.halve_u16(dp) if depth else None
            gx, gy = O.scharr3(img)
            mag = O.gradient_mag(gx, gy)
            assert np.array_equal(ctx.gradient_magnitude(slot, lvl), mag)
            for thr in (20.0, 0.0, 300.0):
                a, na = ctx.obtain_candidate_points(slot, lvl, thr)
                b, nb = O.candidate_points(mag, dp, thr)
                assert na == nb and np.array_equal(a, b)
        for k in (kp, kp[:7], kp[:0]):
            a, na = ctx.obtain_patch_points(slot, k)
            b, nb = O.patch_points(k, dp0, w, h)
            assert na == nb and np.array_equal(a, b)
        b, nb = O.patch_points(kp, dp0, w, h)
        a, na = ctx.obtain_patch_points(slot, kp, cap=10)
        assert a.shape == (10, 4) and na == nb and np.array_equal(a, b[:10])
    full, nfull = ctx.obtain_candidate_points(0, 0, 20.0)
    a, na = ctx.obtain_candidate_points(0, 0, 20.0, cap=10)
    assert a.shape == (10, 4) and na == nfull > 10 and np.array_equal(a, full[:10])
    with pytest.raises(capi.UwtError):
        ctx.obtain_patch_points(0, np.array([[w + 1.0, 2.0]], np.float32))


@pytest.mark.gpu
def test_gpu_point_table_alignment_matches_dense_and_oracle(capi, O, synth):
    w, h = 160, 96
    ctx, ref, tgt, _ = _ctx_pair(capi, synth, w, h, 63)
    dense, _ = ctx.estimate_pose_batch([0], [1], raise_on_pair_failure=True)
    tables = {l: O.dense_points(None, w >> l, h >> l, l) for l in range(1, 5)}
    pose, st = ctx.estimate_pose_points(0, 1, tables)
    assert st["status"] == 0 and np.array_equal(pose, dense[0])
    # semi-dense tables from ObtainCandidatePoints on every level, reference schedule
    cand = {l: ctx.obtain_candidate_points(0, l, 20.0)[0] for l in range(1, 5)}
    pose, st = ctx.estimate_pose_points(0, 1, cand)
    p = O.default_params(w, h, *MID)
    so, pose_cpu, tr = O.align_pair_points(p, ref, tgt, cand, want_trace=True)
    assert so == 0 and st["status"] == 0 and st["iterations"] == len(tr)
    assert np.array_equal(pose, pose_cpu)
    # empty table ⇒ no valid points
    empty = dict(cand)
    empty[4] = np.zeros((0, 4), np.float32)
    pose, st = ctx.estimate_pose_points(0, 1, empty)
    assert st["status"] == capi.ERR_NO_VALID_POINTS


@pytest.mark.gpu
@pytest.mark.parametrize("weights,sampler", [(1, 0), (2, 0), (0, 1), (2, 1)])
def test_gpu_point_tables_on_the_general_path(capi, O, synth, weights, sampler):
    """uwt_params::weights / ::sampler apply to explicit tables as to the dense call (k_table_hist, k_table_general, the call a
    batch of one pair): candidate tables on three levels and a 20 000-row table of arbitrary rows, poses bit-identical."""
    w, h = 160, 96
    over = dict(n_levels=4, first_level=2, last_level=0, max_iters=6, early_exit=0, weights=weights, sampler=sampler)
    ctx, ref, tgt, _ = _ctx_pair(capi, synth, w, h, 65, **over)
    p = O.default_params(w, h, *MID, **over)
    rng = np.random.default_rng(11)
    for factors in ({}, dict(z_factor=0.5, angle_factor=1.5)):
        if factors:
            ctx.update_params(**factors)
            for k, v in factors.items():
                setattr(p, k, v)
        cand = {l: ctx.obtain_candidate_points(0, l, 20.0)[0] for l in range(3)}
        rows = np.empty((20000, 4), np.float32)
        rows[:, 0] = rng.uniform(-3, w + 3, 20000); rows[:, 1] = rng.uniform(-3, h + 3, 20000)
        rows[:, 2] = rng.choice([0.0, -0.5, 0.4, 1.0, 2.0], 20000); rows[:, 3] = rng.choice([1.0, 0.0, 0.5], 20000, p=[0.9, 0.05, 0.05])
        for tables in (cand, {0: rows, 1: cand[1], 2: cand[2]}):
            pose, st = ctx.estimate_pose_points(0, 1, tables)
            so, pose_cpu, tr = O.align_pair_points(p, ref, tgt, tables, want_trace=True)
            assert so == 0 and st["status"] == 0 and st["iterations"] == len(tr)
            assert np.array_equal(pose, pose_cpu), (weights, sampler, factors)


@pytest.mark.gpu
def test_gpu_point_table_rows_outside_the_level_are_dropped(capi, O, synth):
    """A row whose reference position ((int)y, (int)x) is outside the level: the reference's Mat::at would read outside the
    image (src/Tracker.cpp:474-477); both sides drop the row.  The table with such rows aligns like the table without them."""
    w, h = 160, 96
    over = dict(n_levels=4, first_level=0, last_level=0, max_iters=5, early_exit=0)
    ctx, ref, tgt, _ = _ctx_pair(capi, synth, w, h, 66, **over)
    p = O.default_params(w, h, *MID, **over)
    rng = np.random.default_rng(12)
    inside = np.empty((3000, 4), np.float32)
    inside[:, 0] = rng.uniform(0, w - 0.01, 3000); inside[:, 1] = rng.uniform(0, h - 0.01, 3000); inside[:, 2] = 1.0; inside[:, 3] = 1.0
    outside = np.array([[-1.5, 4, 1, 1], [w, 4, 1, 1], [w + 2.5, 4, 1, 1], [5, -1.0, 1, 1], [5, h, 1, 1], [5, h + 7, 1, 1], [-2, -2, 1, 1]], np.float32)
    mixed = np.concatenate([inside[:1000], outside, inside[1000:]])
    a, sa = ctx.estimate_pose_points(0, 1, {0: inside})
    b, sb = ctx.estimate_pose_points(0, 1, {0: mixed})
    so, pose_cpu, tr = O.align_pair_points(p, ref, tgt, {0: mixed}, want_trace=True)
    assert sa["status"] == 0 and sb["status"] == 0 and so == 0
    assert np.array_equal(a, b) and np.array_equal(b, pose_cpu) and sb["n_valid"] == tr[-1]["n_valid"]
    only_out, s_out = ctx.estimate_pose_points(0, 1, {0: outside})
    assert s_out["status"] == capi.ERR_NO_VALID_POINTS and O.align_pair_points(p, ref, tgt, {0: outside})[0] == s_out["status"]


def _rows_inside(rng, n, w, h):
    rows = np.ones((n, 4), np.float32)
    rows[:, 0] = rng.uniform(0, w - 0.01, n)
    rows[:, 1] = rng.uniform(0, h - 0.01, n)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [{}, dict(weights=2), dict(sampler=1)], ids=["identity", "huber", "bilinear"])
def test_gpu_point_table_slice_boundaries(capi, O, synth, mode):
    """Row counts around the 1024 rows of a block of k_table_eval / k_table_hist / k_table_general: none, one, a partial block,
    exactly one block, one row into the next, across 8192, and more slices than the context's own record pool holds (20 000
    rows, max_pairs = 1).  Status as the oracle's; pose, evaluations and valid rows bit for bit where it succeeds."""
    w, h = 160, 96
    over = dict(n_levels=4, first_level=0, last_level=0, max_iters=5, early_exit=0, **mode)
    ref, tgt, _, _, _ = synth.render_pair(w, h, *MID, seed=67)
    ctx = capi.Context(capi.default_params(w, h, *MID, max_frames=2, max_pairs=1, **over))
    ctx.upload_frames(0, np.stack([ref, tgt]))
    ctx.build_pyramids(0, 2)
    ctx.apply_gradient(0, 2)
    p = O.default_params(w, h, *MID, **over)
    rng = np.random.default_rng(13)
    for n in (0, 1, 6, 255, 1023, 1024, 1025, 2048, 8192, 8193, 20000):
        rows = _rows_inside(rng, n, w, h)
        pose, st = ctx.estimate_pose_points(0, 1, {0: rows})
        so, pose_cpu, tr = O.align_pair_points(p, ref, tgt, {0: rows}, want_trace=True)
        assert st["status"] == so, (n, st, so)
        if so == 0:
            assert np.array_equal(pose, pose_cpu), (n, pose, pose_cpu)
            assert st["iterations"] == len(tr) and st["n_valid"] == tr[-1]["n_valid"], (n, st, tr[-1])
    ctx.close()


@pytest.mark.gpu
def test_gpu_point_table_call_leaves_shared_state_clean(capi, O, synth):
    """The histogram rows and the tail tickets are zero again behind a table call: the dense batch that follows it gives what it
    gives on a context that never ran one."""
    w, h = 160, 96
    over = dict(n_levels=4, first_level=2, last_level=0, max_iters=6, early_exit=0, weights=2)
    frames = []
    for seed in (68, 69):
        ref, tgt, _, _, _ = synth.render_pair(w, h, *MID, seed=seed, z=1.1)
        frames += [ref, tgt]
    rng = np.random.default_rng(14)
    tables = {0: _rows_inside(rng, 20000, w, h), 1: _rows_inside(rng, 3000, w // 2, h // 2), 2: _rows_inside(rng, 700, w // 4, h // 4)}
    results = []
    for table_call in (True, False):
        ctx = capi.Context(capi.default_params(w, h, *MID, max_frames=4, max_pairs=2, **over))
        ctx.upload_frames(0, np.stack(frames))
        ctx.build_pyramids(0, 4)
        ctx.apply_gradient(0, 4)
        if table_call:
            assert ctx.estimate_pose_points(0, 1, tables)[1]["status"] == 0
        results.append(ctx.estimate_pose_batch([0, 2], [1, 3], raise_on_pair_failure=True))
        ctx.close()
    (poses_a, stats_a), (poses_b, stats_b) = results
    assert np.array_equal(poses_a, poses_b)
    assert [dict(s) for s in stats_a] == [dict(s) for s in stats_b]


@pytest.mark.gpu
def test_gpu_point_tables_of_different_sizes_per_level(capi, O, synth):
    """Two slices, then one, then an empty table, in the iteration order 2 -> 1 -> 0, out of a scratch sized by the largest: the
    empty level ends the call with the oracle's status."""
    w, h = 160, 96
    over = dict(n_levels=4, first_level=2, last_level=0, max_iters=5, early_exit=0)
    ctx, ref, tgt, _ = _ctx_pair(capi, synth, w, h, 67, **over)
    p = O.default_params(w, h, *MID, **over)
    rng = np.random.default_rng(15)
    tables = {2: _rows_inside(rng, 1500, w // 4, h // 4), 1: _rows_inside(rng, 1024, w // 2, h // 2), 0: np.zeros((0, 4), np.float32)}
    _, st = ctx.estimate_pose_points(0, 1, tables)
    so = O.align_pair_points(p, ref, tgt, tables)[0]
    assert st["status"] == capi.ERR_NO_VALID_POINTS and st["status"] == so
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_estimate_pose_features_flow(capi, O, synth, depth):
    """The reference's live sequence (src/System.cpp:193-223): key points -> ObtainPatchesPoints -> EstimatePoseFeatures."""
    w, h = 160, 96
    ctx, ref, tgt, dep = _ctx_pair(capi, synth, w, h, 64, depth, **FEATURES)
    rng = np.random.default_rng(9)
    kp = rng.uniform([6, 6], [w - 7, h - 7], (150, 2)).astype(np.float32)   # stand-in for the SURF key points
    pts, n = ctx.obtain_patch_points(0, kp)
    assert n == (O.patch_points(kp, dep if depth else None, w, h)[1]) and (depth or n == 150 * 121)  # duplicates allowed
    pose, st = ctx.estimate_pose_points(0, 1, {0: pts})
    p = O.default_params(w, h, *MID, **FEATURES)
    if depth:
        p.has_depth = 1
    pts_cpu, _ = O.patch_points(kp, dep if depth else None, w, h)
    so, pose_cpu, tr = O.align_pair_points(p, ref, tgt, {0: pts_cpu}, ref_depth=dep if depth else None, want_trace=True)
    assert so == 0 and st["status"] == 0 and st["iterations"] == len(tr) and 1 <= len(tr) <= 10
    assert np.array_equal(pose, pose_cpu)


@pytest.mark.gpu
def test_gpu_candidate_points_batch_of_frames_matches_oracle_per_frame(capi, O, synth):
    """uwt_obtain_candidate_points_batch: many frames, many blocks per frame, the reference's x-major order kept."""
    w, h, n = 320, 240, 9
    intr = (262.5, 262.5, 159.5, 119.5)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=n, max_pairs=1, has_depth=1))
    frames, depths = [], []
    for s_ in range(n):
        ref, _, dep, _, _ = synth.render_pair(w, h, *intr, seed=700 + s_, with_depth=True)
        frames.append(ref); depths.append(dep)
    ctx.upload_frames(0, np.stack(frames), np.stack(depths))
    ctx.build_pyramids(0, n)
    ctx.apply_gradient(0, n)
    for lvl, thr in ((0, 20.0), (2, 5.0), (4, 0.0)):
        got, cnt = ctx.obtain_candidate_points_batch(0, n, lvl, thr)
        for f in range(n):
            img, dp = frames[f], depths[f]
            for _ in range(lvl):
                img, dp = O.halve_u8(img), O.halve_u16(dp)
            mag = O.gradient_mag(*O.scharr3(img))
            want, nw = O.candidate_points(mag, dp, thr)
            assert cnt[f] == nw and np.array_equal(got[f], want), (lvl, f)
    capped, cnt = ctx.obtain_candidate_points_batch(2, 3, 0, 20.0, cap=50)      # a sub-range of slots, capped output
    full, cnt2 = ctx.obtain_candidate_points_batch(2, 3, 0, 20.0)
    assert np.array_equal(cnt, cnt2) and all(np.array_equal(capped[f], full[f][:50]) for f in range(3))
    ctx.close()


def test_oracle_add_patch_points_semantics(O):
    w, h = 40, 30
    pts = np.array([[3.4, 2.6, 0.7, 1.0], [0.2, 0.4, 1.5, 1.0], [39.2, 29.4, 0.9, 1.0], [20.5, 10.5, 1.1, 1.0]], np.float32)
    got, n = O.add_patch_points(pts, w, h)
    exp = [list(p) for p in pts]
    for x, y, z, _ in pts:
        x, y = np.float32(np.floor(x + 0.5)) if x >= 0 else x, np.float32(np.floor(y + 0.5)) if y >= 0 else y   # C round(), x, y >= 0
        for i in range(int(x) - 2, int(x) + 3):
            for j in range(int(y) - 2, int(y) + 3):
                if 0 < i < w and 0 < j < h and not (i == x and j == y):
                    exp.append([i, j, z, 1.0])
    assert n == len(exp) and np.array_equal(got, np.array(exp, np.float32))
    assert n == 4 + 24 + 4 + 8 + 24            # interior points: 24 cells; at (0, 0): the 2x2 cells with i, j > 0; at (39, 29): 3x3 - 1


@pytest.mark.gpu
def test_add_patch_points_matches_oracle_over_levels_sizes_and_caps(capi, O):
    """uwt_add_patch_points = Tracker::AddPatchPointsFeatures (src/Tracker.cpp:599-629): the table, then per point the patch
    cells inside the level except the centre, in the reference's push_back order; empty tables, borders, a cap smaller than
    the full count, more points than one chunk of the kernel, other patch sizes."""
    w, h = 160, 96
    ctx = capi.Context(capi.default_params(w, h, 131.25, 131.25, 79.5, 47.5, max_frames=2, max_pairs=1))
    rng = np.random.default_rng(77)
    for lvl in (0, 1, 3):
        L = ctx.level_info(lvl)
        for n in (0, 1, 7, 300, 1000):
            pts = np.column_stack([rng.uniform(-1, L.w + 1, n), rng.uniform(-1, L.h + 1, n), rng.uniform(0.5, 2.0, n), np.ones(n)]).astype(np.float32)
            for ps in (5, 3, 1):
                got, cnt = ctx.add_patch_points(lvl, pts, patch_size=ps)
                want, n_want = O.add_patch_points(pts, L.w, L.h, patch_size=ps)
                assert cnt == n_want and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lvl, n, ps)
        pts = np.array([[10.4, 10.6, 1.0, 1.0], [0.0, 0.0, 2.0, 1.0]], np.float32)
        got, cnt = ctx.add_patch_points(lvl, pts, cap=9)                 # full count reported, nine rows written
        want, n_want = O.add_patch_points(pts, L.w, L.h, cap=9)
        assert cnt == n_want > 9 and got.shape == (9, 4) and np.array_equal(got, want)
    ctx.close()
