"""The RGB-D point-cloud map on the device (uwt_point_cloud_batch*, uwt_point_cloud_points, uwt_accumulate_trajectory_device_async):
points, tags and records compared AS BYTES — no tolerance anywhere — with the numpy restatement of the contract (tests/cloud_ref.py
over oracle.dense_points, candidate_points and se3_matrix)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cloud_ref as CR

OK, INVALID_ARG, CAPACITY, PAIR_FAILED = 0, 1, 5, 6   # uwt_status_code (include/uwt.h)
# 40 x 30: pitch = width; 37 x 23: rows pitched to 40; 160 x 96: 15 360 rows, 60 blocks per frame of one turn (256 rows) each.  Blocks
# that take SEVERAL turns (the launch is capped at 2048 blocks): test_gpu_blocks_of_several_turns below
SIZES = [(40, 30), (37, 23), (160, 96)]
N_LEVELS = 3
THRESHOLD = 5.0
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
SLOTS = [0, 1, 2, 3, 0]   # slot 1: the all-zero depth frame, BETWEEN two non-empty ones; slot 0 again at batch position 4


def intr(w, h):
    return (0.82 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


_scenes = {}


def scene(synth, w, h):
    """Four frames and their depth images.  The depth is a sloping plane with explicit zero rectangles cut into it — a band of whole
    rows, a block in the right half, single pixels at the corners — so that, row selection or not, some selected rows are invalid and
    some are not BY CONSTRUCTION; frame 1's depth is all zero."""
    if (w, h) not in _scenes:
        a = synth.render_pair(w, h, *intr(w, h), seed=5)
        b = synth.render_pair(w, h, *intr(w, h), seed=6)
        frames = [a[0], a[1], b[0], b[1]]
        depths = []
        ys, xs = np.mgrid[0:h, 0:w]
        for k in range(4):
            d = (3000 + 17 * xs + 29 * ys + 100 * k).astype(np.uint16)   # a sloping plane, 0.6 m to 2 m: no zero of its own
            d[h // 3:h // 3 + 3, :] = 0                       # whole rows: every stride below 3 w meets it
            d[h // 2:, w // 2 + k:w // 2 + k + w // 4] = 0    # a block in the right half, shifted from frame to frame
            d[0, 0] = d[h - 1, w - 1] = 0
            depths.append(d)
        depths[1][:] = 0
        _scenes[(w, h)] = (frames, depths)
    return _scenes[(w, h)]


def poses_for(n):
    """distinct, finite, rotated poses (an accumulated trajectory has no special form)"""
    out = []
    for f in range(n):
        a = np.deg2rad(3.0 + 2.0 * f)
        out.append([0.1 * np.sin(a / 2), -0.2 * np.sin(a / 2), np.sqrt(0.95) * np.sin(a / 2), np.cos(a / 2), 0.3 * f - 0.2, 0.05 * f, -0.1 * f + 0.4])
    return np.array(out, np.float32)


def make_ctx(capi, synth, w, h, depth=True, max_frames=5, gradients=False):
    frames, depths = scene(synth, w, h)
    ctx = capi.Context(capi.default_params(w, h, *intr(w, h), max_frames=max_frames, max_pairs=4, n_levels=N_LEVELS, first_level=2,
                                           last_level=0, has_depth=int(depth)))
    ctx.upload_frames(0, np.stack(frames), np.stack(depths) if depth else None)
    ctx.build_pyramids(0, 4)
    if gradients:
        ctx.apply_gradient(0, 4)
    return ctx


def oracle_level(O, w, h, depth=True):
    p = O.default_params(w, h, *intr(w, h), n_levels=N_LEVELS, first_level=2, last_level=0, has_depth=int(depth))
    return p, O.level_intrinsics(p, 0)


def tables_of(O, synth, w, h, source, depth=True):
    """the level-0 table of each of the four slots, from the oracle"""
    frames, depths = scene(synth, w, h)
    p, L = oracle_level(O, w, h, depth)
    out = []
    for s in range(4):
        d = depths[s] if depth else None
        if source == 0:
            out.append(O.dense_points(d, w, h, 0, p.depth_scale))
        else:
            out.append(O.candidate_points(O.gradient_mag(*O.scharr3(frames[s])), d, THRESHOLD)[0])
    return out, L


def info_tuples(info):
    return [tuple(int(r[k]) for k in CR.INFO_FIELDS) for r in np.atleast_1d(info)]


def check(r, want):
    pts, info, call = want
    assert info_tuples(r["info"]) == info
    assert info_tuples(r["call"]) == [call]
    assert r["points"].tobytes() == pts[:call[5]].tobytes()


# ---- 1. the batch against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("source", [0, 1])
def test_gpu_batch_equals_reference(capi, synth, O, arith, w, h, source):
    ctx = make_ctx(capi, synth, w, h, gradients=source == 1)
    frames, depths = scene(synth, w, h)
    tabs, L = tables_of(O, synth, w, h, source)
    if source == 1:
        # asserted through the library's own producer first: the frames have candidates, and one lies on a pixel of zero depth (the
        # reference reads BYTE x of the 16-bit row there, so such a row exists and carries another pixel's byte as its z)
        for s in (0, 2, 3):
            rows, n = ctx.obtain_candidate_points(s, 0, THRESHOLD)
            assert n > 10 and rows.tobytes() == tabs[s].tobytes()
            assert (depths[s][rows[:, 1].astype(int), rows[:, 0].astype(int)] == 0).any(), s
        assert ctx.obtain_candidate_points(1, 0, THRESHOLD)[1] == 0
    n_rows = max(t.shape[0] for t in tabs)
    for n_frames in (1, 3, 5):
        slots = SLOTS[:n_frames]
        traj = poses_for(n_frames)
        for stride in (1, 7, 100, n_rows + 3):
            for mode in (0, 1):
                for skip in (0, 1):
                    want = CR.batch_cloud(O, [(tabs[s], traj[f], frames[s]) for f, s in enumerate(slots)], L, arith, mode, stride, skip)
                    if source == 0 and skip == 1 and stride in (1, 7):
                        assert 0 < want[1][0][3] < want[1][0][2]   # by construction, so that the compaction is not vacuous
                        if n_frames >= 3:   # the empty frame between two others starts where the next one starts
                            assert want[1][1][3] == 0 and want[1][1][2] > 0 and want[1][1][4] == want[1][2][4] and want[1][2][3] > 0
                    if source == 1 and n_frames >= 3:
                        assert want[1][1][1] == 0 and want[1][0][3] == want[1][0][2] > 0   # a candidate row always has w = 1
                    p = capi.default_cloud_params(mode=mode, stride=stride, skip_invalid=skip, source=source, threshold=THRESHOLD)
                    r = ctx.point_cloud_batch(slots, traj, p)
                    assert r["status"] == OK
                    check(r, want)
    ctx.close()


@pytest.mark.gpu
def test_gpu_frame_without_depth_plane(capi, synth, O, arith):
    w, h = 37, 23
    ctx = make_ctx(capi, synth, w, h, depth=False)
    frames, _ = scene(synth, w, h)
    tabs, L = tables_of(O, synth, w, h, 0, depth=False)
    assert (tabs[0][:, 2] == 1).all() and (tabs[0][:, 3] == 1).all()
    traj = poses_for(2)
    for mode in (0, 1):
        for skip in (0, 1):
            want = CR.batch_cloud(O, [(tabs[2], traj[0], frames[2]), (tabs[0], traj[1], frames[0])], L, arith, mode, 3, skip)
            check(ctx.point_cloud_batch([2, 0], traj, capi.default_cloud_params(mode=mode, stride=3, skip_invalid=skip)), want)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_full_size_dense_frame(capi, synth, O, arith):
    w, h = 640, 480
    frames, depths = scene(synth, w, h)
    ctx = capi.Context(capi.default_params(w, h, *intr(w, h), max_frames=1, max_pairs=1, n_levels=N_LEVELS, first_level=2, last_level=0,
                                           has_depth=1))
    ctx.upload_frames(0, frames[0][None], depths[0][None])
    p, L = oracle_level(O, w, h)
    tab = O.dense_points(depths[0], w, h, 0, p.depth_scale)
    traj = poses_for(1)
    for skip in (0, 1):
        want = CR.batch_cloud(O, [(tab, traj[0], frames[0])], L, arith, 0, 1, skip)
        assert want[2][4] == (w * h if skip == 0 else int((tab[:, 3] != 0).sum()))
        check(ctx.point_cloud_batch([0], traj, capi.default_cloud_params(stride=1, skip_invalid=skip)), want)
    ctx.close()


# ---- 1b. blocks that walk their run in several turns ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,skip,mode", [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)])
def test_gpu_blocks_of_several_turns(capi, synth, O, arith, source, skip, mode):
    """256 frames of 160 x 96 at stride 1: the launch is capped at 2048 blocks, so a frame has 8 blocks of 1920 selected rows, walked
    in 8 turns of 256 (the last one half full) — the cursor carried from turn to turn, the per-wave counts summed over turns, LDS
    reused between turns.  The shape of every large batch.  With a cap that ends inside a frame, and with a failed frame in the middle."""
    w, h, F = 160, 96, 256
    ctx = make_ctx(capi, synth, w, h, max_frames=F, gradients=source == 1)
    frames, _ = scene(synth, w, h)
    tabs, L = tables_of(O, synth, w, h, source)
    slots = [(3 * i + i // 7) % 4 for i in range(F)]
    traj = poses_for(F)
    p = capi.default_cloud_params(mode=mode, stride=1, skip_invalid=skip, source=source, threshold=THRESHOLD)
    batch = [(tabs[s], traj[f], frames[s]) for f, s in enumerate(slots)]
    want = CR.batch_cloud(O, batch, L, arith, mode, 1, skip)
    assert -(-(w * h) // 256) * F > 2048 and want[2][4] > 1000 * F   # more one-turn blocks than a launch holds
    r = ctx.point_cloud_batch(slots, traj, p)
    assert r["status"] == OK
    check(r, want)
    cap = want[1][200][4] + want[1][200][3] // 2 + 77   # inside frame 200, inside a block, inside a turn
    want_cap = CR.batch_cloud(O, batch, L, arith, mode, 1, skip, cap=cap)
    assert 0 < want_cap[1][200][5] < want_cap[1][200][3]
    r = ctx.point_cloud_batch(slots, traj, p, cap=cap)
    assert r["status"] == CAPACITY
    check(r, want_cap)
    traj[130, 1] = np.nan
    r = ctx.point_cloud_batch(slots, traj, p)
    assert r["status"] == PAIR_FAILED
    check(r, CR.batch_cloud(O, [(tabs[s], traj[f], frames[s]) for f, s in enumerate(slots)], L, arith, mode, 1, skip))
    ctx.close()


@pytest.mark.gpu
def test_gpu_explicit_table_of_several_turns(capi, synth, O, arith):
    """one table of 600 000 rows: 2048 blocks of 512 rows, two turns each (the last blocks one, or none)"""
    w, h = 40, 30
    ctx = make_ctx(capi, synth, w, h)
    frames, _ = scene(synth, w, h)
    _, L = oracle_level(O, w, h)
    rng = np.random.default_rng(8)
    n = 600_000
    tab = np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n), rng.uniform(0.1, 3, n), np.ones(n)], 1).astype(np.float32)
    tab[rng.random(n) < 0.3, 3] = 0
    pose = poses_for(3)[2]
    for mode, skip in ((0, 0), (1, 1)):
        want, _ = CR.frame_cloud(O, tab, pose, L, arith, mode, 1, skip, frames[0], 0)
        pts, count, st = ctx.point_cloud_points(0, tab, pose, capi.default_cloud_params(mode=mode, stride=1, skip_invalid=skip))
        assert st == OK and count == want.size and (skip == 0 or 0 < count < n) and pts.tobytes() == want.tobytes()
    ctx.close()


# ---- 2. the cap, the failed frame, the explicit table ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,skip", [(0, 0), (0, 1), (1, 0)])
def test_gpu_cap_below_the_total(capi, synth, O, torch, arith, source, skip):
    w, h = 160, 96
    ctx = make_ctx(capi, synth, w, h, gradients=source == 1)
    frames, _ = scene(synth, w, h)
    tabs, L = tables_of(O, synth, w, h, source)
    traj = poses_for(5)
    pts, _, _ = CR.batch_cloud(O, [(tabs[s], traj[f], frames[s]) for f, s in enumerate(SLOTS)], L, arith, 1, 7, skip)
    total = pts.size
    cap = total - total // 3   # ends inside a frame
    want = CR.batch_cloud(O, [(tabs[s], traj[f], frames[s]) for f, s in enumerate(SLOTS)], L, arith, 1, 7, skip, cap=cap)
    assert want[2] == (CAPACITY, 5, 0, 0, total, cap) and any(0 < r[5] < r[3] for r in want[1]) and want[1][-1][5] == 0
    p = capi.default_cloud_params(mode=1, stride=7, skip_invalid=skip, source=source, threshold=THRESHOLD)
    r = ctx.point_cloud_batch(SLOTS, traj, p, cap=cap)
    assert r["status"] == CAPACITY
    check(r, want)
    # the device form: the records beyond cap keep what they held
    room = total + 64
    d_pts = torch.full((room, 16), 0xA5, dtype=torch.uint8, device="cuda")
    d_info = torch.full((6, 32), 0xA5, dtype=torch.uint8, device="cuda")
    d_traj = torch.from_numpy(traj).cuda()
    torch.cuda.synchronize()   # torch's fills run on torch's stream, not on the context's
    ctx.point_cloud_batch_async(SLOTS, d_traj.data_ptr(), d_pts.data_ptr(), cap, d_info.data_ptr(), p)
    ctx.sync()
    got = d_pts.cpu().numpy()
    assert got[:cap].tobytes() == pts[:cap].tobytes() and (got[cap:] == 0xA5).all()
    info = d_info.cpu().numpy().reshape(-1).view(capi.CLOUD_INFO)
    assert info_tuples(info[:5]) == want[1] and info_tuples(info[5]) == [want[2]]
    # cap 0 with no buffer: the counts alone
    ctx.point_cloud_batch_async(SLOTS, d_traj.data_ptr(), None, 0, d_info.data_ptr(), p)
    ctx.sync()
    info = d_info.cpu().numpy().reshape(-1).view(capi.CLOUD_INFO)
    assert info_tuples(info[5]) == [(CAPACITY, 5, 0, 0, total, 0)] and (d_pts.cpu().numpy()[cap:] == 0xA5).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip", [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("bad", [0, 2, 4])
def test_gpu_pose_with_a_nan_empties_its_frame_only(capi, synth, O, arith, source, skip, bad):
    w, h = 40, 30
    ctx = make_ctx(capi, synth, w, h, gradients=source == 1)
    frames, _ = scene(synth, w, h)
    tabs, L = tables_of(O, synth, w, h, source)
    traj = poses_for(5)
    traj[bad, (2, 5, 6)[bad // 2]] = (np.nan, np.inf, -np.inf)[bad // 2]
    p = capi.default_cloud_params(mode=0, stride=3, skip_invalid=skip, source=source, threshold=THRESHOLD)
    r = ctx.point_cloud_batch(SLOTS, traj, p)
    assert r["status"] == PAIR_FAILED
    check(r, CR.batch_cloud(O, [(tabs[s], traj[f], frames[s]) for f, s in enumerate(SLOTS)], L, arith, 0, 3, skip))
    assert info_tuples(r["info"][bad])[0][:4] == (INVALID_ARG, 0, 0, 0)
    # its neighbours: the records of a run without it (their tags name their place in that run)
    keep = [f for f in range(5) if f != bad]
    r2 = ctx.point_cloud_batch([SLOTS[f] for f in keep], traj[keep], p)
    assert r2["status"] == OK and r2["points"].size == r["points"].size
    a, b = r["points"].copy(), r2["points"].copy()
    assert np.array_equal(a["tag"] >> 8, np.array(keep)[(b["tag"] >> 8)])
    a["tag"] &= 255
    b["tag"] &= 255
    assert a.tobytes() == b.tobytes()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(37, 23), (160, 96)])
def test_gpu_explicit_table_equals_the_batch_form(capi, synth, O, arith, w, h):
    ctx = make_ctx(capi, synth, w, h, gradients=True)
    frames, _ = scene(synth, w, h)
    traj = poses_for(1)
    for source in (0, 1):
        tabs, L = tables_of(O, synth, w, h, source)
        for mode in (0, 1):
            for stride in (1, 7, 100):
                for skip in (0, 1):
                    p = capi.default_cloud_params(mode=mode, stride=stride, skip_invalid=skip, source=source, threshold=THRESHOLD)
                    batch = ctx.point_cloud_batch([2], traj, p)
                    pts, count, st = ctx.point_cloud_points(2, tabs[2], traj[0], p)
                    assert st == OK and count == int(batch["call"]["offset"]) and pts.tobytes() == batch["points"].tobytes()
    # any producer's rows: not-a-number coordinates, rows outside the image, w = 0 and w = NaN
    rng = np.random.default_rng(2)
    tab = rng.uniform(-3, max(w, h) + 3, (1000, 4)).astype(np.float32)
    tab[::5, 3] = 0
    tab[7, 0] = np.nan
    tab[8, 1] = np.inf
    tab[9, 3] = np.nan
    _, L = oracle_level(O, w, h)
    for mode in (0, 1):
        for skip in (0, 1):
            want, n_sel = CR.frame_cloud(O, tab, traj[0], L, arith, mode, 1, skip, frames[1], 0)
            pts, count, st = ctx.point_cloud_points(1, tab, traj[0], capi.default_cloud_params(mode=mode, stride=1, skip_invalid=skip))
            assert st == OK and count == want.size and pts.tobytes() == want.tobytes()
            few, count2, st2 = ctx.point_cloud_points(1, tab, traj[0], capi.default_cloud_params(mode=mode, stride=1, skip_invalid=skip),
                                                      cap=10)
            assert st2 == CAPACITY and count2 == want.size and few.tobytes() == want[:10].tobytes()
    pts, count, st = ctx.point_cloud_points(0, np.zeros((0, 4), np.float32), traj[0])
    assert st == OK and count == 0 and pts.size == 0
    ctx.close()


# ---- 3. independence and determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,skip", [(0, 0), (0, 1), (1, 1)])
def test_gpu_place_in_the_batch_and_the_run_do_not_show(capi, synth, source, skip):
    w, h = 160, 96
    ctx = make_ctx(capi, synth, w, h, gradients=source == 1)
    traj = poses_for(5)
    traj[4] = traj[0]   # the same frame under the same pose at batch positions 0 and 4
    p = capi.default_cloud_params(mode=1, stride=1, skip_invalid=skip, source=source, threshold=THRESHOLD)
    r = ctx.point_cloud_batch(SLOTS, traj, p)
    assert r["status"] == OK
    i = r["info"]
    a = r["points"][int(i[0]["offset"]):int(i[0]["offset"]) + int(i[0]["n_points"])].copy()
    b = r["points"][int(i[4]["offset"]):int(i[4]["offset"]) + int(i[4]["n_points"])].copy()
    assert a.size == b.size > 0 and (a["tag"] >> 8 == 0).all() and (b["tag"] >> 8 == 4).all()
    a["tag"] &= 255
    b["tag"] &= 255
    assert a.tobytes() == b.tobytes()
    alone = ctx.point_cloud_batch([0], traj[:1], p)
    assert alone["points"].tobytes() == r["points"][:a.size].tobytes()
    again = ctx.point_cloud_batch(SLOTS, traj, p)
    assert again["points"].tobytes() == r["points"].tobytes() and again["info"].tobytes() == r["info"].tobytes()
    ctx.set_tuning(split=2, chained=0)   # launch shapes of other calls: nothing here depends on them
    tuned = ctx.point_cloud_batch(SLOTS, traj, p)
    assert tuned["points"].tobytes() == r["points"].tobytes()
    ctx.close()


# ---- 4. the trajectory in device memory and the chain ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 65])
def test_gpu_trajectory_on_device_pointers_equals_the_host_entry(capi, synth, torch, n):
    ctx = make_ctx(capi, synth, 40, 30)
    rng = np.random.default_rng(n)
    poses = np.concatenate([rng.normal(0, 0.05, (n, 3)), 1 + rng.normal(0, 0.05, (n, 1)), rng.normal(0, 0.01, (n, 3))], 1).astype(np.float32)
    start = np.array([0.1, 0.2, -0.1, 0.9, 1.0, -2.0, 0.5], np.float32)
    d_in = torch.from_numpy(poses).cuda()
    for axes in (False, True):
        for st, scale in ((None, 40.0), (start, 1.0)):
            d_out = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.accumulate_trajectory_device_async(d_in.data_ptr(), n, d_out.data_ptr(), start=st, t_scale=scale, reference_axes=axes)
            ctx.sync()
            want = ctx.accumulate_trajectory(poses, start=st, t_scale=scale, reference_axes=axes)
            assert d_out.cpu().numpy().tobytes() == want.tobytes(), (axes, scale)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_trajectory_row_by_row_from_a_device_pose(capi, synth, torch):
    """uwt_accumulate_trajectory_device_from_async: row k from row k - 1 in device memory, one pose per call, is bit for bit the one
    call over all poses; overlapping arguments are refused with nothing enqueued"""
    ctx = make_ctx(capi, synth, 40, 30)
    n = 65
    rng = np.random.default_rng(n)
    poses = np.concatenate([rng.normal(0, 0.05, (n, 3)), 1 + rng.normal(0, 0.05, (n, 1)), rng.normal(0, 0.01, (n, 3))], 1).astype(np.float32)
    d_in = torch.from_numpy(poses).cuda()
    d_out = torch.full((n, 7), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.accumulate_trajectory_device_async(d_in[0].data_ptr(), 1, d_out[0].data_ptr(), t_scale=40.0)
    for k in range(1, 20):
        ctx.accumulate_trajectory_device_from_async(d_in[k].data_ptr(), 1, d_out[k - 1].data_ptr(), d_out[k].data_ptr(), t_scale=40.0)
    ctx.accumulate_trajectory_device_from_async(d_in[20].data_ptr(), n - 20, d_out[19].data_ptr(), d_out[20].data_ptr(), t_scale=40.0)
    ctx.sync()
    want = ctx.accumulate_trajectory(poses, t_scale=40.0, reference_axes=False)
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    before = d_out.cpu().numpy().tobytes()
    for call in (lambda: ctx.accumulate_trajectory_device_async(d_out.data_ptr(), n, d_out.data_ptr()),                       # in place
                 lambda: ctx.accumulate_trajectory_device_async(d_out[1].data_ptr(), 4, d_out.data_ptr()),                    # shifted
                 lambda: ctx.accumulate_trajectory_device_from_async(d_in.data_ptr(), 3, d_out[1].data_ptr(), d_out.data_ptr()),   # start inside
                 lambda: ctx.accumulate_trajectory_device_from_async(d_out[4].data_ptr(), 3, d_in.data_ptr(), d_out[2].data_ptr())):
        with pytest.raises(capi.UwtError) as e:
            call()
        assert e.value.status == INVALID_ARG
    ctx.sync()
    assert d_out.cpu().numpy().tobytes() == before
    ctx.close()


@pytest.mark.gpu
def test_gpu_chain_tracking_trajectory_cloud_with_one_wait(capi, synth, torch):
    w, h = 160, 96
    ctx = make_ctx(capi, synth, w, h, gradients=True)
    ref, tgt = [0, 2, 0], [1, 3, 3]
    i32 = dict(dtype=torch.int32, device="cuda")
    cap = 256
    t = dict(poses=torch.zeros((3, 7), **i32), stats=torch.zeros((3, 4), **i32), info=torch.zeros((3, 8), **i32),
             good=torch.zeros((3, cap, 3), **i32), kept_prev=torch.zeros((3, cap, 8), **i32), kept_cur=torch.zeros((3, cap, 8), **i32),
             n_matches=torch.zeros((3,), **i32))
    p = capi.default_cloud_params(stride=7, skip_invalid=1)
    room = 3 * (-(-(w * h) // 7))
    d_traj = torch.zeros((3, 7), dtype=torch.float32, device="cuda")
    d_pts = torch.zeros((room, 16), dtype=torch.uint8, device="cuda")
    d_info = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.tracking_batch_async(ref, tgt, {k: v.data_ptr() for k, v in t.items()}, cap=cap)
    ctx.accumulate_trajectory_device_async(t["poses"].data_ptr(), 3, d_traj.data_ptr(), t_scale=40.0, reference_axes=False)
    ctx.point_cloud_batch_async(tgt, d_traj.data_ptr(), d_pts.data_ptr(), room, d_info.data_ptr(), p)
    ctx.sync()   # the only wait
    poses = t["poses"].cpu().numpy().view(np.float32)
    stats = t["stats"].cpu().numpy().view(capi.STATS).reshape(-1)
    assert stats["status"][0] == OK and not np.array_equal(poses[0], IDENTITY)
    traj = ctx.accumulate_trajectory(poses, t_scale=40.0, reference_axes=False)   # the staged host path
    assert d_traj.cpu().numpy().tobytes() == traj.tobytes()
    staged = ctx.point_cloud_batch(tgt, traj, p)
    info = d_info.cpu().numpy().reshape(-1).view(capi.CLOUD_INFO)
    assert info[:3].tobytes() == staged["info"].tobytes() and info[3].tobytes() == staged["call"].tobytes()
    n = int(info[3]["written"])
    assert n == int(info[3]["offset"]) > 0 and d_pts.cpu().numpy()[:n].tobytes() == staged["points"].tobytes()
    ctx.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_refusals_enqueue_nothing(capi, synth, torch):
    ctx = make_ctx(capi, synth, 40, 30, max_frames=4)
    d_pts = torch.full((64, 16), 0x5A, dtype=torch.uint8, device="cuda")
    d_info = torch.full((6, 32), 0x5A, dtype=torch.uint8, device="cuda")
    d_traj = torch.zeros((5, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    good = dict(slots=[0, 1], traj=d_traj.data_ptr(), pts=d_pts.data_ptr(), cap=64, info=d_info.data_ptr())
    cases = [dict(params=dict(mode=2)), dict(params=dict(mode=-1)), dict(params=dict(source=2)), dict(params=dict(stride=0)),
             dict(params=dict(skip_invalid=2)), dict(params=dict(threshold=float("nan"))), dict(params=dict(threshold=float("inf"))),
             dict(slots=[0, 4]), dict(slots=[-1]), dict(slots=[0, 1, 2, 3, 0]), dict(traj=None), dict(info=None), dict(pts=None),
             dict(cap=-1)]
    for kw in cases:
        a = dict(good, **{k: v for k, v in kw.items() if k != "params"})
        p = capi.default_cloud_params(**kw.get("params", {}))
        with pytest.raises(capi.UwtError) as e:
            ctx.point_cloud_batch_async(a["slots"], a["traj"], a["pts"], a["cap"], a["info"], p)
        assert e.value.status == INVALID_ARG, kw
    p = capi.default_cloud_params()
    p.reserved[1] = 1
    with pytest.raises(capi.UwtError):
        ctx.point_cloud_batch_async(good["slots"], good["traj"], good["pts"], good["cap"], good["info"], p)
    st = capi.lib().uwt_point_cloud_batch_async(ctx._h, 0, None, C.c_void_p(good["traj"]), C.byref(capi.default_cloud_params()),
                                                C.c_void_p(good["pts"]), C.c_int64(64), C.c_void_p(good["info"]))
    assert st == INVALID_ARG
    ctx.sync()
    assert (d_pts.cpu().numpy() == 0x5A).all() and (d_info.cpu().numpy() == 0x5A).all()
    with pytest.raises(capi.UwtError):
        ctx.point_cloud_points(0, np.ones((4, 4), np.float32), [0, 0, 0, 1, np.nan, 0, 0])
    ctx.close()


# ---- 6. the tool -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_track_sequence_cloud_chained_equals_staged(capi, synth, torch):
    """tools/track_sequence.py --live --chained --cloud enqueues trajectory and cloud behind the tracking calls, inside the single wait:
    the records of the staged form over the poses it returns, and poses that --cloud does not change"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "track_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    w, h, intr_ = 256, 240, (210.0, 210.0, 127.5, 119.5)
    frames, _, _, _ = synth.render_sequence(w, h, *intr_, 4, seed=3)
    frames = list(frames)
    plain = tool.track_live_chained(w, h, intr_, frames, None)
    for mode in (0, 1):
        poses, stats, kept, cloud = tool.track_live_chained(w, h, intr_, frames, None, cloud=(7, mode))
        assert poses.view(np.uint32).tobytes() == plain[0].view(np.uint32).tobytes() and kept == plain[2]
        staged = tool.sequence_cloud(w, h, intr_, frames, None, poses, 7, mode)
        assert cloud.size == 3 * -(-(w * h) // 7) and cloud.tobytes() == staged.tobytes()
        assert np.array_equal(np.unique(cloud["tag"] >> 8), [0, 1, 2])
