"""Tracker::ObtainImageTransformed and DebugShowWarpedPerspective on the device (uwt_obtain_image_transformed, uwt_warp_image_batch*,
uwt_warp_mosaic): every output compared AS BYTES / INTEGERS — no tolerance anywhere — with the numpy restatement
(tests/warp_image_ref.py: the literal sequential loop, and the dense form composed from oracle.dense_points, level_intrinsics and warp)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import warp_image_ref as WR

OK, INVALID_ARG, PAIR_FAILED = 0, 1, 6   # uwt_status_code (include/uwt.h)
INTR = {(160, 96): (131.25, 131.25, 79.5, 47.5), (165, 99): (135.0, 135.0, 82.0, 49.0)}
SIZES = [(160, 96), (165, 99)]   # pitch = width; pitch 168 with odd rows, img_w > w at the coarse levels, a masked last group
N_LEVELS = 3
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)   # qx qy qz qw tx ty tz
CONTRACT = np.array([0, 0, 0, 1, 0, 0, 0.3], np.float32)   # z ~ 1 -> 1.3: the image shrinks by 1 / 1.3, many rows share a pixel
EXPAND = np.array([0, 0, 0, 1, 0, 0, -0.3], np.float32)    # z ~ 1 -> 0.7: holes inside the covered region
ROLL = np.array([0, 0, np.sin(np.deg2rad(2.5)), np.cos(np.deg2rad(2.5)), 0, 0, 0], np.float32)   # 5 degrees about the optical axis
PAIRS = [(0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (2, 3), (0, 3), (2, 2)]   # repeated reference slots, one (slot, same slot)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


_scenes = {}


def scene(synth, w, h, depth):
    """four frames (two rendered pairs), their depth images or None, and the first pair's ground-truth pose"""
    key = (w, h, depth)
    if key not in _scenes:
        a = synth.render_pair(w, h, *INTR[(w, h)], seed=5, with_depth=depth)
        b = synth.render_pair(w, h, *INTR[(w, h)], seed=6, with_depth=depth)
        gt = np.concatenate([synth._quat_from_R(a[3]), a[4]]).astype(np.float32)
        frames = [a[0], a[1], b[0], b[1]]
        depths = [a[2], a[2], b[2], b[2]] if depth else None
        _scenes[key] = (frames, depths, gt)
    return _scenes[key]


def make_ctx(capi, synth, w, h, depth, max_pairs=8, gradients=False):
    frames, depths, gt = scene(synth, w, h, depth)
    ctx = capi.Context(capi.default_params(w, h, *INTR[(w, h)], max_frames=4, max_pairs=max_pairs, n_levels=N_LEVELS, first_level=2,
                                           last_level=0, has_depth=int(depth)))
    ctx.upload_frames(0, np.stack(frames), np.stack(depths) if depth else None)
    ctx.build_pyramids(0, 4)
    if gradients:
        ctx.apply_gradient(0, 4)
    return ctx, gt


def oracle_params(O, w, h, depth):
    return O.default_params(w, h, *INTR[(w, h)], n_levels=N_LEVELS, first_level=2, last_level=0, has_depth=int(depth))


def planes(ctx, capi, lvl, depth):
    img = [ctx.get_plane(s, lvl, capi.PLANE_IMAGE) for s in range(4)]
    dep = [ctx.get_plane(s, lvl, capi.PLANE_DEPTH) for s in range(4)] if depth else [None] * 4
    return img, dep


def batch_poses(gt):
    return np.stack([IDENTITY, gt, CONTRACT, EXPAND, ROLL, IDENTITY, CONTRACT, IDENTITY])


def quality_tuple(rec):
    return tuple(int(rec[k]) for k in WR.QUALITY_FIELDS)


def result_of(r, i):
    return dict(quality=quality_tuple(r["quality"][i]), warped=r["warped"][i].tobytes(), valid=r["valid"][i].tobytes(),
                absdiff=r["absdiff"][i].tobytes())


def want_of(ref):
    return dict(quality=tuple(ref["quality"][k] for k in WR.QUALITY_FIELDS), warped=ref["warped"].tobytes(), valid=ref["valid"].tobytes(),
                absdiff=ref["absdiff"].tobytes())


def differs(got, want):
    for k, v in want.items():
        if got[k] != v:
            return "%s: %r against %r" % (k, got[k] if k == "quality" else len(got[k]), v if k == "quality" else len(v))
    return None


def built_table(rng, rows, cols):
    """4 000 rows on 50 distinct targets, targets on row 0, column 0, cols - 1 and rows - 1, exact halves, NaN rows and rows with
    (x1, y1) outside the image"""
    n = 4000
    tx = rng.integers(1, cols - 1, 50).astype(np.float32)
    ty = rng.integers(1, rows - 1, 50).astype(np.float32)
    tx[:8] = [0, 5, cols - 1, 7, cols - 1, 0, cols, 3]
    ty[:8] = [4, 0, 6, rows - 1, rows - 1, 0, 2, rows]
    pick = rng.integers(0, 50, n)
    pts = np.ones((n, 4), np.float32)
    pts[:, 0] = rng.uniform(-0.9, cols - 0.01, n)
    pts[:, 1] = rng.uniform(-0.9, rows - 0.01, n)
    wp = np.ones((n, 4), np.float32)
    wp[:, 0] = tx[pick] + rng.uniform(-0.49, 0.49, n).astype(np.float32)
    wp[:, 1] = ty[pick] + rng.uniform(-0.49, 0.49, n).astype(np.float32)
    wp[100:200, 0] = tx[pick[100:200]] - 0.5   # exact halves: x.5 rounds up, away from zero
    wp[200:300, 1] = ty[pick[200:300]] + 0.5
    wp[300:320, 0] = np.nan
    wp[320:330, 1] = np.inf
    wp[330:340, 0] = 3e9
    pts[340:360, 0] = cols
    pts[360:380, 1] = -1.0
    pts[380:390, 0] = np.nan
    wp[-1, :2] = [tx[20], ty[20]]   # the last row lands for certain
    return pts, wp


# ---- 1. the explicit form -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("lvl", [0, 2])
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_explicit_form_equals_the_loop(capi, synth, O, w, h, lvl, depth):
    ctx, gt = make_ctx(capi, synth, w, h, depth, gradients=True)
    img, dep = planes(ctx, capi, lvl, depth)
    p = oracle_params(O, w, h, depth)
    L, dense_pts, dense_wp = WR.dense_table(O, p, lvl, dep[0], CONTRACT)
    cand = ctx.obtain_candidate_points(0, lvl, 5.0)[0]
    assert len(cand) > 10
    k = int(np.nonzero(WR.landing(img[0].shape, dense_pts, dense_wp)[0])[0][-1])   # a row that lands
    rng = np.random.default_rng(11)
    tables = dict(dense=(dense_pts, dense_wp), candidates=(cand, O.warp(cand, gt, L)), built=built_table(rng, *img[0].shape),
                  empty=(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)), one=(dense_pts[k:k + 1], dense_wp[k:k + 1]))
    prefill = rng.integers(1, 256, img[0].shape, dtype=np.uint8)   # non-zero: pixels not landed on must keep it
    for name, (pts, wp) in tables.items():
        want = prefill.copy()
        want_valid = WR.obtain_image_transformed(img[0], pts, wp, want)
        got, got_valid = ctx.obtain_image_transformed(0, lvl, pts, wp, prefill)
        assert got.tobytes() == want.tobytes() and got_valid.tobytes() == want_valid.tobytes(), name
        assert not got_valid[0].any() and not got_valid[:, 0].any(), name
    assert not ctx.obtain_image_transformed(0, lvl, *tables["empty"], prefill)[1].any()
    assert ctx.obtain_image_transformed(0, lvl, *tables["one"])[1].sum() == 1
    ctx.close()


# ---- 2. the dense batch ---------------------------------------------------------------------------------------------------------------
def dense_references(O, ctx, capi, w, h, lvl, depth, poses, pairs=PAIRS):
    img, dep = planes(ctx, capi, lvl, depth)
    p = oracle_params(O, w, h, depth)
    return [WR.dense_reference(O, p, lvl, img[a], img[b], dep[a], poses[i]) for i, (a, b) in enumerate(pairs)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_dense_batch_equals_explicit_form_and_reference(capi, synth, O, w, h, depth):
    ctx, gt = make_ctx(capi, synth, w, h, depth)
    poses = batch_poses(gt)
    p = oracle_params(O, w, h, depth)
    for lvl in (0, 2):
        refs = dense_references(O, ctx, capi, w, h, lvl, depth, poses)
        Li = ctx.level_info(lvl)
        # asserted on the reference alone, before any comparison: the ordering rule is exercised, and the expanding pose leaves holes
        q = refs[2]["quality"]
        assert q["n_landed"] - q["n_covered"] >= 0.2 * q["n_landed"] and q["n_landed"] > 0, q
        v = refs[3]["valid"]
        ys, xs = np.nonzero(v)
        box = v[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        assert (box == 0).sum() >= 0.1 * box.size
        if not depth:
            assert refs[0]["quality"]["n_covered"] == (min(Li.img_w, Li.w) - 1) * (min(Li.img_h, Li.h) - 1)
        assert refs[0]["quality"]["sum_abs"] == refs[0]["quality"]["sum_abs_unaligned"]
        assert refs[7]["quality"]["sum_abs"] == 0 and refs[7]["quality"]["n_covered"] > 0
        r = ctx.warp_image_batch([a for a, _ in PAIRS], [b for _, b in PAIRS], poses, lvl=lvl)
        assert r["status"] == OK
        img, dep = planes(ctx, capi, lvl, depth)
        for i, (a, b) in enumerate(PAIRS):
            d = differs(result_of(r, i), want_of(refs[i]))
            assert d is None, (lvl, i, d)
            _, pts, wp = WR.dense_table(O, p, lvl, dep[a], poses[i])
            wp_dev = ctx.warp(lvl, pts, poses[i])
            assert wp_dev.tobytes() == wp.tobytes()
            got, got_valid = ctx.obtain_image_transformed(a, lvl, pts, wp_dev)
            assert got.tobytes() == r["warped"][i].tobytes() and got_valid.tobytes() == r["valid"][i].tobytes(), (lvl, i)
    ctx.close()


# ---- 3. determinism and independence ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_gpu_determinism_and_independence(capi, synth, depth):
    w, h = 165, 99
    ctx, gt = make_ctx(capi, synth, w, h, depth)
    poses = batch_poses(gt)
    ref, tgt = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    for lvl in (0, 2):
        first = ctx.warp_image_batch(ref, tgt, poses, lvl=lvl)
        want = [result_of(first, i) for i in range(8)]
        for _ in range(2):
            again = ctx.warp_image_batch(ref, tgt, poses, lvl=lvl)
            assert [result_of(again, i) for i in range(8)] == want
        rev = ctx.warp_image_batch(ref[::-1], tgt[::-1], poses[::-1], lvl=lvl)
        assert [result_of(rev, 7 - i) for i in range(8)] == want
        for i in range(8):
            assert result_of(ctx.warp_image_batch(ref[i:i + 1], tgt[i:i + 1], poses[i:i + 1], lvl=lvl), 0) == want[i], i
        other = dict(split=2, tail_update=2, first_poll=1, typed_loads=0, target_blocks=256)
        t0 = ctx.get_tuning()
        saved = {k: getattr(t0, k) for k in other}
        ctx.set_tuning(**other)
        tuned = ctx.warp_image_batch(ref, tgt, poses, lvl=lvl)
        assert [result_of(tuned, i) for i in range(8)] == want
        ctx.set_tuning(**saved)
    ctx.close()


# ---- 4. chained use ---------------------------------------------------------------------------------------------------------------------
def device_outputs(torch, P, n_plane, fill=0):
    u8 = dict(dtype=torch.uint8, device="cuda")
    s = dict(warped=torch.full((P, n_plane), fill, **u8), valid=torch.full((P, n_plane), fill, **u8),
             absdiff=torch.full((P, n_plane), fill, **u8), quality=torch.full((P, 48), fill, **u8))
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    return s


def fetch(capi, s, L):
    """a device set as warp_image_batch returns its results (the pad columns of the pitched rows dropped)"""
    host = {k: v.cpu().numpy() for k, v in s.items()}
    P = host["quality"].shape[0]
    cut = lambda a: np.ascontiguousarray(a.reshape(P, L.img_h, L.pitch)[:, :, :L.img_w])
    return dict(warped=cut(host["warped"]), valid=cut(host["valid"]), absdiff=cut(host["absdiff"]),
                quality=host["quality"].reshape(-1).view(capi.WARP_QUALITY), raw=host)


@pytest.mark.gpu
def test_gpu_chained_behind_the_tracking_calls(capi, synth, torch):
    w, h = 160, 96
    ctx, gt = make_ctx(capi, synth, w, h, False, gradients=True)
    L = ctx.level_info(0)
    ref, tgt = [0, 2, 0], [1, 3, 3]
    i32 = dict(dtype=torch.int32, device="cuda")
    cap = 256
    t = dict(poses=torch.zeros((3, 7), **i32), stats=torch.zeros((3, 4), **i32), info=torch.zeros((3, 8), **i32),
             good=torch.zeros((3, cap, 3), **i32), kept_prev=torch.zeros((3, cap, 8), **i32), kept_cur=torch.zeros((3, cap, 8), **i32),
             n_matches=torch.zeros((3,), **i32))
    s = device_outputs(torch, 3, L.pitch * L.img_h, fill=0x5A)
    ctx.tracking_batch_async(ref, tgt, {k: v.data_ptr() for k, v in t.items()}, cap=cap)
    ctx.warp_image_batch_async(ref, tgt, t["poses"].data_ptr(), {k: v.data_ptr() for k, v in s.items()}, lvl=0)
    ctx.sync()   # the only wait
    got = fetch(capi, s, L)
    poses = t["poses"].cpu().numpy().view(np.float32)
    stats = t["stats"].cpu().numpy().view(capi.STATS).reshape(-1)
    assert stats["status"][0] == OK and stats["status"][1] == OK and not np.array_equal(poses[0], IDENTITY)
    staged = ctx.warp_image_batch(ref, tgt, poses, lvl=0)   # the poses taken to the host and back
    for i in range(3):
        assert result_of(got, i) == result_of(staged, i), i
    assert got["quality"]["n_covered"][0] > 0.8 * w * h

    # the live call from key points, one pair without any: its tracking fails, its pose is the identity, its record is the identity's
    kept = t["kept_prev"].cpu().numpy().view(capi.KEYPOINT).reshape(3, cap)
    n = t["n_matches"].cpu().numpy()
    kps = [np.stack([kept[i, :n[i]]["x"], kept[i, :n[i]]["y"]], 1) for i in range(2)] + [np.zeros((0, 2), np.float32)]
    t2 = dict(poses=torch.zeros((3, 7), **i32), stats=torch.zeros((3, 4), **i32))
    s2 = device_outputs(torch, 3, L.pitch * L.img_h, fill=0x5A)
    ctx.track_features_batch_async(ref, tgt, kps, t2["poses"].data_ptr(), t2["stats"].data_ptr())
    ctx.warp_image_batch_async(ref, tgt, t2["poses"].data_ptr(), {k: v.data_ptr() for k, v in s2.items()}, lvl=0)
    ctx.sync()
    got2 = fetch(capi, s2, L)
    poses2 = t2["poses"].cpu().numpy().view(np.float32)
    stats2 = t2["stats"].cpu().numpy().view(capi.STATS).reshape(-1)
    assert stats2["status"][0] == OK and stats2["status"][2] != OK and np.array_equal(poses2[2], IDENTITY)
    staged2 = ctx.warp_image_batch(ref, tgt, poses2, lvl=0)
    for i in range(3):
        assert result_of(got2, i) == result_of(staged2, i), i
    ident = ctx.warp_image_batch([0], [3], IDENTITY[None], lvl=0)
    assert result_of(got2, 2) == result_of(ident, 0) and got2["quality"]["status"][2] == OK
    ctx.close()


# ---- 5. refusals and the failed pair ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals_leave_outputs_untouched(capi, synth, torch):
    w, h = 160, 96
    ctx, gt = make_ctx(capi, synth, w, h, False, max_pairs=2)
    L = ctx.level_info(0)
    lib = capi.lib()
    s = device_outputs(torch, 2, L.pitch * L.img_h, fill=0x5A)
    poses = torch.zeros((2, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    io = {k: v.data_ptr() for k, v in s.items()}
    bad = [dict(ref=[4]), dict(tgt=[-1]), dict(ref=[], tgt=[]), dict(ref=[0, 0, 0], tgt=[1, 1, 1]), dict(lvl=-1), dict(lvl=N_LEVELS),
           dict(io=dict(io, quality=None)), dict(poses=0)]
    for kw in bad:
        with pytest.raises(capi.UwtError) as e:
            ctx.warp_image_batch_async(kw.get("ref", [0]), kw.get("tgt", [1]), kw.get("poses", poses.data_ptr()), kw.get("io", io),
                                       lvl=kw.get("lvl", 0))
        assert e.value.status == INVALID_ARG and lib.uwt_last_error(ctx._h), kw
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    rec = capi.WarpImageIO(*[io[k] for k in ("warped", "valid", "absdiff", "quality")])
    for a, b, r in ((None, two, rec), (one, None, rec), (one, two, None)):   # null lists, a null io: the raw entry point
        st = lib.uwt_warp_image_batch_async(ctx._h, 1, C.c_void_p(a.ctypes.data) if a is not None else None,
                                            C.c_void_p(b.ctypes.data) if b is not None else None, 0, C.c_void_p(poses.data_ptr()),
                                            C.byref(r) if r is not None else None)
        assert st == INVALID_ARG
    ctx.sync()
    assert all(bool((v == 0x5A).all()) for v in s.values())   # nothing was enqueued
    # the host forms
    img = np.full((L.img_h, L.img_w), 0x5A, np.uint8)
    valid = np.full((L.img_h, L.img_w), 0x5A, np.uint8)
    pts = np.ones((4, 4), np.float32)
    for slot, lvl, n in ((4, 0, 4), (-1, 0, 4), (0, N_LEVELS, 4), (0, 0, -1)):
        st = lib.uwt_obtain_image_transformed(ctx._h, slot, lvl, C.c_void_p(pts.ctypes.data), C.c_void_p(pts.ctypes.data), n,
                                              C.c_void_p(img.ctypes.data), C.c_void_p(valid.ctypes.data))
        assert st == INVALID_ARG and (img == 0x5A).all() and (valid == 0x5A).all(), (slot, lvl, n)
    mosaic = np.full((2 * L.img_h, 2 * L.img_w), 0x5A, np.uint8)
    for a, b, lvl in ((4, 1, 0), (0, -1, 0), (0, 1, N_LEVELS)):
        st = lib.uwt_warp_mosaic(ctx._h, a, b, lvl, C.c_void_p(img.ctypes.data), C.c_void_p(mosaic.ctypes.data))
        assert st == INVALID_ARG and (mosaic == 0x5A).all()
    assert ctx.warp_image_batch([0], [1], IDENTITY[None])["status"] == OK   # the context still works
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_gpu_failed_pair_leaves_its_neighbours_alone(capi, synth, bad):
    w, h = 165, 99
    ctx, gt = make_ctx(capi, synth, w, h, True)
    poses = batch_poses(gt)
    ref, tgt = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    clean = ctx.warp_image_batch(ref, tgt, poses)
    broken = poses.copy()
    broken[2, 5] = bad
    with pytest.raises(capi.UwtError) as e:
        ctx.warp_image_batch(ref, tgt, broken, raise_on_pair_failure=True)
    assert e.value.status == PAIR_FAILED
    r = ctx.warp_image_batch(ref, tgt, broken)
    assert r["status"] == PAIR_FAILED
    assert quality_tuple(r["quality"][2]) == (INVALID_ARG, 0, 0, 0, 0, 0, 0, 0)
    assert not r["warped"][2].any() and not r["valid"][2].any() and not r["absdiff"][2].any()
    for i in range(8):
        if i != 2:
            assert result_of(r, i) == result_of(clean, i), i
    ctx.close()


# ---- 6. the mosaic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_mosaic_equals_reference(capi, synth, w, h):
    ctx, gt = make_ctx(capi, synth, w, h, False)
    for lvl in (0, 2):
        img, _ = planes(ctx, capi, lvl, False)
        r = ctx.warp_image_batch([0], [1], gt[None], lvl=lvl)
        for warped in (r["warped"][0], np.full(img[0].shape, 255, np.uint8)):   # (255 + 255: the cap)
            got = ctx.warp_mosaic(0, 1, lvl, warped)
            assert got.tobytes() == WR.mosaic(img[0], img[1], warped).tobytes(), lvl
    ctx.close()


# ---- 7. the mirrors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_c_abi(capi, synth, O):
    tracker_mod = importlib.import_module("uw-slam_amd.tracker")
    w, h = 160, 96
    frames, _, gt = scene(synth, w, h, False)
    ctx, _ = make_ctx(capi, synth, w, h, False)
    fx, fy, cx, cy = INTR[(w, h)]
    tr = tracker_mod.Tracker(False, max_frames=4, n_levels=N_LEVELS, first_level=2, last_level=0)
    tr.InitializePyramid(w, h, np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32))
    fr = [tracker_mod.Frame(f) for f in frames]
    poses = np.stack([gt, CONTRACT])
    warped, valid, quality = tr.WarpedImageBatch([(fr[0], fr[1]), (fr[2], fr[3])], poses)
    want = ctx.warp_image_batch([0, 2], [1, 3], poses)
    assert warped.tobytes() == want["warped"].tobytes() and valid.tobytes() == want["valid"].tobytes()
    assert quality.tobytes() == want["quality"].tobytes()
    p = oracle_params(O, w, h, False)
    for lvl, original in ((0, frames[0]), (2, tr.GetFrameData(fr[0], 2, capi.PLANE_IMAGE)), (0, (frames[0] // 2 + 3).astype(np.uint8))):
        _, pts, wp = WR.dense_table(O, p, lvl, None, CONTRACT)
        out = np.full(original.shape, 9, np.uint8)
        ref_out = out.copy()
        ref_valid = WR.obtain_image_transformed(original, pts, wp, ref_out)
        got_valid = tr.ObtainImageTransformed(original, pts, wp, out)   # a resident level 0, a resident level 2, pixels of no frame
        assert out.tobytes() == ref_out.tobytes() and got_valid.tobytes() == ref_valid.tobytes(), lvl
    m = tr.DebugShowWarpedPerspective(frames[0], frames[1], warped[0], 0)
    assert m.tobytes() == ctx.warp_mosaic(0, 1, 0, want["warped"][0]).tobytes()
    ctx.close()


# ---- 8. the tool --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_track_sequence_quality_chained_equals_staged(capi, synth, torch):
    """tools/track_sequence.py --live --chained --quality takes its records from the device poses inside the single wait: the records
    of the staged form over the poses it returns, and poses that --quality does not change"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "track_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    w, h, intr = 256, 240, (210.0, 210.0, 127.5, 119.5)
    frames, _, rel, _ = synth.render_sequence(w, h, *intr, 4, seed=3)
    frames = list(frames)
    plain = tool.track_live_chained(w, h, intr, frames, None)
    poses, stats, kept, records = tool.track_live_chained(w, h, intr, frames, None, quality=True)
    assert len(plain) == 3 and poses.view(np.uint32).tobytes() == plain[0].view(np.uint32).tobytes() and kept == plain[2]
    staged = tool.sequence_quality(w, h, intr, frames, None, poses)
    assert records.tobytes() == staged.tobytes() and (records["status"] == OK).all()
    cols = tool.quality_columns(records, w, h)
    assert sorted(cols) == ["coverage", "mean_abs", "mean_abs_unaligned"] and all(len(v) == 3 for v in cols.values())
    assert min(cols["coverage"]) > 0.8
    # the columns answer the question they are for: under the poses the frames were rendered with, the previous frame carried into
    # the current one's view differs less from it than the previous frame as it is
    true = tool.quality_columns(tool.sequence_quality(w, h, intr, frames, None, np.asarray(rel, np.float32)), w, h)
    assert min(true["coverage"]) > 0.8 and all(a < u for a, u in zip(true["mean_abs"], true["mean_abs_unaligned"]))
