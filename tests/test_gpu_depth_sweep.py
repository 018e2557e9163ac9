"""The depth sweep on the device (uwt_sweep_depth_batch*, EXTENSION): every output compared AS BYTES / INTEGERS — no tolerance anywhere —
with the numpy restatement (tests/depth_sweep_ref.py) on the designed inputs of tests/depth_sweep_cases.py, whose reach
tests/test_depth_sweep_cpu.py shows on the restatement alone."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import depth_sweep_cases as DC
import depth_sweep_ref as SR
import guard_bands as GB

OK, INVALID_ARG, PAIR_FAILED = 0, 1, 6   # uwt_status_code (include/uwt.h)
FILL = 0x5A


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def make_ctx(capi, case, max_pairs=8, has_depth=0, n_levels=DC.N_LEVELS):
    """the case's frames resident in slots 0.. (the reference first), pyramids built, gradients applied"""
    w, h = case["size"]
    n = len(case["frames"])
    ctx = capi.Context(capi.default_params(w, h, *case["intr"], max_frames=max(n, 2), max_pairs=max_pairs, n_levels=n_levels,
                                           first_level=n_levels - 1, last_level=0, has_depth=has_depth, depth_scale=DC.DEPTH_SCALE))
    ctx.upload_frames(0, np.stack(case["frames"]), np.zeros((n, h, w), np.uint16) if has_depth else None)
    ctx.build_pyramids(0, n)
    ctx.apply_gradient(0, n)
    return ctx


def sweep_params(capi, case):
    return capi.default_sweep_params(n_views=len(case["poses"]), n_hyp=len(case["codes"]), **case["params"])


def device_outputs(torch, J, n_plane, fill=FILL):
    u8 = dict(dtype=torch.uint8, device="cuda")
    s = dict(depth=torch.full((J, 2 * n_plane), fill, **u8), cost=torch.full((J, 2 * n_plane), fill, **u8),
             outcome=torch.full((J, n_plane), fill, **u8), info=torch.full((J, 64), fill, **u8))
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    return s


def fetch(capi, s, L):
    """a device set as sweep_depth returns its results, and the pad columns of the pitched rows apart"""
    host = {k: v.cpu().numpy() for k, v in s.items()}
    J = host["info"].shape[0]
    d = host["depth"].view(np.uint16).reshape(J, L.img_h, L.pitch)
    c = host["cost"].view(np.uint16).reshape(J, L.img_h, L.pitch)
    o = host["outcome"].reshape(J, L.img_h, L.pitch)
    pad = np.concatenate([a[:, :, L.img_w:].reshape(-1).view(np.uint8) for a in (d, c, o)])
    cut = lambda a: np.ascontiguousarray(a[:, :, :L.img_w])
    return dict(depth=cut(d), cost=cut(c), outcome=cut(o), info=host["info"].reshape(-1).view(capi.SWEEP_INFO), pad=pad)


def result_of(r, i):
    return dict(info=SR.info_tuple(r["info"][i]), depth=r["depth"][i].tobytes(), cost=r["cost"][i].tobytes(), outcome=r["outcome"][i].tobytes())


def want_of(ref):
    return dict(info=SR.info_tuple(ref["info"]), depth=ref["depth"].tobytes(), cost=ref["cost"].tobytes(), outcome=ref["outcome"].tobytes())


def differs(got, want):
    for k, v in want.items():
        if got[k] != v:
            if k == "info":
                return "info: %r against %r" % (got[k], v)
            dt = np.uint8 if k == "outcome" else np.uint16
            a, b = np.frombuffer(got[k], dt), np.frombuffer(v, dt)
            at = np.flatnonzero(a != b)
            return "%s: %d elements differ, first at %d: %d against %d" % (k, at.size, at[0], a[at[0]], b[at[0]])
    return None


# ---- 1. bit for bit the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_gpu_case_equals_the_restatement(capi, synth, O, torch, arith, name):
    case = DC.build(synth, name)
    ref = DC.reference(O, arith, synth, name)
    ctx = make_ctx(capi, case)
    p = sweep_params(capi, case)
    L = ctx.level_info(p.lvl)
    assert L.pitch % 4 == 0 and (L.pitch != L.img_w) == (case["size"][0] == 61)
    nv = len(case["poses"])
    # the level's images are the restatement's, and source 1 selects exactly the pixels uwt_obtain_candidate_points returns
    imgs = DC.level_images(O, case)
    for s in range(1 + nv):
        assert ctx.get_plane(s, p.lvl, capi.PLANE_IMAGE).tobytes() == imgs[s].tobytes()
    if p.source == 1:
        cand = ctx.obtain_candidate_points(0, p.lvl, p.threshold)[0]
        sel = np.zeros(imgs[0].shape, bool)
        sel[cand[:, 1].astype(int), cand[:, 0].astype(int)] = True
        assert len(cand) > 50 and np.array_equal(sel, ref["outcome"] != SR.NOT_SELECTED)
    s = device_outputs(torch, 1, L.pitch * L.img_h)
    d_poses = torch.from_numpy(case["poses"]).cuda()
    torch.cuda.synchronize()
    ctx.sweep_depth_async([0], list(range(1, 1 + nv)), d_poses.data_ptr(), case["codes"], {k: v.data_ptr() for k, v in s.items()}, p)
    ctx.sync()
    got = fetch(capi, s, L)
    d = differs(result_of(got, 0), want_of(ref))
    assert d is None, (name, d)
    assert (got["pad"] == FILL).all()   # columns >= img_w are never written
    host = ctx.sweep_depth([0], [list(range(1, 1 + nv))], case["poses"], case["codes"], p)
    assert host["status"] == OK and result_of(host, 0) == result_of(got, 0)
    only = ctx.sweep_depth([0], [list(range(1, 1 + nv))], case["poses"], case["codes"], p, cost=False, outcome=False)   # the optional planes
    assert only["depth"].tobytes() == host["depth"].tobytes() and only["info"].tobytes() == host["info"].tobytes()
    ctx.close()


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------------
def batch_of_8(case):
    """eight different jobs over the case's three resident frames: the views in both orders, scaled poses, one view twice, and other
    frames in the reference's place"""
    p0, p1 = case["poses"]
    scaled = lambda f: [np.concatenate([p[:3] * f, p[3:4], p[4:] * f]) for p in (p0, p1)]   # (qw stays: the quaternion is used as given)
    jobs = [(0, (1, 2), [p0, p1]), (0, (2, 1), [p1, p0]), (0, (1, 2), scaled(1.1)), (0, (1, 2), scaled(1.2)), (0, (1, 1), [p0, p0]),
            (0, (2, 2), [p1, p1]), (1, (0, 2), [p0, p1]), (2, (1, 0), [p0, p1])]
    refs = [j[0] for j in jobs]
    views = [list(j[1]) for j in jobs]
    poses = np.stack([np.stack(j[2]) for j in jobs]).astype(np.float32)
    return refs, views, poses


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_views_64_refined", "odd_level1_32"])
def test_gpu_determinism_and_independence(capi, synth, name):
    case = DC.build(synth, name)
    ctx = make_ctx(capi, case)
    p = sweep_params(capi, case)
    refs, views, poses = batch_of_8(case)
    first = ctx.sweep_depth(refs, views, poses, case["codes"], p)
    assert first["status"] == OK
    want = [result_of(first, i) for i in range(8)]
    assert len({w["depth"] for w in want}) >= 5 and want[0]["info"][3] > 0   # the jobs differ, and the first one estimates
    again = ctx.sweep_depth(refs, views, poses, case["codes"], p)
    assert [result_of(again, i) for i in range(8)] == want
    rev = ctx.sweep_depth(refs[::-1], views[::-1], poses[::-1], case["codes"], p)
    assert [result_of(rev, 7 - i) for i in range(8)] == want
    for i in range(8):
        assert result_of(ctx.sweep_depth(refs[i:i + 1], views[i:i + 1], poses[i:i + 1], case["codes"], p), 0) == want[i], i
    other = dict(split=2, tail_update=2, first_poll=1, typed_loads=0, target_blocks=256)
    t0 = ctx.get_tuning()
    saved = {k: getattr(t0, k) for k in other}
    ctx.set_tuning(**other)
    tuned = ctx.sweep_depth(refs, views, poses, case["codes"], p)
    assert [result_of(tuned, i) for i in range(8)] == want
    ctx.set_tuning(**saved)
    ctx.close()


# ---- 3. refusals and the failed job --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals_leave_outputs_untouched(capi, synth, torch):
    case = DC.build(synth, "two_views_64_refined")
    ctx = make_ctx(capi, case, max_pairs=2)
    L = ctx.level_info(0)
    lib = capi.lib()
    s = device_outputs(torch, 2, L.pitch * L.img_h)
    d_poses = torch.from_numpy(np.concatenate([case["poses"], case["poses"]])).cuda()
    torch.cuda.synchronize()
    io = {k: v.data_ptr() for k, v in s.items()}
    codes = case["codes"]
    good = dict(case["params"])

    def call(ref=(0,), views=(1, 2), poses=None, codes=codes, io=io, n_views=2, n_hyp=None, **over):
        q = dict(good)
        q.update(over)
        reserved = q.pop("reserved", None)
        p = capi.default_sweep_params(n_views=n_views, n_hyp=len(codes) if n_hyp is None else n_hyp, **q)
        if reserved is not None:
            p.reserved[reserved] = 1
        ctx.sweep_depth_async(list(ref), list(views), d_poses.data_ptr() if poses is None else poses, codes, io, p)

    dup, down, zero, big = codes.copy(), codes.copy(), codes.copy(), codes.copy()
    dup[5] = dup[4]
    down[7], down[8] = codes[8], codes[7]
    zero[0] = 0
    big[-1] = 32768
    bad = [dict(ref=(3,)), dict(ref=(-1,)), dict(views=(1, 3)), dict(views=(-1, 2)), dict(ref=(), views=()),
           dict(ref=(0, 0, 0), views=(1, 2, 1, 2, 1, 2)), dict(lvl=-1), dict(lvl=DC.N_LEVELS), dict(source=2), dict(source=-1),
           dict(n_views=0, views=()), dict(n_views=5, views=(1, 2, 1, 2, 1)), dict(n_hyp=2), dict(n_hyp=65), dict(radius=0), dict(radius=3),
           dict(refine=2), dict(refine=-1), dict(uniq_num=0), dict(uniq_den=0), dict(max_mean_abs=0), dict(min_parallax=1),
           dict(reserved=0), dict(reserved=3), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(codes=dup),
           dict(codes=down), dict(codes=zero), dict(codes=big), dict(poses=0), dict(io=dict(io, depth=None)), dict(io=dict(io, info=None))]
    for kw in bad:
        with pytest.raises(capi.UwtError) as e:
            call(**kw)
        assert e.value.status == INVALID_ARG and lib.uwt_last_error(ctx._h), kw
    # null lists, codes, params and io: the raw entry point
    one, two = np.array([0], np.int32), np.array([1, 2], np.int32)
    p = capi.default_sweep_params(n_views=2, n_hyp=len(codes), **good)
    rec = capi.SweepIO(*[io[k] for k in ("depth", "cost", "outcome", "info")])
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    for a, b, cd, pp, r in ((None, two, codes, p, rec), (one, None, codes, p, rec), (one, two, None, p, rec), (one, two, codes, None, rec),
                            (one, two, codes, p, None)):
        st = lib.uwt_sweep_depth_batch_async(ctx._h, 1, ptr(a), ptr(b), C.c_void_p(d_poses.data_ptr()), ptr(cd),
                                             C.byref(pp) if pp is not None else None, C.byref(r) if r is not None else None)
        assert st == INVALID_ARG
    ctx.sync()
    assert all(bool((v == FILL).all()) for v in s.values())   # nothing was enqueued
    # the host form
    depth = np.full((1, L.img_h, L.img_w), 0x5A5A, np.uint16)
    info = np.full(1, FILL, np.uint8).repeat(64)
    for kw in (dict(lvl=DC.N_LEVELS), dict(radius=3), dict(min_parallax=0)):
        q = dict(good)
        q.update(kw)
        pp = capi.default_sweep_params(n_views=2, n_hyp=len(codes), **q)
        st = lib.uwt_sweep_depth_batch(ctx._h, 1, ptr(one), ptr(two), ptr(case["poses"]), ptr(codes), C.byref(pp), ptr(depth), None, None,
                                       ptr(info))
        assert st == INVALID_ARG and (depth == 0x5A5A).all() and (info == FILL).all(), kw
    for dd, ii in ((None, info), (depth, None)):
        assert lib.uwt_sweep_depth_batch(ctx._h, 1, ptr(one), ptr(two), ptr(case["poses"]), ptr(codes), C.byref(p), ptr(dd), None, None,
                                         ptr(ii)) == INVALID_ARG
    assert ctx.sweep_depth([0], [[1, 2]], case["poses"], codes, p)["status"] == OK   # the context still works
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_gpu_failed_job_leaves_its_neighbours_alone(capi, synth, bad):
    case = DC.build(synth, "two_views_64_refined")
    ctx = make_ctx(capi, case)
    p = sweep_params(capi, case)
    refs, views, poses = batch_of_8(case)
    clean = ctx.sweep_depth(refs, views, poses, case["codes"], p)
    broken = poses.copy()
    broken[2, 1, 5] = bad   # the second view of job 2
    with pytest.raises(capi.UwtError) as e:
        ctx.sweep_depth(refs, views, broken, case["codes"], p, raise_on_failure=True)
    assert e.value.status == PAIR_FAILED
    r = ctx.sweep_depth(refs, views, broken, case["codes"], p)
    assert r["status"] == PAIR_FAILED
    assert SR.info_tuple(r["info"][2]) == (INVALID_ARG,) + (0,) * 12
    assert not r["depth"][2].any() and not r["cost"][2].any() and not r["outcome"][2].any()
    for i in range(8):
        if i != 2:
            assert result_of(r, i) == result_of(clean, i), i
    ctx.close()


# ---- 4. guard bands ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_views_64_refined", "odd_level1_32"])
def test_gpu_guard_bands_hold_around_every_buffer(capi, synth, torch, name):
    """every device pointer of the call at exactly the alignment the header states, guards before and after each, and the guards
    inside the context's own work area (uwt_debug_guards): nothing is written outside the documented extents"""
    case = DC.build(synth, name)
    ctx = make_ctx(capi, case)
    ctx.debug_guards(4096)
    p = sweep_params(capi, case)
    L = ctx.level_info(p.lvl)
    refs, views, poses = batch_of_8(case)
    plane = L.pitch * L.img_h
    specs = [GB.Buf("poses", data=poses, align=4, stride=28), GB.Buf("depth", nbytes=8 * plane * 2, align=2, stride=plane * 2),
             GB.Buf("cost", nbytes=8 * plane * 2, align=2, stride=plane * 2), GB.Buf("outcome", nbytes=8 * plane, align=1, stride=plane),
             GB.Buf("info", nbytes=8 * 64, align=8, stride=64)]

    def call(a):
        ctx.sweep_depth_async(refs, [v for pair in views for v in pair], a.ptr("poses"), case["codes"],
                              {k: a.ptr(k) for k in ("depth", "cost", "outcome", "info")}, p)
        ctx.sync()

    outs = GB.run_twice(GB.TorchBackend(torch), specs, call)
    assert ctx.debug_check_guards() == (0, "")
    host = ctx.sweep_depth(refs, views, poses, case["codes"], p)
    assert ctx.debug_check_guards() == (0, "")
    ctx.debug_guards(0)
    plain = ctx.sweep_depth(refs, views, poses, case["codes"], p)   # results do not depend on the guards
    assert all(result_of(plain, i) == result_of(host, i) for i in range(8))
    d = np.frombuffer(outs["depth"], np.uint16).reshape(8, L.img_h, L.pitch)
    o = np.frombuffer(outs["outcome"], np.uint8).reshape(8, L.img_h, L.pitch)
    assert d[:, :, :L.img_w].tobytes() == host["depth"].tobytes() and o[:, :, :L.img_w].tobytes() == host["outcome"].tobytes()
    assert np.frombuffer(outs["info"], capi.SWEEP_INFO).tobytes() == host["info"].tobytes()
    assert (d[:, :, L.img_w:].view(np.uint8) == GB.OUT_FILL).all() and (o[:, :, L.img_w:] == GB.OUT_FILL).all()
    ctx.close()


# ---- 5. chained use and the consumers of the plane -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_chained_behind_a_seeded_tracking_call(capi, synth, torch):
    case = DC.build(synth, "two_views_64_refined")
    ctx = make_ctx(capi, case)
    p = sweep_params(capi, case)
    L = ctx.level_info(0)
    poses = torch.zeros((2, 7), dtype=torch.float32, device="cuda")
    stats = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    seeds = torch.from_numpy(case["poses"]).cuda()   # the alignment starts from the true poses
    s = device_outputs(torch, 1, L.pitch * L.img_h)
    ctx.track_batch_seeded_async(0, 3, [0, 0], [1, 2], poses.data_ptr(), stats.data_ptr(), d_seeds_ptr=seeds.data_ptr(), handoff="keep")
    ctx.sweep_depth_async([0], [1, 2], poses.data_ptr(), case["codes"], {k: v.data_ptr() for k, v in s.items()}, p)
    ctx.sync()   # the only wait
    got = fetch(capi, s, L)
    host_poses = poses.cpu().numpy()
    assert np.isfinite(host_poses).all() and not np.array_equal(host_poses, case["poses"])
    staged = ctx.sweep_depth([0], [[1, 2]], host_poses, case["codes"], p)   # the poses taken to the host and back
    assert result_of(got, 0) == result_of(staged, 0) and got["info"]["status"][0] == OK
    assert got["info"]["n_selected"][0] > 0
    ctx.close()


@pytest.mark.gpu
def test_gpu_plane_in_place_and_its_consumers(capi, synth, O, torch, arith):
    name = "two_views_64_refined"
    case = DC.build(synth, name)
    ref = DC.reference(O, arith, synth, name)
    ctx = make_ctx(capi, case, has_depth=1)
    p = sweep_params(capi, case)
    L = ctx.level_info(0)
    info = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    d_poses = torch.from_numpy(case["poses"]).cuda()
    torch.cuda.synchronize()
    ctx.sweep_depth_async([0], [1, 2], d_poses.data_ptr(), case["codes"],
                          dict(depth=ctx.plane_device_ptr(0, 0, capi.PLANE_DEPTH), info=info.data_ptr()), p)
    ctx.sync()
    assert SR.info_tuple(info.cpu().numpy().view(capi.SWEEP_INFO)[0]) == SR.info_tuple(ref["info"])
    assert ctx.get_plane(0, 0, capi.PLANE_DEPTH).tobytes() == ref["depth"].tobytes()   # the keyframe has its depth
    est = ref["outcome"] == SR.ESTIMATED
    n_est = int(est.sum())
    assert n_est > 500
    # the cloud with skip_invalid = 1 emits exactly the estimated pixels, at the depth written
    ident = np.array([[0, 0, 0, 1, 0, 0, 0]], np.float32)
    cloud = ctx.point_cloud_batch([0], ident, capi.default_cloud_params(mode=1, stride=1, skip_invalid=1))
    pts = cloud["points"]
    assert cloud["status"] == OK and len(pts) == n_est
    fx, fy, cx, cy = case["intr"]
    px = np.rint(pts["x"].astype(np.float64) / pts["z"] * fx + cx).astype(int)
    py = np.rint(pts["y"].astype(np.float64) / pts["z"] * fy + cy).astype(int)
    seen = np.zeros(est.shape, bool)
    seen[py, px] = True
    assert np.array_equal(seen, est)
    assert np.array_equal(pts["z"], SR.code_z(ref["depth"][py, px], 0, DC.DEPTH_SCALE))
    # the image warp under view 0's pose: every estimated pixel lands within 1 px of its winning hypothesis' landing in view 0
    valid = ctx.warp_image_batch([0], [1], case["poses"][:1], lvl=0)["valid"][0].astype(bool)
    wx, wy, xs, ys = ref["diag"]["winner_x2"]
    keep = wx >= 0
    assert int(keep.sum()) == n_est
    near = np.zeros(n_est, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yy, xx = np.clip(wy[keep] + dy, 0, L.img_h - 1), np.clip(wx[keep] + dx, 0, L.img_w - 1)
            near |= valid[yy, xx]
    assert near.all()
    # ... and only the estimated pixels' rows land at all
    assert ctx.warp_image_batch([0], [1], case["poses"][:1], lvl=0)["quality"]["n_landed"][0] <= n_est
    ctx.close()


# ---- 6. the mirrors and the tool -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_c_abi(capi, synth):
    tracker_mod = importlib.import_module("uw-slam_amd.tracker")
    case = DC.build(synth, "two_views_64_refined")
    w, h = case["size"]
    fx, fy, cx, cy = case["intr"]
    ctx = make_ctx(capi, case)
    tr = tracker_mod.Tracker(False, max_frames=4, n_levels=DC.N_LEVELS, first_level=DC.N_LEVELS - 1, last_level=0, depth_scale=DC.DEPTH_SCALE)
    tr.InitializePyramid(w, h, np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32))
    fr = [tracker_mod.Frame(f) for f in case["frames"]]
    for source in (0, 1):
        p = capi.default_sweep_params(n_views=2, n_hyp=len(case["codes"]), source=source, threshold=5.0)
        if source == 1:
            with pytest.raises(RuntimeError):
                tr.SweepDepth(fr[0], fr[1:], case["poses"], case["codes"], p)   # no gradients yet
            tr.ApplyGradient(fr[0])
        depth, cost, outcome, info = tr.SweepDepth(fr[0], fr[1:], case["poses"], case["codes"], p)
        want = ctx.sweep_depth([0], [[1, 2]], case["poses"], case["codes"], p)
        assert depth.tobytes() == want["depth"][0].tobytes() and cost.tobytes() == want["cost"][0].tobytes()
        assert outcome.tobytes() == want["outcome"][0].tobytes() and info.tobytes() == want["info"][0].tobytes()
        assert info["n_outcome"][capi.SWEEP_ESTIMATED] > 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.one_arith
def test_gpu_track_sequence_sweeps_keyframes_in_place(capi, synth):
    """tools/track_sequence.py --sweep-depth: each keyframe's plane, written in place, is the host form's over the same frames and poses"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "track_sequence.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    case = DC.build(synth, "two_views_64_refined")
    w, h = case["size"]
    frames = case["frames"] + case["frames"][::-1]            # frames 0..5: keyframes 0 and 3, two frames behind each
    poses = np.concatenate([case["poses"], case["poses"], case["poses"]])[:5]   # pair p: frame p + 1 against its keyframe
    keyframes = [tool.keyframe_of(i, 3) for i in range(1, 6)]
    assert keyframes == [0, 0, 0, 3, 3]
    planes, report = tool.sweep_keyframes(w, h, case["intr"], frames, poses, keyframes, 2, case["codes"])
    assert planes.shape == (2, h, w) and [r["keyframe"] for r in report] == [0, 3] and [r["views"] for r in report] == [[1, 2], [4, 5]]
    for k, (kf, views) in enumerate(((0, [1, 2]), (3, [4, 5]))):
        ctx = capi.Context(capi.default_params(w, h, *case["intr"], max_frames=3, max_pairs=1, has_depth=0, n_levels=2, first_level=1,
                                               last_level=0))
        ctx.upload_frames(0, np.stack([frames[kf]] + [frames[v] for v in views]))
        ctx.build_pyramids(0, 3)
        ctx.apply_gradient(0, 1)
        want = ctx.sweep_depth([0], [[1, 2]], poses[[v - 1 for v in views]], case["codes"])
        ctx.close()
        assert planes[k].tobytes() == want["depth"][0].tobytes()
        assert report[k]["outcomes"] == [int(v) for v in want["info"]["n_outcome"][0]]
        assert report[k]["coverage"] == want["info"]["n_outcome"][0][1] / float(w * h) and report[k]["n_selected"] == want["info"]["n_selected"][0]
    assert report[0]["coverage"] > 0.05
