"""ORB detection and description on the device (uwt_orb_*): key points compared AS INTEGERS (f32 fields as uint32, then octave and
laplacian), descriptors as bytes, layers, score maps and Harris measures as integers with the numpy restatement of the contract
(tests/orb_ref.py) — no tolerance anywhere.  The first test runs without a device: it checks that the inputs are worth testing on."""
import importlib

import numpy as np
import pytest

import match_ref as M
import orb_cases as K
import orb_ref as O
import ransac_ref as R

ARITH_INDEPENDENT = True   # ORB has no arithmetic set
INVALID_ARG, CAPACITY = 1, 5   # uwt_status_code (include/uwt.h)
INTR = {(160, 96): (131.25, 131.25, 79.5, 47.5), (97, 91): (80.0, 80.0, 48.0, 45.0), (256, 240): (210.0, 210.0, 127.5, 119.5)}
WHOLE = [(160, 96, "t3"), (97, 91, "t11"), (256, 240, "blobs")]
STAGES = [(160, 96, "t3"), (97, 91, "t11")]
LIVE_SEED = 5


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def make_ctx(capi, w, h, max_frames=2, **over):
    over.setdefault("n_levels", 1)
    over.setdefault("first_level", 0)
    over.setdefault("last_level", 0)
    return capi.Context(capi.default_params(w, h, *INTR[(w, h)], max_frames=max_frames, max_pairs=1, **over))


_ref = {}


def ref_of(name, img, cap=4096, pattern=None, **over):
    """the restatement's (key points, descriptors) of a named frame, computed once"""
    key = (name, cap, None if pattern is None else pattern.tobytes(), tuple(sorted(over.items())))
    if key not in _ref:
        p = O.default_params()
        p.update(over)
        _ref[key] = O.detect_describe(img, p, cap, pattern)
    return _ref[key]


def params_of(capi, **over):
    return capi.default_orb_params(**over) if over else None


def live_pair():
    synth = importlib.import_module("uw-slam_amd.synth")
    ref, tgt, _, _, _ = synth.render_pair(160, 96, *INTR[(160, 96)], seed=LIVE_SEED)
    return ref, tgt


def cpu_chain(ref, tgt):
    """the staged sequence from the restatement's key points and descriptors through match_ref and ransac_ref"""
    if "live" not in _ref:
        (k0, d0), (k1, d1) = O.detect_describe(ref), O.detect_describe(tgt)
        m, _, _ = M.match(d0, d1, 0.65)
        xy0, xy1 = np.stack([k0["x"], k0["y"]], 1), np.stack([k1["x"], k1["y"]], 1)
        _, good, _ = R.ransac(m, xy0, xy1)
        _ref["live"] = (k0, k1, m, xy0, xy1, good)
    return _ref["live"]


def test_inputs_are_worth_testing():
    """on the CPU: every whole-call input has key points on two layers at least (the blobs on five), the layers are the sizes the
    cases are chosen for, the mirrored texture holds a tie in H that a quota cuts through, and the live pair has 8 symmetric matches"""
    for w, h, name in WHOLE:
        k, _ = ref_of("%s_%dx%d" % (name, w, h), K.frame_of(name, w, h))
        layers = np.count_nonzero(np.bincount(k["octave"], minlength=8))
        assert layers >= (5 if name == "blobs" else 2), (name, np.bincount(k["octave"], minlength=8))
    assert [O.layer_size(160, 96, l)[1] for l in range(4)] == [96, 80, 67, 56]       # the fourth is below 2 * 31 + 1
    assert O.layer_size(97, 91, 2) == (67, 63) and O.layer_size(97, 91, 1)[0] == 81  # a one-pixel band; a partial last column
    img = K.mirrored_texture(160, 96, 3)
    nf = K.tie_cutting_features(img)
    assert nf is not None
    H = np.sort(O.layer_candidates(img, O.default_params())[2])[::-1]
    q = O.level_quota(nf, 8)[0]
    assert H[q - 1] == H[q]
    total = len(ref_of("m3_160x96", img)[0])
    assert total // 2 >= 8
    m = cpu_chain(*live_pair())[2]
    assert len(m) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,name", WHOLE)
def test_gpu_whole_call_equals_restatement(capi, w, h, name):
    img = K.frame_of(name, w, h)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, img[None])
    kp, desc = ctx.orb_detect_describe_batch([0])[0]
    wk, wd = ref_of("%s_%dx%d" % (name, w, h), img)
    per = np.bincount(wk["octave"], minlength=8)
    print(w, h, name, "key points", len(wk), "per layer", per)
    assert np.count_nonzero(per) >= (5 if name == "blobs" else 2)
    assert K.same_keypoints(kp, wk) is None, K.same_keypoints(kp, wk)
    assert K.same_descriptors(desc, wd) is None, K.same_descriptors(desc, wd)
    assert desc.dtype == np.uint8 and desc.shape == (len(wk), 32)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,name", STAGES)
def test_gpu_stages_equal_restatement(capi, w, h, name):
    img = K.frame_of(name, w, h)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, img[None])
    p = O.default_params()
    layers = [O.layer(img, l) for l in range(8)]
    for l in range(8):
        got = ctx.orb_layer(0, l)
        assert got.shape == layers[l].shape == O.layer_size(w, h, l)[::-1], l
        assert np.array_equal(got, layers[l]), (l, int((got != layers[l]).sum()))
    for l in (0, 2):
        got = ctx.orb_fast_scores(0, l)
        want = O.fast_scores(layers[l], p["edge_threshold"], p["fast_threshold"])
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), (l, int((got != want).sum()))
        assert np.count_nonzero(want) > 0
    for l in range(3):
        ys, xs, H = O.layer_candidates(layers[l], p)
        assert len(ys) > 0
        got = ctx.orb_harris(0, l, np.stack([xs, ys], 1))
        assert got.dtype == np.int64 and np.array_equal(got, H), l
    with pytest.raises(capi.UwtError) as e:
        ctx.orb_harris(0, 0, [[3, 10]])
    assert e.value.status == INVALID_ARG
    with pytest.raises(capi.UwtError) as e:
        ctx.orb_layer(0, 8)
    assert e.value.status == INVALID_ARG
    ctx.close()


@pytest.mark.gpu
def test_gpu_selection_quota_ties_and_capacity(capi):
    w, h = 160, 96
    img = K.mirrored_texture(w, h, 3)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, img[None])
    # every layer's quota cuts, and layer 0's falls between two corners of equal H: the (y, x) rule decides
    nf = K.tie_cutting_features(img)
    assert nf is not None
    wk, wd = ref_of("m3_160x96", img, n_features=nf)
    kp, desc = ctx.orb_detect_describe_batch([0], params=params_of(capi, n_features=nf))[0]
    quota = O.level_quota(nf, 8)
    per = np.bincount(wk["octave"], minlength=8)
    assert all(per[l] == quota[l] for l in range(8) if per[l]) and per[0] == quota[0] > 0
    assert K.same_keypoints(kp, wk) is None, K.same_keypoints(kp, wk)
    assert K.same_descriptors(desc, wd) is None, K.same_descriptors(desc, wd)
    # cap below the total: the cap strongest, in the order of the full list
    full = ref_of("m3_160x96", img)[0]
    cap = len(full) // 2
    wk, wd = ref_of("m3_160x96", img, cap=cap)
    kp, desc = ctx.orb_detect_describe_batch([0], cap=cap)[0]
    assert len(kp) == cap < len(full)
    assert K.same_keypoints(kp, wk) is None, K.same_keypoints(kp, wk)
    assert K.same_descriptors(desc, wd) is None, K.same_descriptors(desc, wd)
    order = {(int(k["octave"]), float(k["y"]), float(k["x"])): i for i, k in enumerate(full)}
    at = [order[(int(k["octave"]), float(k["y"]), float(k["x"]))] for k in kp]
    assert at == sorted(at) and min(kp["response"]) >= np.sort(full["response"])[::-1][cap - 1]
    ctx.close()


@pytest.mark.gpu
def test_gpu_describe_at_given_keypoints_and_its_errors(capi):
    w, h = 160, 96
    img = K.texture(w, h, 3)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, np.stack([img, K.texture(w, h, 4)]))
    wk, wd = ref_of("t3_160x96", img)
    det = ctx.orb_detect_describe_batch([0])[0]
    stripped = det[0].copy()
    stripped["dir_x"], stripped["dir_y"] = 0.25, -7.0       # the direction is recomputed, the other fields pass through
    got = ctx.orb_describe_batch([0, 1], [stripped, stripped[:0]])
    assert K.same_keypoints(got[0][0], wk) is None, K.same_keypoints(got[0][0], wk)
    assert K.same_descriptors(got[0][1], wd) is None, K.same_descriptors(got[0][1], wd)
    assert len(got[1][0]) == 0
    up = ctx.orb_describe_batch([0], [det[0]], params=params_of(capi, upright=1))[0]
    pu = O.default_params()
    pu["upright"] = 1
    uk, ud = O.describe(img, wk, pu)
    assert K.same_keypoints(up[0], uk) is None and K.same_descriptors(up[1], ud) is None
    assert (up[0]["dir_x"] == 1).all() and (up[0]["dir_y"] == 0).all()

    def one(**f):
        k = det[0][:2].copy()
        for name, v in f.items():
            k[name][1] = v
        return k

    s2 = float(np.float32(36.0 / 25.0))
    bad = [one(x=np.nan), one(y=np.inf), one(octave=-1), one(octave=8), one(x=30.0), one(x=float(w - 31)), one(y=30.0), one(y=float(h - 31)),
           one(octave=2, x=30.0 * s2, y=32.0 * s2), one(octave=3, x=60.0, y=50.0)]   # (layer 3 is 56 high: no band)
    for k in bad:
        out = (np.zeros((1, 2), capi.KEYPOINT), np.full((1, 2, 32), 0xA5, np.uint8))
        out[0].view(np.uint8)[:] = 0x5A
        with pytest.raises(capi.UwtError) as e:
            ctx.orb_describe_batch([0], [k], out=out)
        assert e.value.status == INVALID_ARG, k
        assert (out[0].view(np.uint8) == 0x5A).all() and (out[1] == 0xA5).all(), k
    with pytest.raises(capi.UwtError) as e:    # a record of layer 2 is outside a two-layer pyramid
        ctx.orb_describe_batch([0], [wk[wk["octave"] == 2][:1]], params=params_of(capi, n_levels=2))
    assert e.value.status == INVALID_ARG and (wk["octave"] == 2).any()
    # the borders themselves pass
    edge = one(x=31.0, y=float(h - 32))
    assert len(ctx.orb_describe_batch([0], [edge])[0][0]) == 2
    ctx.close()


@pytest.mark.gpu
def test_gpu_argument_errors_leave_outputs_untouched(capi):
    w, h, cap = 160, 96, 64
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, K.texture(w, h, 3)[None])
    bad = [(dict(slots=[2]), INVALID_ARG), (dict(slots=[-1]), INVALID_ARG),
           (dict(params=dict(n_features=0)), INVALID_ARG), (dict(params=dict(n_features=65537)), INVALID_ARG),
           (dict(params=dict(n_levels=0)), INVALID_ARG), (dict(params=dict(n_levels=9)), INVALID_ARG),
           (dict(params=dict(edge_threshold=15)), INVALID_ARG), (dict(params=dict(edge_threshold=1025)), INVALID_ARG),
           (dict(params=dict(fast_threshold=-1)), INVALID_ARG), (dict(params=dict(fast_threshold=256)), INVALID_ARG),
           (dict(cap=0), INVALID_ARG), (dict(cap=capi.UWT_MATCH_MAX_ROWS + 1), CAPACITY)]
    for kw, status in bad:
        c = kw.get("cap", cap)
        kp = np.zeros((1, min(max(c, 1), 64)), capi.KEYPOINT)
        kp.view(np.uint8)[:] = 0x5A
        out = (kp, np.full((1, kp.shape[1], 32), 0xA5, np.uint8), np.full(1, -9, np.int32))
        with pytest.raises(capi.UwtError) as e:
            ctx.orb_detect_describe_batch(kw.get("slots", [0]), params=capi.default_orb_params(**kw.get("params", {})), cap=c, out=out)
        assert e.value.status == status, (kw, e.value.status)
        assert (out[0].view(np.uint8) == 0x5A).all() and (out[1] == 0xA5).all() and out[2][0] == -9, kw
    # rows past the count stay as they are; the context still works
    kp = np.zeros((1, 256), capi.KEYPOINT)
    kp.view(np.uint8)[:] = 0x5A
    out = (kp, np.full((1, 256, 32), 0xA5, np.uint8), np.full(1, -9, np.int32))
    got = ctx.orb_detect_describe_batch([0], cap=256, out=out)[0]
    n = int(out[2][0])
    assert 0 < n == len(got[0]) < 256 and (kp[0, n:].view(np.uint8) == 0x5A).all() and (out[1][0, n:] == 0xA5).all()
    ctx.close()


@pytest.mark.gpu
def test_gpu_independent_of_batch_place_tuning_and_async(capi):
    import torch
    w, h, cap = 160, 96, 128
    a, b = K.texture(w, h, 3), K.texture(w, h, 4)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, np.stack([a, b]))
    wa, wb = ref_of("t3_160x96", a), ref_of("t4_160x96", b)
    assert 0 < len(wa[0]) <= cap and 0 < len(wb[0]) <= cap
    got = ctx.orb_detect_describe_batch([0, 1, 1, 0, 1], cap=cap)      # five frames over two slots
    for i, want in enumerate((wa, wb, wb, wa, wb)):
        assert K.same_keypoints(got[i][0], want[0]) is None and K.same_descriptors(got[i][1], want[1]) is None, i
    assert got[0][0].tobytes() == got[3][0].tobytes() and got[0][1].tobytes() == got[3][1].tobytes()
    assert got[1][0].tobytes() == got[4][0].tobytes() and got[1][1].tobytes() == got[4][1].tobytes()
    only = ctx.orb_detect_describe_batch([0], describe=False, cap=cap)[0]
    assert only[1] is None and K.same_keypoints(only[0], wa[0]) is None
    ctx.set_tuning(split=1, target_blocks=64, coarse=0)
    again = ctx.orb_detect_describe_batch([0, 1], cap=cap)
    assert again[0][0].tobytes() == got[0][0].tobytes() and again[0][1].tobytes() == got[0][1].tobytes()
    assert again[1][0].tobytes() == got[1][0].tobytes() and again[1][1].tobytes() == got[1][1].tobytes()
    d_kp = torch.zeros((2, cap, 8), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    ctx.orb_detect_describe_batch_async([0, 1], d_kp.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap=cap)
    ctx.sync()
    cnt = d_cnt.cpu().numpy()
    assert cnt.tolist() == [len(wa[0]), len(wb[0])]
    a_kp = d_kp.cpu().numpy().view(capi.KEYPOINT).reshape(2, cap)
    a_desc = d_desc.cpu().numpy()
    for f in range(2):
        assert a_kp[f, :cnt[f]].tobytes() == got[f][0].tobytes() and a_desc[f, :cnt[f]].tobytes() == got[f][1].tobytes(), f
    ctx.close()


@pytest.mark.gpu
def test_gpu_set_pattern(capi):
    w, h = 160, 96
    img = K.texture(w, h, 3)
    ctx = make_ctx(capi, w, h)
    ctx.upload_frames(0, img[None])
    wk, wd = ref_of("t3_160x96", img)
    second = K.second_pattern()
    assert O.pattern_ok(second) and second.tobytes() != O.default_pattern().tobytes()
    wk2, wd2 = ref_of("t3_160x96", img, pattern=second)
    assert wd2.tobytes() != wd.tobytes()
    ctx.orb_set_pattern(second)
    kp, desc = ctx.orb_detect_describe_batch([0])[0]
    assert K.same_keypoints(kp, wk) is None and K.same_keypoints(kp, wk2) is None     # the key points do not depend on the pattern
    assert K.same_descriptors(desc, wd2) is None, K.same_descriptors(desc, wd2)
    invalid = second.copy()
    invalid[200] = (0, 0, 11, 11)                                                    # 242 > 225
    with pytest.raises(capi.UwtError) as e:
        ctx.orb_set_pattern(invalid)
    assert e.value.status == INVALID_ARG
    assert K.same_descriptors(ctx.orb_detect_describe_batch([0])[0][1], wd2) is None   # refused: the table in force stays
    ctx.orb_set_pattern(None)
    assert K.same_descriptors(ctx.orb_detect_describe_batch([0])[0][1], wd) is None    # null restores the default
    ctx.close()


@pytest.mark.gpu
def test_gpu_staged_live_path(capi):
    """System::Tracking through the Python mirror with RobustMatcher(detector=1): the kept matches, n_matches_ and the pose equal
    the same stages driven by hand from the restatement's key points and descriptors"""
    T = importlib.import_module("uw-slam_amd.tracker")
    w, h = 160, 96
    intr = INTR[(w, h)]
    ref, tgt = live_pair()
    k0, k1, m, xy0, xy1, good = cpu_chain(ref, tgt)
    assert len(m) >= 8 and len(good) >= 8
    Kmat = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32)

    def frames(tracker):
        tracker.InitializePyramid(w, h, Kmat)
        return T.Frame(ref, None, 0), T.Frame(tgt, None, 1)

    tracker = T.Tracker(False, max_frames=2)
    prev, cur = frames(tracker)
    rm = T.RobustMatcher(tracker, detector=1)
    st = T.Tracking(tracker, rm, prev, cur)
    assert st["status"] == 0 and prev.n_matches_ == cur.n_matches_ == len(good)
    assert prev.keypoints_.tobytes() == xy0[good["query_idx"]].tobytes() and cur.keypoints_.tobytes() == xy1[good["train_idx"]].tobytes()
    assert K.same_keypoints(prev.orb_keypoints_, k0[good["query_idx"]]) is None
    assert K.same_keypoints(cur.orb_keypoints_, k1[good["train_idx"]]) is None
    assert len(prev.surf_keypoints_) == 0 and len(cur.surf_keypoints_) == 0
    # by hand: the restatement's kept key points into the existing features entry points of a fresh tracker
    hand = T.Tracker(False, max_frames=2)
    hp, hc = frames(hand)
    hand.ApplyGradient(hp)
    hand.ApplyGradient(hc)
    hp.keypoints_, hc.keypoints_ = xy0[good["query_idx"]], xy1[good["train_idx"]]
    hand.ObtainPatchesPoints(hp)
    hst = hand.EstimatePoseFeatures(hp, hc)
    assert hst["status"] == 0 and (hst["iterations"], hst["n_valid"]) == (st["iterations"], st["n_valid"])
    got, want = np.asarray(prev.rigid_transformation_, np.float32), np.asarray(hp.rigid_transformation_, np.float32)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (got, want)
    assert np.isfinite(got).all()
    # the next call describes the previous frame at the records it kept (it cannot gain matches) when asked to
    kept = len(prev.orb_keypoints_)
    again = rm.DetectAndTrackFeatures(prev, cur, True)
    assert 8 <= len(again) <= kept
    hand._ctx.close()
    tracker._ctx.close()
