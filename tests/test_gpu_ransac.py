"""RANSAC inlier selection on the device (uwt_ransac_inliers_batch, uwt_ransac_inliers_batch_async and the RobustMatcher::ransacTest
mirrors): mask, kept matches, count, best_hypothesis, hypotheses_run and the nine doubles of F compared AS INTEGERS with the
numpy restatement of the contract (tests/ransac_ref.py) — no tolerance anywhere."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ransac_cases as K
import ransac_ref as R

ARITH_INDEPENDENT = True   # the selection has no arithmetic set
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [0, 7, 8, 9, 63, 64, 65, 257, 2000, 4096]


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def small_ctx(capi, **over):
    return capi.Context(capi.default_params(160, 96, 131.25, 131.25, 79.5, 47.5, max_frames=2, max_pairs=1, **over))


def same_result(got, want):
    """(mask, good, info) of the device against the restatement's, every field as integers; returns a description of the first
    difference or None"""
    (gm, gg, gi), (wm, wg, wi) = got, want
    if gm.tobytes() != np.asarray(wm, np.uint8).tobytes():
        return "mask: %d against %d set" % (int(gm.sum()), int(wm.sum()))
    if gg.tobytes() != wg.tobytes():
        return "kept matches"
    for f in ("status", "n_inliers", "best_hypothesis", "hypotheses_run"):
        if int(gi[f]) != int(wi[f]):
            return "%s: %d against %d" % (f, int(gi[f]), int(wi[f]))
    if np.asarray(gi["F"]).view(np.uint64).tolist() != np.asarray(wi["F"]).view(np.uint64).tolist():
        return "F: %r against %r" % (gi["F"], wi["F"])
    return None


def run_ref(pair, **kw):
    return R.ransac(pair[0], pair[1], pair[2], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f[0] for f in K.FAMILIES])
def test_gpu_scene_families_equal_restatement(capi, family):
    scenes = [s[:3] for s in K.family_scenes(family)]
    ctx = small_ctx(capi)
    got = ctx.ransac_inliers_batch(scenes)
    for i, s in enumerate(scenes):
        want = run_ref(s)
        print(family, i, "inliers", int(want[2]["n_inliers"]), "best", int(want[2]["best_hypothesis"]), "run", int(want[2]["hypotheses_run"]))
        assert same_result(got[i], want) is None, (family, i, same_result(got[i], want))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", K.known_cases(), ids=[c[0] for c in K.known_cases()])
def test_gpu_known_cases(capi, case):
    name, m, k0, k1, truth, expect = case
    ctx = small_ctx(capi)
    got = ctx.ransac_inliers_batch([(m, k0, k1)])[0]
    assert same_result(got, run_ref((m, k0, k1))) is None, (name, same_result(got, run_ref((m, k0, k1))))
    mask, good, info = got
    if expect == "nothing":
        assert not mask.any() and len(good) == 0 and info["best_hypothesis"] == -1 and not np.any(info["F"]) and info["status"] == 0
    elif expect == "all_at_1":
        assert mask.all() and len(good) == len(m) and info["hypotheses_run"] == 1 and info["best_hypothesis"] == 0
    elif expect == "truth_kept":
        assert mask.astype(bool)[truth].all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEF])
def test_gpu_ragged_sizes_budgets_and_confidences(capi, seed):
    """N = 0 .. 4096 across the block and wave edges, hypothesis budgets across the round edges, adaptive and full runs"""
    pairs = [K.scene(300 + i, n, 0.3 if n >= 63 else 0.0, 0.3)[:3] for i, n in enumerate(RAGGED)]
    ctx = small_ctx(capi)
    for H in (1, 255, 256, 257, 1000):
        for conf in (0.5, 0.99, 1.0):
            par = capi.default_ransac_params(max_hypotheses=H, confidence=conf, seed=seed)
            got = ctx.ransac_inliers_batch(pairs, params=par, cap=4096)
            for i, pr in enumerate(pairs):
                want = run_ref(pr, max_hypotheses=H, confidence=conf, seed=seed)
                assert same_result(got[i], want) is None, (RAGGED[i], H, conf, same_result(got[i], want))
    ctx.close()


@pytest.mark.gpu
def test_gpu_pair_without_matches_beside_the_minimum_sample(capi):
    """A pair of 0 matches beside one of 8, the minimum sample, and the empty pair alone: then the batch has no row, no gather launch
    is made, and k_ransac still writes the pair's record"""
    empty, eight = K.scene(800, 0, 0.0, 0.2)[:3], K.scene(6, 8, 0.0, 0.2)[:3]
    ctx = small_ctx(capi)
    for pairs in ([empty, eight], [empty]):
        got = ctx.ransac_inliers_batch(pairs)
        for i, pr in enumerate(pairs):
            assert same_result(got[i], run_ref(pr)) is None, (len(pairs), i, same_result(got[i], run_ref(pr)))
        mask, good, info = got[0]
        assert len(mask) == 0 and len(good) == 0 and info["status"] == 0 and info["best_hypothesis"] == -1 and not np.any(info["F"])
    ctx.close()


def mixed_pairs(count=64, seed=5):
    """pairs of mixed sizes: empty, below the sample size, around the wave and block edges, a large one; some with outliers"""
    rng = np.random.default_rng(seed)
    sizes = [0, 7, 8, 64, 257, 1500] + [int(rng.integers(8, 400)) for _ in range(count - 6)]
    order = rng.permutation(count)
    return [K.scene(500 + i, sizes[i], 0.3 if sizes[i] >= 30 else 0.0, 0.3, motion=("general", "x", "none")[i % 3])[:3] for i in order]


@pytest.mark.gpu
def test_gpu_batch_independence_and_async(capi):
    """64 pairs of mixed sizes: the batch, the pairs one per call, the batch reversed, a second context whose scratch a different
    call has used before, and the asynchronous form (matches in, results out: device memory) give the same integers"""
    import torch
    pairs = mixed_pairs()
    P = len(pairs)
    ctx = small_ctx(capi)
    batch = ctx.ransac_inliers_batch(pairs, cap=1536, kp_cap=1536)
    for i in (0, 9, 33, 63):   # anchored to the restatement
        assert same_result(batch[i], run_ref(pairs[i])) is None, i
    assert sum(len(b[1]) for b in batch) > 0 and any(0 < len(b[1]) < len(p[0]) for b, p in zip(batch, pairs))
    for i, pr in enumerate(pairs):
        assert same_result(ctx.ransac_inliers_batch([pr])[0], batch[i]) is None, i       # cap = the pair's own size
    rev = ctx.ransac_inliers_batch(pairs[::-1], cap=1600)
    assert all(same_result(rev[P - 1 - i], batch[i]) is None for i in range(P))
    ctx2 = small_ctx(capi)
    synth = importlib.import_module("uw-slam_amd.synth")
    ctx2.match_descriptors_batch([synth.descriptor_pair(3, 300, 280, 64, "l2")[:2]])
    ctx2.ransac_inliers_batch(pairs[:2], params=capi.default_ransac_params(confidence=0.5, max_hypotheses=300))   # other need(k) rows
    after = ctx2.ransac_inliers_batch(pairs[5:20])
    assert all(same_result(after[i], batch[5 + i]) is None for i in range(15))
    ctx2.close()
    # asynchronous: the matches and their counts in device memory, in the layout the matching call leaves them
    cap, kp_cap, mt, nm, *_ = capi.Context._ransac_block(pairs, 1536, 1536)
    d_m = torch.from_numpy(mt.view(np.int32).reshape(P, cap, 3)).cuda()
    d_n = torch.from_numpy(nm).cuda()
    d_mask = torch.full((P, cap), 0x5A, dtype=torch.uint8, device="cuda")
    d_good = torch.full((P, cap, 3), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    d_info = torch.full((P, 11), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # torch's copies and fills run on torch's stream, not on the context's
    assert ctx.ransac_inliers_batch_async(d_m.data_ptr(), d_n.data_ptr(), cap, [p[1:] for p in pairs], d_mask.data_ptr(), d_good.data_ptr(),
                                          d_cnt.data_ptr(), d_info.data_ptr(), kp_cap=kp_cap) == kp_cap
    ctx.sync()
    mask, good, cnt = d_mask.cpu().numpy(), d_good.cpu().numpy(), d_cnt.cpu().numpy()
    info = np.frombuffer(d_info.cpu().numpy().tobytes(), capi.RANSAC_INFO)
    for i in range(P):
        got = (mask[i, :nm[i]], np.frombuffer(good[i, :cnt[i]].tobytes(), capi.MATCH), info[i])
        assert same_result(got, batch[i]) is None, (i, same_result(got, batch[i]))
        assert np.all(mask[i, nm[i]:] == 0x5A) and np.all(good[i, cnt[i]:] == -7)   # nothing written past the counts
    # an index outside its key-point count in device matches fails that pair alone
    mt2 = mt.copy()
    victim = next(i for i in range(P) if nm[i] > 100)
    mt2[victim, 17]["train_idx"] = len(pairs[victim][2])
    d_m2 = torch.from_numpy(mt2.view(np.int32).reshape(P, cap, 3)).cuda()
    torch.cuda.synchronize()
    ctx.ransac_inliers_batch_async(d_m2.data_ptr(), d_n.data_ptr(), cap, [p[1:] for p in pairs], d_mask.data_ptr(), d_good.data_ptr(),
                                   d_cnt.data_ptr(), d_info.data_ptr(), kp_cap=kp_cap)
    ctx.sync()
    mask, good, cnt = d_mask.cpu().numpy(), d_good.cpu().numpy(), d_cnt.cpu().numpy()
    info = np.frombuffer(d_info.cpu().numpy().tobytes(), capi.RANSAC_INFO)
    for i in range(P):
        if i == victim:
            assert info[i]["status"] == capi.ERR_INVALID_ARG and cnt[i] == 0 and info[i]["n_inliers"] == 0 and info[i]["best_hypothesis"] == -1
            assert not mask[i, :nm[i]].any() and not np.any(info[i]["F"])
        else:
            got = (mask[i, :nm[i]], np.frombuffer(good[i, :cnt[i]].tobytes(), capi.MATCH), info[i])
            assert same_result(got, batch[i]) is None, i
    ctx.close()


@pytest.mark.gpu
def test_gpu_growth_under_a_queued_async_call(capi):
    """A small asynchronous call is still queued when a synchronous call of the same context needs the stage's buffer larger:
    both give, as bytes, what the same two calls give on fresh contexts."""
    import torch
    small = K.scene(700, 24, 0.0, 0.3)[:3]
    large = mixed_pairs()[:4]
    cap, kp_cap, mt, nm, *_ = capi.Context._ransac_block([small], 32, 32)

    def run(ctx_small, ctx_large):
        d_m = torch.from_numpy(mt.view(np.int32).reshape(1, cap, 3)).cuda()
        d_n = torch.from_numpy(nm).cuda()
        d_mask = torch.full((1, cap), 0x5A, dtype=torch.uint8, device="cuda")
        d_good = torch.full((1, cap, 3), -7, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        d_info = torch.full((1, 11), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()   # torch's copies and fills run on torch's stream, not on the context's
        ctx_small.ransac_inliers_batch_async(d_m.data_ptr(), d_n.data_ptr(), cap, [small[1:]], d_mask.data_ptr(), d_good.data_ptr(),
                                             d_cnt.data_ptr(), d_info.data_ptr(), kp_cap=kp_cap)
        big = ctx_large.ransac_inliers_batch(large, cap=1536, kp_cap=1536)     # no sync in between
        ctx_small.sync()
        first = b"".join(t.cpu().numpy().tobytes() for t in (d_cnt, d_mask, d_good, d_info))
        return first, [m.tobytes() + g.tobytes() + i.tobytes() for m, g, i in big], int(d_cnt.cpu()[0])

    ctx = small_ctx(capi)
    got = run(ctx, ctx)
    ctx.close()
    a, b = small_ctx(capi), small_ctx(capi)
    want = run(a, b)
    a.close()
    b.close()
    assert got[2] >= 8   # the small call kept a model's inliers
    assert got[0] == want[0] and got[1] == want[1]


@pytest.mark.gpu
def test_gpu_argument_errors_leave_the_outputs_untouched(capi):
    import ctypes as C
    ctx = small_ctx(capi)
    m, k0, k1, _ = K.scene(1, 40, 0.2, 0.3)
    cap, kp_cap, mt, nm, a, n0, b, n1 = capi.Context._ransac_block([(m, k0, k1)], 48, 48)
    INV, CAPACITY = capi.ERR_INVALID_ARG, capi.ERR_CAPACITY
    par = capi.default_ransac_params

    def call(n_pairs=1, mt=mt, nm=nm, cap=cap, a=a, n0=n0, b=b, n1=n1, kp_cap=kp_cap, params=None, null_out=None):
        out = dict(mask=np.full(64, 0x5A, np.uint8), good=np.full(3 * 48, 0x5A5A5A5A, np.uint32),
                   cnt=np.full(1, 0x5A5A5A5A, np.uint32), info=np.full(22, 0x5A5A5A5A, np.uint32))
        ptr = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None
        o = {k: (None if k == null_out else v) for k, v in out.items()}
        st = capi.lib().uwt_ransac_inliers_batch(ctx._h, n_pairs, ptr(mt), ptr(nm), cap, ptr(a), ptr(n0), ptr(b), ptr(n1), kp_cap,
                                                 C.byref(params) if params is not None else None, ptr(o["mask"]), ptr(o["good"]),
                                                 ptr(o["cnt"]), ptr(o["info"]))
        untouched = all(np.all(v == (0x5A if v.dtype == np.uint8 else 0x5A5A5A5A)) for v in out.values())
        return st, untouched

    i32 = lambda v: np.array([v], np.int32)
    bad_q, bad_t = mt.copy(), mt.copy()
    bad_q[0, 3]["query_idx"] = 40
    bad_t[0, 39]["train_idx"] = -1
    rows = [
        (INV, dict(n_pairs=0)), (INV, dict(mt=None)), (INV, dict(nm=None)), (INV, dict(a=None)), (INV, dict(n0=None)), (INV, dict(b=None)),
        (INV, dict(n1=None)), (INV, dict(cap=0)), (INV, dict(kp_cap=0)), (INV, dict(nm=i32(49))), (INV, dict(nm=i32(-1))),
        (INV, dict(n0=i32(49))), (INV, dict(n1=i32(-1))), (INV, dict(mt=bad_q)), (INV, dict(mt=bad_t)),
        (INV, dict(n0=i32(39))),   # a match now points past the key points of the previous frame
        (INV, dict(params=par(distance=float("nan")))), (INV, dict(params=par(distance=-1.0))), (INV, dict(params=par(confidence=0.0))),
        (INV, dict(params=par(confidence=1.5))), (INV, dict(params=par(max_hypotheses=0))),
        (INV, dict(params=par(max_hypotheses=capi.RANSAC_MAX_HYPOTHESES + 1))),
        (INV, dict(null_out="mask")), (INV, dict(null_out="good")), (INV, dict(null_out="cnt")), (INV, dict(null_out="info")),
        (CAPACITY, dict(cap=capi.MATCH_MAX_ROWS + 1)), (CAPACITY, dict(kp_cap=capi.MATCH_MAX_ROWS + 1)),
    ]
    for k, (want, kw) in enumerate(rows):
        st, untouched = call(**kw)
        assert st == want and untouched, (k, kw.keys(), st, want, untouched)
    st, untouched = call()
    assert st == 0 and not untouched
    assert same_result(ctx.ransac_inliers_batch([(m, k0, k1)], params=par(max_hypotheses=capi.RANSAC_MAX_HYPOTHESES, confidence=0.999))[0],
                       run_ref((m, k0, k1), max_hypotheses=capi.RANSAC_MAX_HYPOTHESES, confidence=0.999)) is None   # the limit itself
    ctx.close()


def descriptor_scene(synth, seed, n=400, m=380):
    """descriptor sets with known correspondences whose key points follow a two-view geometry; the generator's other rows are
    unrelated points, so wrong matches — if the matcher lets any through — are outliers"""
    A, B, dst, src = synth.descriptor_pair(seed, n, m, 64, "l2")
    mt, p0, p1, _ = K.scene(seed + 1, len(src), 0.25, 0.3)
    rng = np.random.default_rng(seed + 2)
    kpa = rng.uniform([6, 6], [K.W - 7, K.H - 7], (n, 2)).astype(np.float32)
    kpb = rng.uniform([6, 6], [K.W - 7, K.H - 7], (m, 2)).astype(np.float32)
    kpa[src] = p0                      # row src[i] of A is point i of the scene,
    kpb[dst] = p1[mt["train_idx"]]     # row dst[i] of B its partner (scene() shuffles the second frame: undone through its matches)
    return A, B, kpa, kpb


@pytest.mark.gpu
def test_gpu_python_mirror_runs_the_reference_sequence(capi):
    """match -> ransacTest -> SetKeypoints through the Python mirror = the C ABI entries one after the other = the restatements"""
    import match_ref
    tracker = importlib.import_module("uw-slam_amd.tracker")
    synth = importlib.import_module("uw-slam_amd.synth")
    A, B, kpa, kpb = descriptor_scene(synth, 900)
    ctx = small_ctx(capi)
    rm = tracker.RobustMatcher(ctx)
    assert (rm.distance_, rm.confidence_, rm.refineF_) == (3.0, 0.99, True)   # include/Tracker.h:81-83
    sym = match_ref.match(A, B, rm.ratio_)[0]
    want = run_ref((sym, kpa, kpb))
    assert 8 < len(want[1]) < len(sym)   # RANSAC removes something
    out = []
    good, mask, info = rm.ransacTest(sym, kpa, kpb, out)
    assert same_result((mask, good, info), want) is None and len(out) == len(good)
    prev, cur = tracker.Frame(np.zeros((4, 4), np.uint8)), tracker.Frame(np.zeros((4, 4), np.uint8))
    kept = rm.DetectAndTrackFeatures(prev, cur, A, B, (kpa, kpb))
    assert kept.tobytes() == want[1].tobytes() and prev.n_matches_ == cur.n_matches_ == len(kept)
    assert np.array_equal(prev.keypoints_, kpa[kept["query_idx"]]) and np.array_equal(cur.keypoints_, kpb[kept["train_idx"]])
    ctx.close()


@pytest.mark.gpu
def test_gpu_cpp_mirror_runs_the_reference_sequence(capi, tmp_path):
    import match_ref
    synth = importlib.import_module("uw-slam_amd.synth")
    exe = str(tmp_path / "shim_ransac")
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_ransac.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pairs = [K.scene(700 + i, n, 0.3 if n > 20 else 0.0, 0.3)[:3] for i, n in enumerate((200, 7, 8, 640))]
    with open(tmp_path / "pairs.bin", "wb") as f:
        for m, a, b in pairs:
            f.write(np.array([len(m), len(a), len(b)], np.int32).tobytes() + m.tobytes() + a.tobytes() + b.tobytes())
    r = subprocess.run([exe, "ransac", str(tmp_path / "pairs.bin"), str(len(pairs))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    ctx = small_ctx(capi)
    got = ctx.ransac_inliers_batch(pairs)
    for i, (mask, good, info) in enumerate(got):
        tok = [l for l in r.stdout.split("\n") if l.startswith("RANSAC %d " % i)][0].split()
        assert [int(v) for v in tok[2:6]] == [len(good), info["best_hypothesis"], info["hypotheses_run"], info["status"]]
        assert [int(v, 16) for v in tok[6:15]] == np.asarray(info["F"]).view(np.uint64).tolist()
        assert tok[15] == ("".join(str(int(v)) for v in mask) or "-")
    scenes = [descriptor_scene(synth, 950 + 10 * i, n=300 + 40 * i, m=320) for i in range(2)]
    with open(tmp_path / "desc.bin", "wb") as f:
        for A, B, kpa, kpb in scenes:
            f.write(np.array([len(A), len(B), A.shape[1]], np.int32).tobytes() + A.tobytes() + B.tobytes() + kpa.tobytes() + kpb.tobytes())
    r = subprocess.run([exe, "detect", str(tmp_path / "desc.bin"), "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    for i, (A, B, kpa, kpb) in enumerate(scenes):
        sym = ctx.match_descriptors_batch([(A, B)])[0]
        good = ctx.ransac_inliers_batch([(sym, kpa, kpb)])[0][1]
        tok = [l for l in r.stdout.split("\n") if l.startswith("DETECT %d " % i)][0].split()
        assert int(tok[2]) == len(good) and tok[3:] == ["%d:%d" % (g["query_idx"], g["train_idx"]) for g in good]
        assert 8 < len(good) < len(sym)
    ctx.close()
