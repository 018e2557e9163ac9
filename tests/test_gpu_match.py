"""Descriptor matching on the device (uwt_knn_match_batch, uwt_match_descriptors_batch, uwt_match_descriptors_batch_async and the
RobustMatcher mirrors): every record compared as integers with the numpy restatement of the contract (tests/match_ref.py)."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases
import match_ref as R

ARITH_INDEPENDENT = True   # matching has no arithmetic set
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2000, 2000), (1500, 1400), (500, 480), (1, 2), (2, 1), (3, 257), (65, 63), (0, 5), (5, 0), (5, 1)]
KINDS = {"l2_64": (64, "l2"), "l2_128": (128, "l2"), "hamming_32": (32, "hamming")}
VGA = (640, 480, (525.0, 525.0, 319.5, 239.5))


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("uw-slam_amd.synth")


def small_ctx(capi, **over):
    return capi.Context(capi.default_params(160, 96, 131.25, 131.25, 79.5, 47.5, max_frames=2, max_pairs=1, **over))


def same(a, b):
    """record arrays equal as integers (the float fields bit for bit)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_sized = {}


def sized_pairs(synth, kind):
    if kind not in _sized:
        dim, k = KINDS[kind]
        _sized[kind] = [synth.descriptor_pair(7 + i, n, m, dim, k)[:2] for i, (n, m) in enumerate(SIZES)]
    return _sized[kind]


_want = {}


def wanted(kind, i, a, b, ratio=0.65):
    if (kind, i) not in _want:
        _want[(kind, i)] = R.match(a, b, ratio)
    return _want[(kind, i)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_knn_match_equals_restatement(capi, synth, kind):
    """idx0, idx1, d0, d1 of every query row at every size, full-size and ragged ones that cross every tile edge"""
    pairs = sized_pairs(synth, kind)
    ctx = small_ctx(capi)
    got = ctx.knn_match_batch(pairs, cap=2048)
    for i, (a, b) in enumerate(pairs):
        _, fwd, _ = wanted(kind, i, a, b)
        assert len(got[i]) == len(a)
        bad = np.nonzero(got[i].view(np.uint32).reshape(-1, 4) != fwd.view(np.uint32).reshape(-1, 4))[0]
        assert bad.size == 0, (SIZES[i], bad[:5], got[i][bad[:5]], fwd[bad[:5]])
    assert list(got[9]["idx1"]) == [-1] * 5 and np.all(got[9]["idx0"] == 0)   # 5 x 1: idx0 / d0 reported, no second
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_match_descriptors_equals_restatement(capi, synth, kind):
    """counts and every (query_idx, train_idx, distance)"""
    pairs = sized_pairs(synth, kind)
    ctx = small_ctx(capi)
    got = ctx.match_descriptors_batch(pairs, ratio=0.65, cap=2048)
    for i, (a, b) in enumerate(pairs):
        want, _, _ = wanted(kind, i, a, b)
        print(kind, SIZES[i], "matches", len(want))
        assert len(got[i]) == len(want), (SIZES[i], len(got[i]), len(want))
        assert same(got[i], want), SIZES[i]
    assert len(got[0]) > 0 and all(len(got[i]) == 0 for i in (4, 7, 8, 9))   # n < 2 or m < 2: no match, no error
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", match_cases.CASES, ids=[c[0] for c in match_cases.CASES])
def test_gpu_constructed_cases(capi, case):
    _, A, B, ratio, want_fwd, want = case
    ctx = small_ctx(capi)
    assert same(ctx.knn_match_batch([(A, B)])[0], np.array(want_fwd, R.KNN2))
    assert same(ctx.match_descriptors_batch([(A, B)], ratio=ratio)[0], np.array(want, R.MATCH))
    ctx.close()


def mixed_batch(synth, seed, count=64):
    """pairs of mixed sizes, both norms apart; both empty kinds and single rows among them"""
    rng = np.random.default_rng(seed)
    shapes = [(0, 40), (40, 0), (1, 30), (30, 1)] + [(int(rng.integers(2, 300)), int(rng.integers(2, 300))) for _ in range(count - 4)]
    order = rng.permutation(count)
    return [shapes[i] for i in order]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l2_64", "hamming_32"])
def test_gpu_batch_independence_and_async(capi, synth, kind):
    """64 pairs of mixed sizes: the batch, the same pairs one per call, the batch reversed and the asynchronous form give the same
    records bit for bit; a second context that sees a small call first and a large one after (scratch reuse, then growth) too"""
    import torch
    dim, k = KINDS[kind]
    shapes = mixed_batch(synth, 5)
    pairs = [synth.descriptor_pair(100 + i, n, m, dim, k)[:2] for i, (n, m) in enumerate(shapes)]
    ctx = small_ctx(capi)
    batch = ctx.match_descriptors_batch(pairs, cap=320)
    knn = ctx.knn_match_batch(pairs, cap=320)
    for i in (5, 17, 40):   # anchored to the restatement
        want, fwd, _ = R.match(*pairs[i])
        assert same(batch[i], want) and same(knn[i], fwd)
    assert sum(len(b) for b in batch) > 0
    for i, pr in enumerate(pairs):
        assert same(ctx.match_descriptors_batch([pr])[0], batch[i]), i      # cap = the pair's own largest count
        assert same(ctx.knn_match_batch([pr])[0], knn[i]), i
    rev = ctx.match_descriptors_batch(pairs[::-1], cap=300)
    assert all(same(rev[len(pairs) - 1 - i], batch[i]) for i in range(len(pairs)))
    # asynchronous, results in device memory
    P, cap = len(pairs), 320
    d_m = torch.full((P, cap, 3), -7, dtype=torch.int32, device="cuda")
    d_c = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    assert ctx.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), pairs, cap=cap) == cap
    ctx.sync()
    cnt, rec = d_c.cpu().numpy(), d_m.cpu().numpy()
    for i in range(P):
        assert cnt[i] == len(batch[i]) and same(np.frombuffer(rec[i, :cnt[i]].tobytes(), capi.MATCH), batch[i]), i
        assert np.all(rec[i, cnt[i]:] == -7)   # nothing written past the count
    ctx.close()
    ctx2 = small_ctx(capi)
    assert same(ctx2.match_descriptors_batch(pairs[:1])[0], batch[0])
    big = ctx2.match_descriptors_batch(pairs, cap=512)
    small = ctx2.match_descriptors_batch(pairs[3:9])
    assert all(same(big[i], batch[i]) for i in range(P)) and all(same(small[i], batch[3 + i]) for i in range(6))
    ctx2.close()


@pytest.mark.gpu
def test_gpu_growth_under_a_queued_async_call(capi, synth):
    """A small asynchronous call is still queued when a synchronous call of the same context needs every buffer of the stage
    larger: both give, as bytes, what the same two calls give on fresh contexts."""
    import torch
    small = [synth.descriptor_pair(900, 40, 40, 64, "l2")[:2]]
    large = [synth.descriptor_pair(901 + i, 300, 280, 64, "l2")[:2] for i in range(4)]

    def run(ctx_small, ctx_large):
        d_m = torch.full((1, 64, 3), -7, dtype=torch.int32, device="cuda")
        d_c = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
        ctx_small.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), small, cap=64)
        big = ctx_large.match_descriptors_batch(large, cap=512)     # no sync in between
        ctx_small.sync()
        return d_c.cpu().numpy().tobytes() + d_m.cpu().numpy().tobytes(), [b.tobytes() for b in big]

    ctx = small_ctx(capi)
    got = run(ctx, ctx)
    ctx.close()
    a, b = small_ctx(capi), small_ctx(capi)
    want = run(a, b)
    a.close()
    b.close()
    assert np.frombuffer(got[0][:4], np.int32)[0] > 0 and sum(len(x) for x in got[1]) > 0
    assert got[0] == want[0] and got[1] == want[1]


def raw_call(capi, ctx, name, n_pairs, norm, dim, q, nq, t, nt, cap, ratio, out, cnt):
    def ptr(a):
        return C.c_void_p(a.ctypes.data) if a is not None else None
    fn = getattr(capi.lib(), name)
    if name == "uwt_knn_match_batch":
        return fn(ctx._h, n_pairs, norm, dim, ptr(q), ptr(nq), ptr(t), ptr(nt), cap, ptr(out))
    return fn(ctx._h, n_pairs, norm, dim, ptr(q), ptr(nq), ptr(t), ptr(nt), cap, C.c_float(ratio), ptr(out), ptr(cnt))


@pytest.mark.gpu
def test_gpu_argument_errors_leave_the_outputs_untouched(capi):
    ctx = small_ctx(capi)
    cap, dim = 8, 8
    q, t = np.zeros((1, cap, dim), np.float32), np.ones((1, cap, dim), np.float32)
    nq, nt = np.array([4], np.int32), np.array([5], np.int32)
    L2, HAM, INV, CAPACITY = capi.NORM_L2, capi.NORM_HAMMING, capi.ERR_INVALID_ARG, capi.ERR_CAPACITY
    big = capi.MATCH_MAX_ROWS + 1
    bad = [  # (expected, n_pairs, norm, dim, q, nq, t, nt, cap, ratio)
        (INV, 0, L2, dim, q, nq, t, nt, cap, 0.65),
        (INV, 1, L2, dim, None, nq, t, nt, cap, 0.65), (INV, 1, L2, dim, q, None, t, nt, cap, 0.65),
        (INV, 1, L2, dim, q, nq, None, nt, cap, 0.65), (INV, 1, L2, dim, q, nq, t, None, cap, 0.65),
        (INV, 1, L2, dim, q, np.array([cap + 1], np.int32), t, nt, cap, 0.65), (INV, 1, L2, dim, q, nq, t, np.array([-1], np.int32), cap, 0.65),
        (INV, 1, L2, 0, q, nq, t, nt, cap, 0.65), (INV, 1, L2, 6, q, nq, t, nt, cap, 0.65), (INV, 1, HAM, 6, q, nq, t, nt, cap, 0.65),
        (INV, 1, 2, dim, q, nq, t, nt, cap, 0.65), (INV, 1, -1, dim, q, nq, t, nt, cap, 0.65),
        (CAPACITY, 1, L2, dim, q, nq, t, nt, big, 0.65), (CAPACITY, 1, L2, 132, q, nq, t, nt, cap, 0.65),
        (CAPACITY, 1, HAM, capi.MATCH_MAX_ROW_BYTES + 4, q, nq, t, nt, cap, 0.65),
    ]
    for name in ("uwt_knn_match_batch", "uwt_match_descriptors_batch"):
        rows = bad + ([(INV, 1, L2, dim, q, nq, t, nt, cap, float("nan")), (INV, 1, L2, dim, q, nq, t, nt, cap, float("inf"))]
                      if name != "uwt_knn_match_batch" else [])
        for k, (want, n_pairs, norm, d, qq, nqq, tt, ntt, cp, ratio) in enumerate(rows):
            out = np.full(cap * 4, 0x5A5A5A5A, np.uint32)
            cnt = np.full(1, 0x5A5A5A5A, np.uint32)
            st = raw_call(capi, ctx, name, n_pairs, norm, d, qq, nqq, tt, ntt, cp, ratio, out, cnt)
            assert st == want, (name, k, st, want)
            assert np.all(out == 0x5A5A5A5A) and cnt[0] == 0x5A5A5A5A, (name, k)
    # the limits themselves are accepted: a row of UWT_MATCH_MAX_ROW_BYTES
    wide = np.zeros((1, 4, capi.MATCH_MAX_ROW_BYTES), np.uint8)
    wide[0, 1, 3] = 0xF0
    got = ctx.knn_match_batch(packed=(wide, np.array([2], np.int32), wide, np.array([2], np.int32)))
    assert list(got[0]["idx0"]) == [0, 1] and list(got[0]["d1"]) == [4.0, 4.0]
    ctx.close()


@pytest.mark.gpu
def test_gpu_every_count_zero_runs_the_filter_alone(capi):
    """Two pairs, dim 64, cap 8, every count 0: the batch has no row, so no k_knn2 launch is made (its grid would be empty) and
    k_match_filter still runs.  The synchronous call delivers counts 0 and no match row; the asynchronous one, whose rows the test
    reads in device memory, writes counts 0 and leaves every row as it was — though the rows behind the counts are equal sets"""
    import torch
    ctx = small_ctx(capi)
    P, cap, dim = 2, 8, 64
    rows = np.random.default_rng(21).normal(size=(P, cap, dim)).astype(np.float32)
    none = np.zeros(P, np.int32)
    out = np.full(P * cap * 3, 0x5A5A5A5A, np.uint32)
    cnt = np.full(P, 0x5A5A5A5A, np.uint32)
    assert raw_call(capi, ctx, "uwt_match_descriptors_batch", P, capi.NORM_L2, dim, rows, none, rows, none, cap, 0.65, out, cnt) == 0
    assert cnt.tolist() == [0, 0] and np.all(out == 0x5A5A5A5A)
    d_m = torch.full((P, cap, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_c = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # torch's fill kernels run on torch's stream, not on the context's
    assert ctx.match_descriptors_batch_async(d_m.data_ptr(), d_c.data_ptr(), packed=(rows, none, rows, none)) == cap
    ctx.sync()
    assert d_c.cpu().tolist() == [0, 0] and bool((d_m.cpu() == 0x5A5A5A5A).all())
    ctx.close()


@pytest.mark.gpu
def test_gpu_tracking_is_untouched_by_match_calls(capi, synth):
    """one live call before and after match calls on the same context: the same bits, the same params"""
    w, h, intr = VGA
    ref, tgt = synth.render_pair(w, h, *intr, seed=4100)[:2]
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2, max_pairs=1))
    ctx.upload_frames(0, np.stack([ref, tgt]))
    ctx.build_pyramids(0, 2)
    ctx.apply_gradient(0, 2)
    kp = np.random.default_rng(3).uniform([6, 6], [w - 7, h - 7], (200, 2)).astype(np.float32)
    before, st0 = ctx.estimate_pose_features_batch([0], [1], [kp], raise_on_pair_failure=True)
    params0 = bytes(ctx.params)
    A, B, _, _ = synth.descriptor_pair(11, 700, 650, 64, "l2")
    want, _, _ = R.match(A, B)
    assert same(ctx.match_descriptors_batch([(A, B)])[0], want)
    H = synth.descriptor_pair(12, 300, 310, 32, "hamming")[:2]
    assert same(ctx.match_descriptors_batch([H] * 3)[2], R.match(*H)[0])
    ctx.knn_match_batch([(A, B)])
    after, st1 = ctx.estimate_pose_features_batch([0], [1], [kp], raise_on_pair_failure=True)
    assert np.array_equal(before, after) and st0 == st1
    assert bytes(ctx.params) == params0
    p = capi.Params()
    assert capi.lib().uwt_get_params(ctx._h, C.byref(p)) == 0 and bytes(p) == params0
    ctx.close()


def scene_with_descriptors(synth, seed, n=300, m=280):
    """a rendered pair, descriptor sets with known correspondences, and key points placed on the generator's matched rows"""
    w, h, intr = VGA
    ref, tgt = synth.render_pair(w, h, *intr, seed=seed)[:2]
    A, B, dst, src = synth.descriptor_pair(seed + 1, n, m, 64, "l2")
    rng = np.random.default_rng(seed + 2)
    kpa = rng.uniform([6, 6], [w - 7, h - 7], (n, 2)).astype(np.float32)
    kpb = rng.uniform([6, 6], [w - 7, h - 7], (m, 2)).astype(np.float32)
    kpb[dst] = kpa[src]
    return ref, tgt, A, B, kpa, kpb


@pytest.mark.gpu
def test_gpu_python_mirror_end_to_end(capi, synth):
    """descriptors -> MatchDescriptors -> getGoodKeypoints -> the live call; the pose equals the one the restatement's key points
    give through the existing call"""
    tracker = importlib.import_module("uw-slam_amd.tracker")
    w, h, intr = VGA
    ref, tgt, A, B, kpa, kpb = scene_with_descriptors(synth, 4200)
    tr = tracker.Tracker(False, max_frames=2)
    tr.InitializePyramid(w, h, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    prev, cur = tracker.Frame(ref), tracker.Frame(tgt, id_frame=1)
    rm = tracker.RobustMatcher(tr)
    want, _, _ = R.match(A, B, rm.ratio_)
    assert 100 < len(want) < 300
    kept = rm.MatchAndSetKeypoints(prev, cur, A, B, (kpa, kpb))
    assert same(kept, want) and prev.n_matches_ == cur.n_matches_ == len(want)
    assert np.array_equal(prev.keypoints_, kpa[want["query_idx"]]) and np.array_equal(cur.keypoints_, kpb[want["train_idx"]])
    assert np.array_equal(prev.keypoints_, cur.keypoints_)   # every symmetric match of this scene is a true correspondence
    tr.ApplyGradient(prev)
    tr.ApplyGradient(cur)
    assert tr.EstimatePoseFeaturesBatch([(prev, cur)])[0]["status"] == 0
    # the restatement's key points through the existing batched call on a context of its own
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2, max_pairs=1))
    ctx.upload_frames(0, np.stack([ref, tgt]))
    ctx.build_pyramids(0, 2)
    ctx.apply_gradient(0, 2)
    poses, st = ctx.estimate_pose_features_batch([0], [1], [kpa[want["query_idx"]]], raise_on_pair_failure=True)
    assert np.array_equal(prev.rigid_transformation_, poses[0])
    # with an inlier mask from the caller's RANSAC: every second match
    mask = np.arange(len(want)) % 2 == 0
    kept = rm.MatchAndSetKeypoints(prev, cur, A, B, (kpa, kpb), inlier_mask=mask)
    assert same(kept, want[mask]) and prev.n_matches_ == int(mask.sum())
    ctx.close()


@pytest.mark.gpu
def test_gpu_cpp_mirror_end_to_end(capi, synth, tmp_path, arith):
    w, h, intr = VGA
    exe = str(tmp_path / "shim_match")
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_match.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    scenes = [scene_with_descriptors(synth, 4300 + 10 * i, n=260 + 30 * i, m=300 - 20 * i) for i in range(3)]
    (tmp_path / "frames.raw").write_bytes(b"".join(s[0].tobytes() + s[1].tobytes() for s in scenes))
    with open(tmp_path / "desc.bin", "wb") as f:
        for _, _, A, B, kpa, kpb in scenes:
            f.write(np.array([len(A), len(B), A.shape[1]], np.int32).tobytes() + A.tobytes() + B.tobytes() + kpa.tobytes() + kpb.tobytes())
    r = subprocess.run([exe, str(tmp_path / "frames.raw"), str(tmp_path / "desc.bin"), str(w), str(h), "3"] +
                       (["legacy"] if arith == "legacy" else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.split("\n")
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=6, max_pairs=3))
    ctx.upload_frames(0, np.stack([f for s in scenes for f in s[:2]]))
    ctx.build_pyramids(0, 6)
    ctx.apply_gradient(0, 6)
    wants = [R.match(s[2], s[3], np.float32(0.65))[0] for s in scenes]
    poses, st = ctx.estimate_pose_features_batch([0, 2, 4], [1, 3, 5], [s[4][wn["query_idx"]] for s, wn in zip(scenes, wants)],
                                                 raise_on_pair_failure=True)
    for i, wn in enumerate(wants):
        mt = [l for l in lines if l.startswith("MATCH %d " % i)][0].split()
        assert [int(v) for v in mt[2:]] == [len(wn), wn["query_idx"][0], wn["train_idx"][0]]
        pr = [l for l in lines if l.startswith("PAIR %d " % i)][0].split()
        assert np.array_equal(np.array(pr[2:9], np.float32), poses[i]), (i, pr, poses[i])
        assert [int(v) for v in pr[9:]] == [st[i]["iterations"], st[i]["status"], st[i]["n_valid"]]
    ctx.close()


@pytest.mark.gpu
def test_gpu_match_bench_tool_parity_is_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "match_bench.py"), "--reps", "2"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert out["parity"]["clean"] is True, out["parity"]
    assert set(out["throughput"]["surf_2000x2000x64"]) == {"1", "64", "1024"}
