"""Early preparation of a batch call (uwt_tuning::overlap_gradients): a dense batch call that ends on level 0 leaves a
window behind its level 1, and the next uwt_track_batch_async puts its pyramids and its gradients of the levels >= 1 on the side
stream inside that window.  HOW the launches are ordered, never WHAT they compute: every comparison here is bitwise against a second
context with the early preparation off (overlap_gradients = 2: the order of the library before it existed), on a context that forces
the path at any batch size (overlap_gradients = 3).

Frames are 64 x 48 with 4 levels and depth (the one-pass pyramid of a batch needs width % 16 == 0 and height % 8 == 0; level 3 is
8 x 6), 12 pairs per call; calls are enqueued back to back with no wait between them, as a pipeline of calls does."""
import importlib

import numpy as np
import pytest

import guard_bands as GB

pytestmark = pytest.mark.gpu
ARITH_INDEPENDENT = True   # the order of launches does not depend on the arithmetic set

W, H, LEVELS, P = 64, 48, 4, 12
INTR = (52.5, 52.5, 31.5, 23.5)
ON, OFF = dict(overlap_gradients=3), dict(overlap_gradients=2)
FIXED = dict(n_levels=LEVELS, first_level=3, last_level=0, max_iters=5, early_exit=0, has_depth=1)
# launch shapes under which a window exists: one part with every level in one launch (the default at this size), two parts on two
# streams, a launch per evaluation on every level (the form of the large levels), both
SHAPES = [dict(), dict(split_min_px=1, split_min=2), dict(coarse_batch_px=0), dict(coarse_batch_px=0, split_min_px=1, split_min=2)]
INVALID_ARG = 1


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def scenes(synth):
    """three sets of 2 P frames with depth (pair i in frames 2 i, 2 i + 1), rendered once and never changed"""
    out = []
    for base in (100, 300, 500):
        fr, dp = [], []
        for i in range(P):
            ref, tgt, dep, _, _ = synth.render_pair(W, H, *INTR, seed=base + i, with_depth=True)
            fr += [ref, tgt]
            dp += [dep, dep]
        out.append((np.stack(fr), np.stack(dp)))
    return out


def make(capi, tuning, max_frames=2 * P, **over):
    params = dict(FIXED, max_frames=max_frames, max_pairs=P)
    params.update(over)
    return capi.Context(capi.default_params(W, H, *INTR, **params), tuning=tuning)


def pinned(capi, frames, depth):
    f = capi.pinned_empty(frames.shape, np.uint8)
    d = capi.pinned_empty(depth.shape, np.uint16)
    f[...] = frames
    d[...] = depth
    return f, d


class Results:
    """device buffers for the poses and stats of a run of calls, one pair of buffers per call: nothing waits between the calls"""

    def __init__(self, n_calls, n_pairs=P):
        import torch
        self.poses = [torch.zeros((n_pairs, 7), dtype=torch.float32, device="cuda") for _ in range(n_calls)]
        self.stats = [torch.zeros((n_pairs, 4), dtype=torch.int32, device="cuda") for _ in range(n_calls)]
        torch.cuda.synchronize()   # torch's fills run on torch's stream, not on the context's

    def ptrs(self, k):
        return self.poses[k].data_ptr(), self.stats[k].data_ptr()

    def bytes(self):
        return [(p.cpu().numpy().tobytes(), s.cpu().numpy().tobytes()) for p, s in zip(self.poses, self.stats)]


def planes(capi, ctx, slots, grad_slots):
    """img and depth of levels 1..3 of `slots`; gx, gy of levels 0..3 and depth of `grad_slots` (what a call prepared)"""
    out = {}
    slots, grad_slots = [int(s) for s in slots], [int(s) for s in grad_slots]
    for s in slots:
        for l in range(1, LEVELS):
            out[("img", s, l)] = ctx.get_plane(s, l, capi.PLANE_IMAGE).tobytes()
    for s in grad_slots:
        for l in range(LEVELS):
            if l:
                out[("depth", s, l)] = ctx.get_plane(s, l, capi.PLANE_DEPTH).tobytes()
            out[("gx", s, l)] = ctx.get_plane(s, l, capi.PLANE_GRADX).tobytes()
            out[("gy", s, l)] = ctx.get_plane(s, l, capi.PLANE_GRADY).tobytes()
    return out


REF = np.arange(P, dtype=np.int32) * 2
TGT = REF + 1


def run_both(capi, run, shape=None, **over):
    """run(ctx) on a context that forces the early preparation and on one without it; both results"""
    got = []
    for switch in (ON, OFF):
        ctx = make(capi, dict(shape or {}, **switch), **over)
        try:
            got.append(run(ctx))
        finally:
            ctx.close()
    return got


@pytest.mark.parametrize("refs_only", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()) or "default")
def test_back_to_back_calls_on_the_same_slots(capi, scenes, shape, refs_only):
    """four calls on the same slots and lists, enqueued without a wait: poses and stats of every call, then every plane a call
    prepares, equal the switch-off context's"""
    frames, depth = scenes[0]

    def run(ctx):
        ctx.upload_frames(0, frames, depth)
        res = Results(4)
        for k in range(4):
            ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(k), grad_refs_only=refs_only)
        ctx.sync()
        return res.bytes(), planes(capi, ctx, range(2 * P), REF if refs_only else range(2 * P))

    (on_res, on_planes), (off_res, off_planes) = run_both(capi, run, shape)
    assert on_res == off_res
    assert on_res[0] == on_res[3]   # (the same inputs: the same bits, call after call)
    assert on_planes.keys() == off_planes.keys() and all(on_planes[k] == off_planes[k] for k in on_planes), [
        k for k in on_planes if on_planes[k] != off_planes[k]][:8]


@pytest.mark.parametrize("shape", SHAPES[:2], ids=["one_part", "two_parts"])
def test_streaming_pattern_two_slot_ranges_two_lists(capi, scenes, shape):
    """two slot ranges with different pair lists; new content is uploaded (uwt_upload_frames_async) into the idle range while a call
    runs on the other; six calls.  The lists alternate — a call's lists equal those of two calls back, which the idle device set
    still holds — and the fifth call brings a third list for the first range."""
    lists = [(REF, TGT), (2 * P + TGT, 2 * P + REF), (REF, TGT), (2 * P + TGT, 2 * P + REF), (REF[::-1].copy(), TGT[::-1].copy()),
             (2 * P + TGT, 2 * P + REF)]
    content = [scenes[0], scenes[1], scenes[2], (scenes[0][0][::-1].copy(), scenes[0][1][::-1].copy()),
               (np.roll(scenes[1][0], 2, axis=0), np.roll(scenes[1][1], 2, axis=0)), (scenes[2][0][::-1].copy(), scenes[2][1][::-1].copy())]

    def run(ctx):
        res = Results(6)
        held = [pinned(capi, *c) for c in content]   # untouched until the sync below
        for k in range(6):
            first = (k & 1) * 2 * P
            ctx.upload_frames_async(first, *held[k])
            ctx.track_batch_async(first, 2 * P, *lists[k], *res.ptrs(k), grad_refs_only=True)
        ctx.sync()
        return res.bytes()

    on, off = run_both(capi, run, shape, max_frames=4 * P)
    assert on == off
    assert len(set(on)) == 6   # (six different calls)


def test_upload_into_the_same_slots_between_two_calls(capi, scenes):
    """call on content X, asynchronous upload of Y into the same slots, call again: the upload waits for the first call, the early
    preparation for the upload — the second call's poses are a fresh context's on Y"""
    (xf, xd), (yf, yd) = scenes[0], scenes[1]

    def run(ctx):
        ctx.upload_frames(0, xf, xd)
        res = Results(2)
        held = pinned(capi, yf, yd)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(0))
        ctx.upload_frames_async(0, *held)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(1))
        ctx.sync()
        return res.bytes()

    on, off = run_both(capi, run)
    assert on == off
    fresh = make(capi, OFF)
    fresh.upload_frames(0, yf, yd)
    res = Results(1)
    fresh.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(0))
    fresh.sync()
    assert res.bytes()[0] == on[1] and on[0] != on[1]
    fresh.close()


def test_a_plane_read_back_between_two_calls_closes_the_window(capi, scenes):
    """call, read-back of a level-2 plane, upload, second call: the read-back returns the first call's pyramid bytes and the second
    call is the switch-off context's"""
    (xf, xd), (yf, yd) = scenes[0], scenes[1]

    def run(ctx):
        ctx.upload_frames(0, xf, xd)
        res = Results(2)
        held = pinned(capi, yf, yd)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(0))
        got = [ctx.get_plane(s, 2, capi.PLANE_IMAGE).tobytes() for s in (0, 5, 2 * P - 1)]
        ctx.upload_frames_async(0, *held)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(1))
        ctx.sync()
        return res.bytes(), got

    (on, on_planes), (off, off_planes) = run_both(capi, run)
    assert on == off and on_planes == off_planes
    ref = make(capi, OFF)   # level 2 of X by the stage call
    ref.upload_frames(0, xf, xd)
    ref.build_pyramids(0, 2 * P)
    assert on_planes == [ref.get_plane(s, 2, capi.PLANE_IMAGE).tobytes() for s in (0, 5, 2 * P - 1)]
    ref.close()


@pytest.mark.parametrize("entry", ["candidates_async", "residual_jacobian"])
def test_another_entry_between_two_calls_closes_the_window(capi, scenes, entry):
    """the second range holds the planes of content X while its level 0 has taken content Y; a call on the first range, then an entry
    that reads the second range's planes of the levels >= 1 (enqueued behind that call), then a call on the second range: the entry
    still finds X's planes there — its results and both calls' are the switch-off context's"""
    (xf, xd), (yf, yd), (zf, zd) = scenes

    def run(ctx):
        res = Results(4)
        ctx.upload_frames(0, zf, zd)
        ctx.upload_frames(2 * P, xf, xd)
        ctx.track_batch_async(2 * P, 2 * P, 2 * P + REF, 2 * P + TGT, *res.ptrs(0), grad_refs_only=False)
        ctx.sync()
        held = pinned(capi, yf, yd)
        ctx.upload_frames_async(2 * P, *held)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(1))
        if entry == "candidates_async":
            ctx.track_candidates_batch_async(2 * P + REF, 2 * P + TGT, *res.ptrs(2), threshold=10.0)
            between = None
        else:
            acc = ctx.residual_jacobian(2 * P, 2 * P + 1, 2, [0, 0, 0, 1, 0, 0, 0], dump=True)
            between = (acc["A"].tobytes(), acc["jtr"].tobytes(), acc["sum_r2"], acc["n_valid"], acc["J"].tobytes(), acc["r"].tobytes(),
                       acc["valid"].tobytes())
        ctx.track_batch_async(2 * P, 2 * P, 2 * P + REF, 2 * P + TGT, *res.ptrs(3))
        ctx.sync()
        return res.bytes(), between

    on, off = run_both(capi, run, max_frames=4 * P)
    assert on == off


NO_WINDOW = {
    "early_exit": (dict(early_exit=1, max_iters=20), P),
    "last_level_1": (dict(last_level=1), P),
    "three_pairs": (dict(), 3),
    "huber": (dict(weights=2), P),
}


@pytest.mark.parametrize("case", sorted(NO_WINDOW))
def test_schedules_without_a_window(capi, scenes, case):
    """an early-exit schedule, a schedule that ends above level 0, the chained form of a few pairs, robust weights: three calls in a
    row run as they always did, under either setting"""
    over, n = NO_WINDOW[case]
    frames, depth = scenes[0]

    def run(ctx):
        ctx.upload_frames(0, frames, depth)
        res = Results(3, n)
        for k in range(3):
            ctx.track_batch_async(0, 2 * P, REF[:n], TGT[:n], *res.ptrs(k))
        ctx.sync()
        return res.bytes()

    on, off = run_both(capi, run, **over)
    assert on == off


def test_set_tuning_and_a_failed_call_leave_no_window(capi, scenes):
    """call, uwt_set_tuning, call; then a call that fails with UWT_ERR_INVALID_ARG (a slot out of range), and a call after it"""
    frames, depth = scenes[0]

    def run(ctx):
        ctx.upload_frames(0, frames, depth)
        res = Results(4)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(0))
        ctx.set_tuning(split_min_px=1, split_min=2)
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(1))
        bad = TGT.copy()
        bad[-1] = 2 * P
        with pytest.raises(capi.UwtError) as err:
            ctx.track_batch_async(0, 2 * P, REF, bad, *res.ptrs(2))
        assert err.value.status == INVALID_ARG
        ctx.track_batch_async(0, 2 * P, REF, TGT, *res.ptrs(3))
        ctx.sync()
        return res.bytes()

    on, off = run_both(capi, run)
    assert on == off
    assert on[0] == on[1] == on[3] and on[2] == (bytes(P * 28), bytes(P * 16))   # the failed call wrote nothing


def result_specs(n_calls):
    specs = []
    for k in range(n_calls):
        specs += [GB.Buf("poses%d" % k, nbytes=P * 28, align=4, stride=28), GB.Buf("stats%d" % k, nbytes=P * 16, align=4, stride=16)]
    return specs


@pytest.mark.parametrize("end", ["destroy", "sync"])
def test_teardown_with_early_work_in_flight(capi, scenes, end):
    """two calls enqueued into guarded result buffers on a context with guarded work areas, then uwt_destroy at once — or uwt_sync and
    plane read-backs: the results are the switch-off context's and no guard byte has changed"""
    frames, depth = scenes[0]
    backend = GB.TorchBackend(importlib.import_module("torch"))

    def run(ctx):
        ctx.debug_guards(4096)
        ctx.upload_frames(0, frames, depth)
        arena = GB.Arena(backend, result_specs(2), GB.FILLS[1])
        for k in range(2):
            ctx.track_batch_async(0, 2 * P, REF, TGT, arena.ptr("poses%d" % k), arena.ptr("stats%d" % k))
        if end == "destroy":
            ctx.close()
            return arena.check(), None
        ctx.sync()
        got = planes(capi, ctx, range(2 * P), REF)
        assert ctx.debug_check_guards() == (0, "")
        return arena.check(), got

    (on, on_planes), (off, off_planes) = run_both(capi, run, SHAPES[1])
    assert on == off and on_planes == off_planes
    assert on["poses0"] == on["poses1"] and on["poses0"] != bytes([GB.OUT_FILL]) * (P * 28)
