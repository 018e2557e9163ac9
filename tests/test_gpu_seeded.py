"""The seeded calls (include/uwt.h "seeded calls"): an alignment that starts from a given pose, in every launch form and every
family, against tests/seeded_ref.py — the loop of the oracle written out over its stage functions with a start pose and the hand-off
choice.  Poses and uwt_stats are compared bit for bit everywhere; where a comparison is with another call of the library instead of
the reference, the docstring says so.

No input had to be replaced for the f64-sum-at-an-f32-midpoint event (README "Parity")."""
import ctypes as C
import importlib

import numpy as np
import pytest

import guard_bands as GB
import seeded_cases as SC
import seeded_ref as SR
import tracking_ref as TR

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, NO_VALID_POINTS, PAIR_FAILED = 0, 1, 2, 6
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
SENTINEL = 0x5A5A5A5A
SCHEDULES = {"fixed": dict(max_iters=4, early_exit=0), "early": dict(max_iters=50, early_exit=1)}
# EstimatePoseFeatures' locals (src/Tracker.cpp:633-640, 834, 856): what the reference loop is run with for the live call
FEATURES = dict(first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002, handoff_scale_t=1)
FAMILIES = ("dense_sync", "dense_async", "features_sync", "features_async", "candidates_sync", "candidates_async")
# the pair that spends more than first_poll + 1 = 4 evaluations on level 0 under early exit, per hand-off: pair 1 (scene 1, seed 1)
# under the reference's, pair 11 (scene 5, seed 11) under keep
HEAVY_PAIR = {0: 1, 1: 11}


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


# ---- contexts, device buffers, results -------------------------------------------------------------------------------------------
def make_ctx(capi, synth, max_pairs, size=(SC.W, SC.H, SC.INTR), depth=True, tuning=None, **over):
    w, h, intr = size
    kw = dict(SC.LEVELS)
    kw.update(over)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2 * SC.N_SCENES, max_pairs=max_pairs, has_depth=1 if depth else 0, **kw),
                       tuning=tuning)
    sc = SC.scenes(synth, size)
    ctx.upload_frames(0, np.stack([f for r, t, _ in sc for f in (r, t)]), np.stack([d for _, _, d in sc for _ in (0, 1)]) if depth else None)
    ctx.build_pyramids(0, 2 * SC.N_SCENES)
    ctx.apply_gradient(0, 2 * SC.N_SCENES)
    return ctx


def bits(poses, stats):
    """a call's results, one tuple per pair: (pose bytes, status, iterations, n_valid, error bits)"""
    return [(np.ascontiguousarray(poses[i], np.float32).tobytes(), int(s["status"]), int(s["iterations"]), int(s["n_valid"]),
             int(np.float32(s["error"]).view(np.uint32))) for i, s in enumerate(stats)]


def want_bits(result):
    st, pose, tr = result
    return (np.asarray(pose, np.float32).tobytes(),) + SR.stats_of(st, tr)


BAD_BITS = (IDENTITY.tobytes(), INVALID_ARG, 0, 0, 0)   # the record of a pair whose seed has a non-finite entry


class Dev:
    """device buffers of an asynchronous call: poses [n, 7] and stats [n, 4] filled with a sentinel, the seeds (None: no buffer)"""

    def __init__(self, torch, n, seeds=None):
        self.torch = torch
        self.poses = torch.full((n, 7), SENTINEL, dtype=torch.int32, device="cuda")
        self.stats = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
        self.seeds = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, np.float32)).cuda()
        torch.cuda.synchronize()   # (torch fills on its own stream)

    def seeds_ptr(self):
        return None if self.seeds is None else self.seeds.data_ptr()

    def fetch(self, capi):
        self.torch.cuda.synchronize()
        p = self.poses.cpu().numpy().view(np.float32)
        s = self.stats.cpu().numpy().view(capi.STATS).reshape(-1)
        return p, [dict(status=int(r["status"]), iterations=int(r["iterations"]), n_valid=int(r["n_valid"]), error=np.float32(r["error"])) for r in s]

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.poses == SENTINEL).all()) and bool((self.stats == SENTINEL).all())


def keypoints(n):
    """key-point lists of different lengths for n pairs; pair 2's is empty"""
    rng = np.random.default_rng(77)
    counts = [40, 12, 0, 25, 60, 7]
    return [rng.uniform([6, 6], [SC.W - 7, SC.H - 7], (counts[k % len(counts)], 2)).astype(np.float32) for k in range(n)]


def run(capi, torch, ctx, family, n, seeds="unseeded", handoff=None, weights=None, sampler=None):
    """One call of a family on the first n pairs.  seeds "unseeded": the unseeded entry; else the seeded one (None: a null pointer).
    Returns (poses, stats) as the synchronous mirrors do."""
    ref, tgt = SC.pair_slots(n)
    seeded = not isinstance(seeds, str)
    kind, form = family.split("_")
    if form == "sync":
        if kind == "dense":
            return ctx.estimate_pose_batch_seeded(ref, tgt, seeds, handoff) if seeded else ctx.estimate_pose_batch(ref, tgt)
        if kind == "features":
            if seeded:
                return ctx.estimate_pose_features_batch_seeded(ref, tgt, keypoints(n), seeds, handoff, weights=weights, sampler=sampler)
            return ctx.estimate_pose_features_batch(ref, tgt, keypoints(n), weights=weights, sampler=sampler)
        if seeded:
            return ctx.estimate_pose_candidates_batch_seeded(ref, tgt, seeds, handoff, weights=weights, sampler=sampler)
        return ctx.estimate_pose_candidates_batch(ref, tgt, weights=weights, sampler=sampler)
    d = Dev(torch, n, seeds if seeded else None)
    P, S = d.poses.data_ptr(), d.stats.data_ptr()
    if kind == "dense":
        if seeded:
            ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, P, S, d_seeds_ptr=d.seeds_ptr(), handoff=handoff)
        else:
            ctx.track_batch_async(0, 2 * SC.N_SCENES, ref, tgt, P, S)
    elif kind == "features":
        if seeded:
            ctx.track_features_batch_seeded_async(ref, tgt, keypoints(n), P, S, d.seeds_ptr(), handoff, weights=weights, sampler=sampler)
        else:
            ctx.track_features_batch_async(ref, tgt, keypoints(n), P, S, weights=weights, sampler=sampler)
    else:
        if seeded:
            ctx.track_candidates_batch_seeded_async(ref, tgt, P, S, d.seeds_ptr(), handoff, weights=weights, sampler=sampler)
        else:
            ctx.track_candidates_batch_async(ref, tgt, P, S, weights=weights, sampler=sampler)
    ctx.sync()
    return d.fetch(capi)


def dense_want(O, synth, arith, n, seeds, keep=False, **over):
    return [want_bits(SC.expect(O, synth, arith, k % SC.N_SCENES, None if seeds is None else seeds[k], keep, **over)) for k in range(n)]


# ---- A. null and identity seeds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_null_and_identity_seeds_equal_the_unseeded_entry(capi, torch, synth, family):
    """null seeds under handoff 0, a null options pointer, and explicit identity seeds: the unseeded entry's bytes, on 1, 2, 5 and 20
    pairs (a comparison of two calls of the library)"""
    ctx = make_ctx(capi, synth, 20)
    for n in (1, 2, 5, 20):
        base = bits(*run(capi, torch, ctx, family, n))
        assert bits(*run(capi, torch, ctx, family, n, None, 0)) == base, (family, n, "null seeds, handoff 0")
        assert bits(*run(capi, torch, ctx, family, n, None, None)) == base, (family, n, "null seeds, null options")
        assert bits(*run(capi, torch, ctx, family, n, np.tile(IDENTITY, (n, 1)), 0)) == base, (family, n, "identity seeds")
    ctx.close()


# ---- B. the dense launch forms against the reference --------------------------------------------------------------------------------
DENSE_FORMS = {   # name: (pairs, tuning, schedules)
    "inline_1": (1, None, ("fixed", "early")),
    "inline_2": (2, None, ("fixed", "early")),
    "chained_list": (5, None, ("fixed", "early")),
    "batch_coarse": (5, dict(chained=0, coarse_batch_px=6144), ("fixed", "early")),
    "batch_plain": (5, dict(chained=0, coarse_batch_px=0), ("fixed", "early")),
    "split": (5, dict(chained=0, split=2, split_min=1, split_min_px=1), ("fixed",)),      # parts of 2 and 3 pairs
    "split_plain": (5, dict(chained=0, coarse_batch_px=0, split=2, split_min=1, split_min_px=1), ("fixed",)),
    "tail_update": (5, dict(chained=0, tail_update=2), ("fixed", "early")),
}


@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
@pytest.mark.parametrize("form", list(DENSE_FORMS))
def test_dense_launch_forms_equal_the_reference(capi, torch, O, synth, arith, form, handoff):
    n, tuning, schedules = DENSE_FORMS[form]
    seeds = SC.seeds(O, n)
    for schedule in schedules:
        over = SCHEDULES[schedule]
        want = dense_want(O, synth, arith, n, seeds, bool(handoff), **over)
        assert all(w[1] == OK for w in want)
        ctx = make_ctx(capi, synth, n, tuning=tuning, **over)
        for family in ("dense_sync", "dense_async"):
            got = bits(*run(capi, torch, ctx, family, n, seeds, handoff))
            print(form, schedule, family, "handoff", handoff, [g[1:] for g in got])
            assert got == want, (form, schedule, family, [g[1:] for g in got], [w[1:] for w in want])
        ctx.close()


@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
def test_dense_handoff_scale_t(capi, torch, O, synth, arith, handoff):
    """the hand-off under handoff_scale_t = 1: the reference's doubles the translation too, keep leaves it"""
    seeds = SC.seeds(O, 3)
    over = dict(SCHEDULES["fixed"], handoff_scale_t=1)
    want = dense_want(O, synth, arith, 3, seeds, bool(handoff), **over)
    for tuning in (None, dict(chained=0), dict(chained=0, coarse_batch_px=0)):
        ctx = make_ctx(capi, synth, 3, tuning=tuning, **over)
        assert bits(*run(capi, torch, ctx, "dense_sync", 3, seeds, handoff)) == want, tuning
        ctx.close()


def test_handoff_scale_t_is_read_as_non_zero(capi, torch, O, synth):
    """uwt_params::handoff_scale_t is any int and has always meant "non-zero": a context with 2 there gives the bytes of one with 1 —
    unseeded, and seeded under handoff 0 — in the chained and the per-evaluation forms; it never reads as keep (comparisons of calls
    of the library)"""
    seeds = SC.seeds(O, 3)
    for tuning in (None, dict(chained=0), dict(chained=0, coarse_batch_px=0)):
        got = {}
        for value in (1, 2):
            ctx = make_ctx(capi, synth, 3, tuning=tuning, handoff_scale_t=value, **SCHEDULES["fixed"])
            got[value] = [bits(*run(capi, torch, ctx, "dense_sync", 3)), bits(*run(capi, torch, ctx, "dense_sync", 3, seeds, 0)),
                          bits(*run(capi, torch, ctx, "dense_async", 3, seeds, 0)), bits(*run(capi, torch, ctx, "candidates_sync", 3, seeds, 0))]
            keep = bits(*run(capi, torch, ctx, "dense_sync", 3, seeds, 1))
            ctx.close()
        assert got[1] == got[2], tuning
        assert keep != got[2][1]
    ctx0 = make_ctx(capi, synth, 3, handoff_scale_t=0, **SCHEDULES["fixed"])
    assert bits(*run(capi, torch, ctx0, "dense_sync", 3)) != got[2][0]
    ctx0.close()


@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
@pytest.mark.parametrize("weights,sampler", [(1, 0), (2, 0), (0, 1), (2, 1)], ids=["tukey", "huber", "bilinear", "huber_bilinear"])
def test_dense_robust_and_bilinear_equal_the_reference(capi, torch, O, synth, arith, weights, sampler, handoff):
    """3 pairs: the chained robust flow (k_coarse_weighted, k_hist_iterate) and the per-evaluation launches, both schedules"""
    seeds = SC.seeds(O, 3)
    for schedule, over in SCHEDULES.items():
        over = dict(over, weights=weights, sampler=sampler)
        want = dense_want(O, synth, arith, 3, seeds, bool(handoff), **over)
        for tuning in (None, dict(chained=0), dict(chained=0, coarse_batch_px=0, coarse_weighted=0)):
            ctx = make_ctx(capi, synth, 3, tuning=tuning, **over)
            got = bits(*run(capi, torch, ctx, "dense_sync", 3, seeds, handoff))
            print(schedule, tuning, [g[1:] for g in got], [w[1:] for w in want])
            assert got == want, (schedule, tuning)
            ctx.close()


def test_dense_f32_sums_forms_agree(capi, torch, O, synth):
    """accumulate_f64 = 0: the oracle does not reproduce f32 partial sums, so the seeded call is held to the library's own forms — the
    update as a launch of its own against the update in the evaluation's tail, one stream against two parts, the synchronous entry
    against the device entry — and must differ from the identity start"""
    seeds = SC.seeds(O, 5)
    got = []
    for tuning in (dict(tail_update=0), dict(tail_update=2), dict(split=2, split_min=1, split_min_px=1, tail_update=0),
                   dict(split=2, split_min=1, split_min_px=1, tail_update=1)):
        ctx = make_ctx(capi, synth, 5, tuning=tuning, accumulate_f64=0, **SCHEDULES["fixed"])
        got.append(bits(*run(capi, torch, ctx, "dense_sync", 5, seeds, 0)))
        got.append(bits(*run(capi, torch, ctx, "dense_async", 5, seeds, 0)))
        unseeded = bits(*run(capi, torch, ctx, "dense_sync", 5))
        ctx.close()
    assert all(g == got[0] for g in got)
    assert all(g[1] == OK and g[0] != u[0] for g, u in zip(got[0], unseeded))


def test_dense_odd_size(capi, torch, O, synth, arith):
    """101 x 67 x 3: ragged rows on every level, both hand-offs, chained and per-evaluation launches"""
    seeds = SC.seeds(O, 3)
    for handoff in (0, 1):
        want = [want_bits(SC.expect(O, synth, arith, k, seeds[k], bool(handoff), size=SC.ODD, **SCHEDULES["early"])) for k in range(3)]
        assert all(w[1] == OK for w in want)
        for tuning in (None, dict(chained=0)):
            ctx = make_ctx(capi, synth, 3, size=SC.ODD, tuning=tuning, **SCHEDULES["early"])
            assert bits(*run(capi, torch, ctx, "dense_sync", 3, seeds, handoff)) == want, (handoff, tuning)
            ctx.close()


def test_batch_independence(capi, torch, O, synth):
    """a pair's bits depend neither on the batch nor on its place in it: 20 pairs (the per-evaluation launches) against each pair in a
    call of its own (the inline chained flow) — a comparison of calls of the library; the reference holds 5 of them in test B"""
    seeds = SC.seeds(O, 20)
    ctx = make_ctx(capi, synth, 20, **SCHEDULES["early"])
    batch = bits(*run(capi, torch, ctx, "dense_sync", 20, seeds, 1))
    ref, tgt = SC.pair_slots(20)
    for k in (0, 7, 13, 19):
        alone = bits(*ctx.estimate_pose_batch_seeded(ref[k:k + 1], tgt[k:k + 1], seeds[k:k + 1], 1))
        assert alone[0] == batch[k], k
    ctx.close()


def test_null_seeds_under_keep_equal_the_reference(capi, torch, O, synth, arith):
    """a null seed pointer with handoff 1 — the identity start whose pose crosses the levels unchanged — against
    seeded_ref.align(seed=None, keep=True): dense (inline, chained, per-evaluation launches) and candidates, both schedules"""
    for schedule, over in SCHEDULES.items():
        for n, tuning in ((1, None), (5, None), (5, dict(chained=0)), (5, dict(chained=0, coarse_batch_px=0))):
            want = dense_want(O, synth, arith, n, None, True, **over)
            assert all(w[1] == OK for w in want) and want != dense_want(O, synth, arith, n, None, False, **over)
            ctx = make_ctx(capi, synth, n, tuning=tuning, **over)
            for family in ("dense_sync", "dense_async"):
                assert bits(*run(capi, torch, ctx, family, n, None, 1)) == want, (schedule, n, tuning, family)
            ctx.close()
        n = 3
        ctx = make_ctx(capi, synth, n, **over)
        ref, tgt = SC.pair_slots(n)
        want = []
        for k in range(n):
            tables = {l: ctx.obtain_candidate_points(int(ref[k]), l, 20.0)[0] for l in range(3)}
            key = hash(("cand",) + tuple(tables[l].tobytes() for l in range(3)))
            want.append(want_bits(SC.expect(O, synth, arith, k, None, True, tables=tables, tables_key=key, **over)))
        for family in ("candidates_sync", "candidates_async"):
            assert bits(*run(capi, torch, ctx, family, n, None, 1)) == want, (schedule, family)
        ctx.close()


# ---- C. the speculative rerun ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
@pytest.mark.parametrize("n", [1, 2])
def test_speculative_rerun_starts_from_the_seed(capi, O, synth, arith, n, handoff):
    """a fresh context, early exit, the one- and two-pair synchronous call on the pair that needs more than first_poll + 1 = 4
    evaluations on level 0: the first run is cut short and the alignment runs again — from the seed, or the result is not the
    reference's"""
    seeds = SC.seeds(O)
    heavy = HEAVY_PAIR[handoff]
    ks = [heavy] if n == 1 else [0, heavy]
    want = [want_bits(SC.expect(O, synth, arith, k % SC.N_SCENES, seeds[k], bool(handoff), **SCHEDULES["early"])) for k in ks]
    tr = SC.expect(O, synth, arith, heavy % SC.N_SCENES, seeds[heavy], bool(handoff), **SCHEDULES["early"])[2]
    assert SR.level_evaluations(tr)[0] > 4   # level 0 is the chained level: the speculative run is cut short there
    ref, tgt = SC.pair_slots(SC.N_SEEDS)
    got = {}
    for speculation in (1, 0):
        ctx = make_ctx(capi, synth, 2, tuning=dict(speculation=speculation), **SCHEDULES["early"])
        got[speculation] = bits(*ctx.estimate_pose_batch_seeded(ref[ks], tgt[ks], seeds[ks], handoff))
        ctx.close()
    assert got[1] == want and got[0] == want, (got[1], got[0], want)


# ---- E. bad seeds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [3, 20])
def test_bad_seed_fails_its_pair_alone(capi, torch, O, synth, family, n):
    """a seed with a non-finite entry in the middle of 3 and of 20 pairs: that pair's record is {INVALID_ARG, 0, 0, 0} with the
    identity, the neighbours have the bits of the same call with a good seed in its place (a comparison of calls of the library; the
    synchronous forms return UWT_ERR_PAIR_FAILED)"""
    ctx = make_ctx(capi, synth, n)
    good = SC.seeds(O, n)
    base = bits(*run(capi, torch, ctx, family, n, good, 0))
    mid = n // 2
    for bad in SC.bad_seeds():
        seeds = good.copy()
        seeds[mid] = bad
        got = bits(*run(capi, torch, ctx, family, n, seeds, 0))
        assert got[mid] == BAD_BITS, (family, n, bad, got[mid][1:])
        assert got[:mid] == base[:mid] and got[mid + 1:] == base[mid + 1:], (family, n, bad)
    if family.endswith("sync"):
        seeds = good.copy()
        seeds[mid] = SC.bad_seeds()[0]
        ref, tgt = SC.pair_slots(n)
        with pytest.raises(capi.UwtError) as e:
            if family == "dense_sync":
                ctx.estimate_pose_batch_seeded(ref, tgt, seeds, raise_on_pair_failure=True)
            elif family == "features_sync":
                ctx.estimate_pose_features_batch_seeded(ref, tgt, [keypoints(1)[0]] * n, seeds, raise_on_pair_failure=True)
            else:
                ctx.estimate_pose_candidates_batch_seeded(ref, tgt, seeds, raise_on_pair_failure=True)
        assert e.value.status == PAIR_FAILED
    ctx.close()


# ---- F. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["dense_async", "features_async", "candidates_async"])
def test_refusals_enqueue_nothing(capi, torch, O, synth, family):
    """seeds overlapping an output (equal, shifted by one row, inside the stats), a non-zero reserved word, handoff outside 0..1:
    UWT_ERR_INVALID_ARG, the outputs untouched"""
    n = 3
    ctx = make_ctx(capi, synth, n)
    ref, tgt = SC.pair_slots(n)
    kind = family.split("_")[0]

    def call(d, seeds_ptr, sopt):
        P, S = d.poses.data_ptr(), d.stats.data_ptr()
        if kind == "dense":
            ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, P, S, d_seeds_ptr=seeds_ptr, handoff=sopt)
        elif kind == "features":
            ctx.track_features_batch_seeded_async(ref, tgt, keypoints(n), P, S, seeds_ptr, sopt)
        else:
            ctx.track_candidates_batch_seeded_async(ref, tgt, P, S, seeds_ptr, sopt)

    big = torch.full((2 * n + 2, 7), SENTINEL, dtype=torch.int32, device="cuda")   # poses at rows 1..n: seeds may start a row earlier or later
    big[n + 1:2 * n + 1] = torch.from_numpy(SC.seeds(O, n).view(np.int32)).cuda()    # (the legal call's seeds: the rows behind the poses)
    torch.cuda.synchronize()

    class Overlaid:
        poses = big[1:n + 1]
        stats = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")

    for shift in (0, 28, -28, 4, 28 * (n - 1) + 24):
        with pytest.raises(capi.UwtError) as e:
            call(Overlaid, Overlaid.poses.data_ptr() + shift, None)
        assert e.value.status == INVALID_ARG, shift
    with pytest.raises(capi.UwtError) as e:
        call(Overlaid, Overlaid.stats.data_ptr() + 16, None)   # inside the stats
    assert e.value.status == INVALID_ARG
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((Overlaid.poses == SENTINEL).all()) and bool((Overlaid.stats == SENTINEL).all()) and bool((big[0] == SENTINEL).all())
    call(Overlaid, Overlaid.poses.data_ptr() + 28 * n, None)   # the row behind the poses: legal
    ctx.sync()
    d = Dev(torch, n, SC.seeds(O, n))
    for field, value in (("handoff", 2), ("handoff", -1), ("reserved", 1)):
        o = capi.seed_options()
        if field == "handoff":
            o.handoff = value
        else:
            o.reserved[6] = value
        with pytest.raises(capi.UwtError) as e:
            call(d, d.seeds_ptr(), o)
        assert e.value.status == INVALID_ARG, (field, value)
    ctx.sync()
    assert d.untouched()
    # the synchronous forms check their options too
    with pytest.raises(capi.UwtError) as e:
        o = capi.seed_options()
        o.reserved[0] = 7
        ctx.estimate_pose_batch_seeded(ref, tgt, SC.seeds(O, n), o)
    assert e.value.status == INVALID_ARG
    ctx.close()


# ---- G. device chaining ----------------------------------------------------------------------------------------------------------------
def test_device_chaining_without_a_wait(capi, torch, O, synth, arith):
    """call 1's pose buffer is call 2's seeds with no sync between, one sync at the end: the same two calls staged through the host,
    and the reference's two alignments one after the other"""
    n = 5
    seeds = SC.seeds(O, n)
    ref, tgt = SC.pair_slots(n)
    ctx = make_ctx(capi, synth, n, **SCHEDULES["fixed"])
    a, b = Dev(torch, n, seeds), Dev(torch, n)
    ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, a.poses.data_ptr(), a.stats.data_ptr(), d_seeds_ptr=a.seeds_ptr(), handoff=1)
    ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, b.poses.data_ptr(), b.stats.data_ptr(), d_seeds_ptr=a.poses.data_ptr(), handoff=1)
    ctx.sync()
    first, second = bits(*a.fetch(capi)), bits(*b.fetch(capi))
    p1, s1 = ctx.estimate_pose_batch_seeded(ref, tgt, seeds, 1)
    p2, s2 = ctx.estimate_pose_batch_seeded(ref, tgt, p1, 1)
    assert first == bits(p1, s1) and second == bits(p2, s2)
    want1 = dense_want(O, synth, arith, n, seeds, True, **SCHEDULES["fixed"])
    want2 = dense_want(O, synth, arith, n, np.stack([np.frombuffer(w[0], np.float32) for w in want1]), True, **SCHEDULES["fixed"])
    assert first == want1 and second == want2
    ctx.close()


def test_predict_seed_track_accumulate_without_a_wait(capi, torch, O, synth, arith):
    """predict_seeds -> seeded dense call -> accumulate_trajectory_device_from_async on one stream, one sync: the three steps staged
    through the host and their restatements (seeded_ref.predict_seeds, seeded_ref.align, oracle.accumulate_trajectory)"""
    n = 5
    S = SC.seeds(O, 2 * n)
    prev, cur = S[:n], np.stack([O.se3_mul(S[k], S[n + k]) for k in range(n)])
    ref, tgt = SC.pair_slots(n)
    ctx = make_ctx(capi, synth, n, **SCHEDULES["fixed"])
    f32 = dict(dtype=torch.float32, device="cuda")
    d_prev, d_cur = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
    d_seed, d_traj = torch.zeros((n, 7), **f32), torch.zeros((n, 7), **f32)
    d_start = torch.from_numpy(S[7].copy()).cuda()
    d = Dev(torch, n)
    ctx.predict_seeds_device_async(n, d_prev.data_ptr(), d_cur.data_ptr(), d_seed.data_ptr())
    ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, d.poses.data_ptr(), d.stats.data_ptr(), d_seeds_ptr=d_seed.data_ptr(), handoff=1)
    ctx.accumulate_trajectory_device_from_async(d.poses.data_ptr(), n, d_start.data_ptr(), d_traj.data_ptr())
    ctx.sync()
    want_seed = SR.predict_seeds(O, prev, cur)
    assert d_seed.cpu().numpy().tobytes() == want_seed.tobytes()
    want = dense_want(O, synth, arith, n, want_seed, True, **SCHEDULES["fixed"])
    got = bits(*d.fetch(capi))
    assert got == want
    poses = np.stack([np.frombuffer(w[0], np.float32) for w in want])
    assert d_traj.cpu().numpy().tobytes() == O.accumulate_trajectory(poses, start=S[7]).tobytes()
    ctx.close()


def test_predict_seeds_contract(capi, torch, O):
    """the bits of the numpy restatement over many rows, the same under both arithmetic sets' contexts; a non-finite input row gives an
    all-NaN row; an output that overlaps an input is refused; n = 0 enqueues nothing"""
    rng = np.random.default_rng(5)
    n = 300
    tw = rng.uniform(-1, 1, (2 * n, 6)) * [0.3, 0.3, 0.3, 0.5, 0.5, 0.5]
    poses = np.stack([O.se3_exp(t.astype(np.float32)) for t in tw])
    prev, cur = poses[:n].copy(), poses[n:].copy()
    prev[3, 2] = np.nan
    cur[10, 6] = np.inf
    prev[11, 4] = -np.inf
    want = SR.predict_seeds(O, prev, cur)
    assert np.isnan(want[[3, 10, 11]]).all() and np.isfinite(np.delete(want, [3, 10, 11], 0)).all()
    out = []
    for ar in (0, 1):
        ctx = capi.Context(capi.default_params(SC.W, SC.H, *SC.INTR, arith=ar, **SC.LEVELS))
        d_prev, d_cur = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
        d_out = torch.zeros((n + 1, 7), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.predict_seeds_device_async(n, d_prev.data_ptr(), d_cur.data_ptr(), d_out.data_ptr())
        ctx.predict_seeds_device_async(0, d_prev.data_ptr(), d_cur.data_ptr(), d_prev.data_ptr())
        ctx.sync()
        got = d_out.cpu().numpy()
        assert got[:n].view(np.uint32).tobytes() == want.view(np.uint32).tobytes() and not got[n].any()
        out.append(got.tobytes())
        for bad in (d_prev.data_ptr(), d_cur.data_ptr() + 28 * (n - 1), d_prev.data_ptr() - 4):
            with pytest.raises(capi.UwtError) as e:
                ctx.predict_seeds_device_async(n, d_prev.data_ptr(), d_cur.data_ptr(), bad)
            assert e.value.status == INVALID_ARG
        ctx.close()
    assert out[0] == out[1]


# ---- H. tables ----------------------------------------------------------------------------------------------------------------------
TABLE_OPTIONS = {"identity": (None, None), "huber_bilinear": (2, 1), "tukey": (1, 0)}


@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
@pytest.mark.parametrize("options", list(TABLE_OPTIONS))
def test_features_equal_the_reference(capi, torch, O, synth, arith, options, handoff):
    """the live call (level 0, 3 pairs, 40 / 12 / 0 key points) from seeds, over the tables uwt_obtain_patch_points gives; the pair
    without a key point fails with NO_VALID_POINTS and the SEED as its pose, as the identity stood there in the unseeded call"""
    weights, sampler = TABLE_OPTIONS[options]
    n = 3
    seeds = SC.seeds(O, n)
    kps = keypoints(n)
    ctx = make_ctx(capi, synth, n)
    ref, tgt = SC.pair_slots(n)
    want = []
    for k in range(n):
        pts = ctx.obtain_patch_points(int(ref[k]), kps[k])[0] if len(kps[k]) else np.zeros((0, 4), np.float32)
        want.append(SC.expect(O, synth, arith, k, seeds[k], bool(handoff), tables={0: pts}, tables_key=hash(("patch", pts.tobytes())),
                              **dict(FEATURES, weights=weights or 0, sampler=sampler or 0)))
    for family in ("features_sync", "features_async"):
        got = bits(*run(capi, torch, ctx, family, n, seeds, handoff, weights=weights, sampler=sampler))
        print(options, family, [g[1:] for g in got], [want_bits(w)[1:] for w in want])
        for k in range(n):
            if want[k][0] == OK:
                assert got[k] == want_bits(want[k]), (family, k)
            else:
                assert (got[k][0], got[k][1]) == (np.asarray(seeds[k], np.float32).tobytes(), NO_VALID_POINTS) == \
                    (want[k][1].tobytes(), want[k][0]), (family, k)
        assert [w[0] for w in want] == [OK, OK, NO_VALID_POINTS]
    ctx.close()


@pytest.mark.parametrize("handoff", [0, 1], ids=["reference", "keep"])
@pytest.mark.parametrize("options", list(TABLE_OPTIONS))
def test_candidates_equal_the_reference(capi, torch, O, synth, arith, options, handoff):
    """semi-dense tracking over 3 levels from seeds, over the tables uwt_obtain_candidate_points gives, both schedules"""
    weights, sampler = TABLE_OPTIONS[options]
    n = 3
    seeds = SC.seeds(O, n)
    ref, tgt = SC.pair_slots(n)
    for schedule, over in SCHEDULES.items():
        ctx = make_ctx(capi, synth, n, **over)
        want = []
        for k in range(n):
            tables = {l: ctx.obtain_candidate_points(int(ref[k]), l, 20.0)[0] for l in range(3)}
            key = ("cand",) + tuple(tables[l].tobytes() for l in range(3))
            want.append(want_bits(SC.expect(O, synth, arith, k, seeds[k], bool(handoff), tables=tables, tables_key=hash(key),
                                            **dict(over, weights=weights or 0, sampler=sampler or 0))))
        assert all(w[1] == OK for w in want)
        for family in ("candidates_sync", "candidates_async"):
            got = bits(*run(capi, torch, ctx, family, n, seeds, handoff, weights=weights, sampler=sampler))
            print(options, schedule, family, [g[1:] for g in got], [w[1:] for w in want])
            assert got == want, (schedule, family)
        ctx.close()


# ---- I. the chains ---------------------------------------------------------------------------------------------------------------------
CW, CH = 256, 240
CAP = 2048


def chain_ctx(capi, synth, n):
    frames = [f for s in range(n) for f in synth.render_pair(CW, CH, *TR.INTR[(CW, CH)], seed=31 + 10 * s)[:2]]
    ctx = capi.Context(capi.default_params(CW, CH, *TR.INTR[(CW, CH)], max_frames=2 * n, max_pairs=n))
    ctx.upload_frames(0, np.stack(frames))
    ctx.build_pyramids(0, 2 * n)
    ctx.apply_gradient(0, 2 * n)
    return ctx


def chain_set(torch, n):
    i32 = dict(dtype=torch.int32, device="cuda")
    s = dict(poses=torch.full((n, 7), SENTINEL, **i32), stats=torch.full((n, 4), SENTINEL, **i32), info=torch.full((n, 8), SENTINEL, **i32),
             good=torch.full((n, CAP, 3), SENTINEL, **i32), kept_prev=torch.full((n, CAP, 8), SENTINEL, **i32),
             kept_cur=torch.full((n, CAP, 8), SENTINEL, **i32), n_matches=torch.full((n,), SENTINEL, **i32))
    torch.cuda.synchronize()
    return s


def chain_fetch(torch, s):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in s.items()}


CHAIN_SCENES = 6
_chain_frames = []


def chain_ctx20(capi, synth):
    """CHAIN_SCENES rendered pairs resident (scene s: slots 2s, 2s + 1), room for 20 pairs per call"""
    if not _chain_frames:
        _chain_frames.extend(f for s in range(CHAIN_SCENES) for f in synth.render_pair(CW, CH, *TR.INTR[(CW, CH)], seed=31 + 10 * s)[:2])
    ctx = capi.Context(capi.default_params(CW, CH, *TR.INTR[(CW, CH)], max_frames=2 * CHAIN_SCENES, max_pairs=20))
    ctx.upload_frames(0, np.stack(_chain_frames))
    ctx.build_pyramids(0, 2 * CHAIN_SCENES)
    ctx.apply_gradient(0, 2 * CHAIN_SCENES)
    return ctx


def chain_slots(n):
    k = np.arange(n) % CHAIN_SCENES
    return (2 * k).astype(np.int32), (2 * k + 1).astype(np.int32)


def chain_io(s):
    return {k: v.data_ptr() for k, v in s.items()}


def chain_fns(ctx, detector):
    """(unseeded async, seeded async, seeded sync) of a detector"""
    if detector == "surf":
        return ctx.tracking_batch_async, ctx.tracking_batch_seeded_async, ctx.tracking_batch_seeded
    return ctx.tracking_orb_batch_async, ctx.tracking_orb_batch_seeded_async, ctx.tracking_orb_batch_seeded


@pytest.mark.one_arith
@pytest.mark.parametrize("detector", ["surf", "orb"])
def test_chain_null_and_identity_seeds_equal_the_unseeded_entry(capi, torch, synth, detector):
    """test A for the two chain entries at 256 x 240: the unseeded call, null seeds under handoff 0 and explicit identity seeds (seeds and
    a gate in k_init_state, an identity row loaded by first_state) give the same bytes in EVERY io output, on 1, 2, 5 and 20 pairs"""
    ctx = chain_ctx20(capi, synth)
    unseeded_fn, seeded_fn, _ = chain_fns(ctx, detector)
    for n in (1, 2, 5, 20):
        ref, tgt = chain_slots(n)
        ident = torch.from_numpy(np.tile(IDENTITY, (n, 1))).cuda()
        a, b, c = chain_set(torch, n), chain_set(torch, n), chain_set(torch, n)
        unseeded_fn(ref, tgt, chain_io(a), cap=CAP)
        seeded_fn(ref, tgt, chain_io(b), cap=CAP, d_seeds_ptr=None, handoff=0)
        seeded_fn(ref, tgt, chain_io(c), cap=CAP, d_seeds_ptr=ident.data_ptr(), handoff=0)
        ctx.sync()
        A, B, Cc = chain_fetch(torch, a), chain_fetch(torch, b), chain_fetch(torch, c)
        assert (A["n_matches"] > 0).all() and not (A["poses"] == SENTINEL).all(axis=1).any()
        for k in A:
            assert A[k].tobytes() == B[k].tobytes(), (detector, n, k, "null seeds")
            assert A[k].tobytes() == Cc[k].tobytes(), (detector, n, k, "identity seeds")
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("detector", ["surf", "orb"])
@pytest.mark.parametrize("n", [3, 20])
def test_chain_bad_seed_fails_its_pair_alone(capi, torch, O, synth, detector, n):
    """test E for the chains, device and synchronous forms: a seed with a non-finite entry in the middle of 3 and of 20 pairs gives that
    pair {INVALID_ARG, 0, 0, 0} and the identity; every other byte of every output is that of the call with a good seed in its place;
    the synchronous form returns UWT_ERR_PAIR_FAILED (comparisons of calls of the library)"""
    ctx = chain_ctx20(capi, synth)
    _, seeded_fn, sync_fn = chain_fns(ctx, detector)
    ref, tgt = chain_slots(n)
    good = SC.seeds(O, n)
    mid = n // 2

    def device(seeds):
        d, s = torch.from_numpy(seeds).cuda(), chain_set(torch, n)
        seeded_fn(ref, tgt, chain_io(s), cap=CAP, d_seeds_ptr=d.data_ptr(), handoff=0)
        ctx.sync()
        return chain_fetch(torch, s)

    base = device(good)
    assert (base["stats"][:, 0] == OK).all(), base["stats"][:, 0]
    sync_base = sync_fn(ref, tgt, cap=CAP, seeds=good, raise_on_pair_failure=True)
    assert sync_base["status"] == OK and sync_base["poses"].tobytes() == base["poses"].view(np.float32).tobytes()
    assert sync_base["stats"].tobytes() == base["stats"].tobytes()
    for bad in SC.bad_seeds():
        seeds = good.copy()
        seeds[mid] = bad
        got = device(seeds)
        assert got["poses"][mid].tobytes() == IDENTITY.tobytes() and got["stats"][mid].tolist() == [INVALID_ARG, 0, 0, 0], (bad, got["stats"][mid])
        for k in got:
            rows = [i for i in range(n) if i != mid or k not in ("poses", "stats")]
            assert got[k][rows].tobytes() == base[k][rows].tobytes(), (k, bad)
        r = sync_fn(ref, tgt, cap=CAP, seeds=seeds)
        assert r["status"] == PAIR_FAILED
        assert r["poses"].tobytes() == got["poses"].view(np.float32).tobytes() and r["stats"].tobytes() == got["stats"].tobytes()
        assert r["info"].tobytes() == sync_base["info"].tobytes()
        for k in ("good", "kept_prev", "kept_cur"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(r[k], sync_base[k])), k
    seeds = good.copy()
    seeds[mid] = SC.bad_seeds()[3]
    with pytest.raises(capi.UwtError) as e:
        sync_fn(ref, tgt, cap=CAP, seeds=seeds, raise_on_pair_failure=True)
    assert e.value.status == PAIR_FAILED
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("detector", ["surf", "orb"])
def test_chain_refusals_enqueue_nothing(capi, torch, O, synth, detector):
    """seeds that share a byte with ANY output of io (the poses: equal and shifted by one row either way; the stats, the info, the good
    matches, both kept lists, the counts), a non-zero reserved word, handoff outside 0..1: UWT_ERR_INVALID_ARG, every output untouched"""
    n = 3
    ctx = chain_ctx20(capi, synth)
    _, seeded_fn, sync_fn = chain_fns(ctx, detector)
    ref, tgt = chain_slots(n)
    s = chain_set(torch, n)
    spare = torch.full((n + 2, 7), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    io = chain_io(s)
    io["poses"] = spare[1:n + 1].data_ptr()   # a row of room on either side of the poses
    overlaps = [io["poses"], io["poses"] + 28, io["poses"] - 28, io["poses"] + 28 * n - 4, io["stats"], io["stats"] + 16 * n - 4, io["info"] + 8,
                io["good"] + 12 * CAP, io["kept_prev"], io["kept_cur"] + 32 * CAP * n - 4, io["n_matches"], io["n_matches"] - 28 * n + 4]
    for ptr in overlaps:
        with pytest.raises(capi.UwtError) as e:
            seeded_fn(ref, tgt, io, cap=CAP, d_seeds_ptr=ptr, handoff=0)
        assert e.value.status == INVALID_ARG, hex(ptr)
    d_seeds = torch.from_numpy(SC.seeds(O, n)).cuda()
    for field, value in (("handoff", 2), ("handoff", -1), ("reserved", 1)):
        o = capi.seed_options()
        if field == "handoff":
            o.handoff = value
        else:
            o.reserved[2] = value
        with pytest.raises(capi.UwtError) as e:
            seeded_fn(ref, tgt, io, cap=CAP, d_seeds_ptr=d_seeds.data_ptr(), handoff=o)
        assert e.value.status == INVALID_ARG, (field, value)
        with pytest.raises(capi.UwtError) as e:
            sync_fn(ref, tgt, cap=CAP, seeds=SC.seeds(O, n), handoff=o)
        assert e.value.status == INVALID_ARG, (field, value, "synchronous")
    ctx.sync()
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in s.values()) and bool((spare == SENTINEL).all())
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("detector", ["surf", "orb"])
@pytest.mark.parametrize("n", [1, 3])
def test_chain_from_seeds(capi, torch, O, synth, detector, n):
    """System::Tracking on the device from seeds at 256 x 240: the front-end records (info, good, kept lists, counts) are the unseeded
    chain's bytes, the pose and stats those of uwt_estimate_pose_features_batch_seeded on the chain's kept key points under the same
    seeds; null seeds give the unseeded chain's bytes everywhere"""
    ctx = chain_ctx(capi, synth, n)
    ref, tgt = 2 * np.arange(n, dtype=np.int32), 2 * np.arange(n, dtype=np.int32) + 1
    seeds = SC.seeds(O, n)
    d_seeds = torch.from_numpy(seeds).cuda()
    unseeded_fn = ctx.tracking_batch_async if detector == "surf" else ctx.tracking_orb_batch_async
    seeded_fn = ctx.tracking_batch_seeded_async if detector == "surf" else ctx.tracking_orb_batch_seeded_async
    io = lambda s: {k: v.data_ptr() for k, v in s.items()}
    a, b, c = chain_set(torch, n), chain_set(torch, n), chain_set(torch, n)
    unseeded_fn(ref, tgt, io(a), cap=CAP)
    seeded_fn(ref, tgt, io(b), cap=CAP, d_seeds_ptr=None, handoff=0)
    seeded_fn(ref, tgt, io(c), cap=CAP, d_seeds_ptr=d_seeds.data_ptr(), handoff=0)
    ctx.sync()
    A, B, Cc = chain_fetch(torch, a), chain_fetch(torch, b), chain_fetch(torch, c)
    for k in A:
        assert A[k].tobytes() == B[k].tobytes(), (k, "null seeds")
        if k not in ("poses", "stats"):
            assert A[k].tobytes() == Cc[k].tobytes(), (k, "front end under seeds")
    info = A["info"].view(capi.TRACKING_INFO).reshape(-1)
    print(detector, n, "n_matches", info["n_matches"], "status", info["status"])
    assert (info["status"] == OK).all() and (info["n_matches"] > 0).all()
    kept = Cc["kept_prev"].view(capi.KEYPOINT).reshape(n, CAP)
    kps = [np.stack([kept[i]["x"], kept[i]["y"]], 1)[:min(int(info["n_matches"][i]), 200)].astype(np.float32) for i in range(n)]
    poses, stats = ctx.estimate_pose_features_batch_seeded(ref, tgt, kps, seeds, 0)
    got = bits(Cc["poses"].view(np.float32), [dict(status=r["status"], iterations=r["iterations"], n_valid=r["n_valid"], error=r["error"])
                                              for r in Cc["stats"].view(capi.STATS).reshape(-1)])
    assert got == bits(poses, stats)
    assert all(g[0] != u for g, u in zip(got, [A["poses"][i].tobytes() for i in range(n)]))   # the seed took effect
    # refusal: the seeds are io's pose buffer
    with pytest.raises(capi.UwtError) as e:
        seeded_fn(ref, tgt, io(c), cap=CAP, d_seeds_ptr=c["poses"].data_ptr(), handoff=0)
    assert e.value.status == INVALID_ARG
    # a seed with a non-finite entry fails its pair alone: {INVALID_ARG, 0, 0, 0} and the identity, the rest of the call as before
    mid = n // 2
    bad = seeds.copy()
    bad[mid] = SC.bad_seeds()[2]
    d_bad = torch.from_numpy(bad).cuda()
    e_ = chain_set(torch, n)
    seeded_fn(ref, tgt, io(e_), cap=CAP, d_seeds_ptr=d_bad.data_ptr(), handoff=0)
    ctx.sync()
    E = chain_fetch(torch, e_)
    assert E["poses"][mid].tobytes() == IDENTITY.tobytes() and E["stats"][mid].tolist() == [INVALID_ARG, 0, 0, 0]
    for k in E:
        rows = [i for i in range(n) if i != mid or k not in ("poses", "stats")]
        assert E[k][rows].tobytes() == Cc[k][rows].tobytes(), (k, "beside the refused pair")
    ctx.close()


@pytest.mark.one_arith
def test_chain_pair_the_front_end_fails_keeps_the_identity(capi, torch, O, synth):
    """pair 1 puts two unrelated scenes together: the front end finds no motion between them, and the pair has the unseeded chain's
    record and the identity pose whatever its seed row holds — here a row with a NaN"""
    ctx = chain_ctx(capi, synth, 2)
    ref, tgt = np.array([0, 0], np.int32), np.array([1, 3], np.int32)
    tp = capi.default_tracking_params()
    seeds = SC.seeds(O, 2)
    seeds[1] = SC.bad_seeds()[0]
    d_seeds = torch.from_numpy(seeds).cuda()
    io = lambda s: {k: v.data_ptr() for k, v in s.items()}
    a, b = chain_set(torch, 2), chain_set(torch, 2)
    ctx.tracking_batch_async(ref, tgt, io(a), params=tp, cap=CAP)
    ctx.tracking_batch_seeded_async(ref, tgt, io(b), params=tp, cap=CAP, d_seeds_ptr=d_seeds.data_ptr())
    ctx.sync()
    A, B = chain_fetch(torch, a), chain_fetch(torch, b)
    print("n_matches", A["n_matches"], "stats", A["stats"])
    for i in range(2):
        if A["n_matches"][i] == 0:
            assert A["poses"][i].tobytes() == B["poses"][i].tobytes() == IDENTITY.tobytes() and A["stats"][i].tobytes() == B["stats"][i].tobytes()
    assert A["n_matches"][1] == 0 and A["n_matches"][0] > 0
    assert B["poses"][0].tobytes() != A["poses"][0].tobytes()   # the good pair took its seed
    for k in A:
        if k not in ("poses", "stats"):
            assert A[k].tobytes() == B[k].tobytes(), k
    ctx.close()


# ---- J. guard bands ------------------------------------------------------------------------------------------------------------------
def test_guard_bands_around_seeds_and_outputs(capi, torch, O, synth):
    """every _async seeded entry and uwt_predict_seeds_device_async with the seeds and every output in an arena at exactly 4-byte
    alignment: no guard byte damaged, no output byte depending on the fill around the inputs; and the context's own scratch under
    uwt_debug_guards(4096) around one call of each family: zero damaged bytes"""
    n = 5
    seeds = SC.seeds(O, n)
    seeds[3] = SC.bad_seeds()[1]   # a refused pair's record is written inside the extents too
    ref, tgt = SC.pair_slots(n)
    be = GB.TorchBackend(torch)
    ctx = make_ctx(capi, synth, n, **SCHEDULES["fixed"])
    ctx.debug_guards(4096)

    def specs():
        return [GB.Buf("seeds", data=seeds, align=4, stride=28), GB.Buf("poses", nbytes=28 * n, align=4, stride=28),
                GB.Buf("stats", nbytes=16 * n, align=4, stride=16)]

    calls = {
        "dense": lambda a: ctx.track_batch_seeded_async(0, 2 * SC.N_SCENES, ref, tgt, a.ptr("poses"), a.ptr("stats"), d_seeds_ptr=a.ptr("seeds"), handoff=1),
        "features": lambda a: ctx.track_features_batch_seeded_async(ref, tgt, keypoints(n), a.ptr("poses"), a.ptr("stats"), a.ptr("seeds"), 0, weights=2),
        "candidates": lambda a: ctx.track_candidates_batch_seeded_async(ref, tgt, a.ptr("poses"), a.ptr("stats"), a.ptr("seeds"), 1),
    }
    for name, fn in calls.items():
        out = GB.run_twice(be, specs(), lambda a: (fn(a), ctx.sync()))
        st = np.frombuffer(out["stats"], np.int32).reshape(n, 4)
        assert st[3].tolist() == [INVALID_ARG, 0, 0, 0] and np.frombuffer(out["poses"], np.float32).reshape(n, 7)[3].tobytes() == IDENTITY.tobytes(), name
        assert ctx.debug_check_guards()[0] == 0, (name, ctx.debug_check_guards())
    # predict
    S = SC.seeds(O, 2 * n)
    pspecs = [GB.Buf("prev", data=S[:n], align=4, stride=28), GB.Buf("cur", data=S[n:], align=4, stride=28),
              GB.Buf("out", nbytes=28 * n, align=4, stride=28)]
    out = GB.run_twice(be, pspecs, lambda a: (ctx.predict_seeds_device_async(n, a.ptr("prev"), a.ptr("cur"), a.ptr("out")), ctx.sync()))
    assert out["out"] == SR.predict_seeds(O, S[:n], S[n:]).tobytes()
    ctx.debug_guards(0)
    ctx.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("detector", ["surf", "orb"])
def test_guard_bands_chain(capi, torch, O, synth, detector):
    n = 2
    ctx = chain_ctx(capi, synth, n)
    ctx.debug_guards(4096)
    ref, tgt = 2 * np.arange(n, dtype=np.int32), 2 * np.arange(n, dtype=np.int32) + 1
    seeds = SC.seeds(O, n)
    fn = ctx.tracking_batch_seeded_async if detector == "surf" else ctx.tracking_orb_batch_seeded_async
    specs = [GB.Buf("seeds", data=seeds, align=4, stride=28), GB.Buf("poses", nbytes=28 * n, align=4, stride=28),
             GB.Buf("stats", nbytes=16 * n, align=4, stride=16), GB.Buf("info", nbytes=32 * n, align=4, stride=32),
             GB.Buf("good", nbytes=12 * CAP * n, align=4, stride=12 * CAP), GB.Buf("kept_prev", nbytes=32 * CAP * n, align=4, stride=32 * CAP),
             GB.Buf("kept_cur", nbytes=32 * CAP * n, align=4, stride=32 * CAP), GB.Buf("n_matches", nbytes=4 * n, align=4, stride=4)]
    names = ("poses", "stats", "info", "good", "kept_prev", "kept_cur", "n_matches")
    GB.run_twice(GB.TorchBackend(torch), specs,
                 lambda a: (fn(ref, tgt, {k: a.ptr(k) for k in names}, cap=CAP, d_seeds_ptr=a.ptr("seeds"), handoff=0), ctx.sync()))
    assert ctx.debug_check_guards()[0] == 0, ctx.debug_check_guards()
    ctx.debug_guards(0)
    ctx.close()


# ---- K. the tool -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handoff", ["keep"])
def test_track_sequence_tool_keyframes_and_motion_model(capi, O, synth, arith, tmp_path, handoff):
    """tools/track_sequence.py --keyframe-interval 3 --motion-model constant on 7 rendered frames at 160 x 96: the poses and the
    trajectory it writes are those of this test's own sequence of synchronous seeded calls, seeds from seeded_ref.predict_seeds and the
    trajectory from the oracle's accumulation — plumbing only, no accuracy threshold"""
    import os
    import subprocess
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, N = 7, 3
    frames = synth.render_sequence(SC.W, SC.H, *SC.INTR, n, seed=5)[0]
    img_dir = tmp_path / "rgb"
    img_dir.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(f).save(img_dir / ("%06d.png" % i))
    out = tmp_path / "traj"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "track_sequence.py"), "--images", str(img_dir), "--fx", str(SC.INTR[0]),
                        "--fy", str(SC.INTR[1]), "--cx", str(SC.INTR[2]), "--cy", str(SC.INTR[3]), "--width", str(SC.W), "--height", str(SC.H),
                        "--keyframe-interval", str(N), "--motion-model", "constant", "--handoff", handoff, "--arith", arith, "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    poses, traj, keys = np.load(str(out) + "_poses.npy"), np.load(str(out) + "_trajectory.npy"), np.load(str(out) + "_keyframes.npy")
    assert keys.tolist() == [0, 0, 0, 3, 3, 3]
    ctx = capi.Context(capi.default_params(SC.W, SC.H, *SC.INTR, max_frames=n, max_pairs=1))
    ctx.upload_frames(0, np.stack(frames))
    ctx.build_pyramids(0, n)
    ctx.apply_gradient(0, n)
    want_p, want_t, seeded = [], [], 0
    for i in range(1, n):
        kf = N * ((i - 1) // N)
        if kf == i - 1:
            seed = None
        else:
            seed = SR.predict_seeds(O, IDENTITY[None] if kf == i - 2 else want_p[i - 3][None], want_p[i - 2][None])
            seeded += 1
        p, st = ctx.estimate_pose_batch_seeded([kf], [i], seed, handoff, raise_on_pair_failure=True)
        want_p.append(p[0].copy())
        want_t.append(O.accumulate_trajectory(p, start=None if kf == 0 else want_t[kf - 1])[0])
    ctx.close()
    assert seeded == 4
    assert poses.tobytes() == np.stack(want_p).tobytes() and traj.tobytes() == np.stack(want_t).tobytes()


@pytest.mark.one_arith
def test_track_sequence_live_chained_constant_motion(capi, synth, tmp_path):
    """--live --chained --motion-model constant: pair k's live alignment starts from pair k - 1's pose out of device memory; the poses
    are those of the synchronous seeded chain fed the previous pose through the host"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        tool = importlib.import_module("track_sequence")
    finally:
        sys.path.pop(0)
    intr = TR.INTR[(CW, CH)]
    frames = list(synth.render_sequence(CW, CH, *intr, 4, seed=3)[0])
    poses, stats, kept = tool.track_live_chained(CW, CH, intr, frames, None, motion_model="constant")
    T = importlib.import_module("uw-slam_amd.tracker")
    tracker = T.Tracker(False, max_frames=6)
    tracker.InitializePyramid(CW, CH, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    rm = T.RobustMatcher(tracker)
    fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
    want = []
    for k in range(3):
        T.TrackingBatch(tracker, rm, [(fr[k], fr[k + 1])], seeds=None if k == 0 else want[-1][None])
        want.append(np.asarray(fr[k].rigid_transformation_, np.float32).copy())
    tracker._ctx.close()
    assert poses.tobytes() == np.stack(want).tobytes()
    assert all(s["status"] == OK for s in stats)
