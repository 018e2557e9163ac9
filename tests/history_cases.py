"""The catalogue of the call-history tests (tests/test_history_cpu.py, tests/test_gpu_history.py, tools/exp/history_fuzz.py): every entry
family of include/uwt.h as an ACTION on ONE world, with its expectation from the CPU restatements alone, and the predecessors that
could leave something behind — EXCURSIONS (change a setting or a cache, work under it, put it back) and REFUSALS (calls that fail as
the header documents).  A helper of the tests, not a test.

The world: 256 x 240 with depth (tracking_ref.INTR), 4 levels, the reference early-exit schedule on levels 3..1, max_frames 8,
max_pairs 4.  Content X is four rendered pairs (pair i in slots 2 i, 2 i + 1, the pair's depth under both frames), content Y four other
pairs.  Everything is rendered once and never changed.

The contract under test: a call's result depends on its arguments and on the context state the header names — the
params, the Jacobian mode, the ORB pattern, the slot contents and which planes have been prepared — never on earlier calls.  So an
action's expectation is a function of (world, state) and of nothing else; `state` is a plain dict (BASE below) and every expectation is
cached per (action, the state keys it reads).  No expectation ever comes from a GPU run, a fresh context included.

An action: name, forms ("sync", "async" into device buffers, "host" into pinned memory behind a ticket), run(rig, form, state) -> a dict
of named byte strings or a Pending (collected later, with no wait in between), expected(world, state) -> the same dict, reaches (the
exported symbols the action calls, tests/test_history_cpu.py accounts for every export).  A comparison walks the EXPECTED keys: a pair
the restatement fails is compared by its status alone.
"""
import importlib

import numpy as np

import cloud_ref as CR
import depth_sweep_ref as DR
import gn_update_cases as GC
import gn_update_ref as GR
import match_ref as M
import metric_ref as MR
import orb_cases as OK_
import orb_ref as OR
import ransac_ref as R
import scale_ref as SCR
import seeded_ref as SR
import surf_ref as S
import tracking_orb_ref as TOR
import tracking_ref as TR
import warp_image_ref as WR

W, H = 256, 240
INTR = TR.INTR[(W, H)]
N_LEVELS, MAX_FRAMES, MAX_PAIRS = 4, 8, 4
SCHEDULES = {"early": dict(first_level=3, last_level=1, max_iters=50, early_exit=1),     # the reference's schedule (src/Tracker.cpp:364-372)
             "fixed": dict(first_level=3, last_level=0, max_iters=10, early_exit=0)}     # 4 levels x 10 evaluations, ends on level 0
FEATURES = dict(first_level=0, last_level=0, max_iters=10, early_exit=1, gain=1.0, z_factor=0.002, handoff_scale_t=1)   # the live call's locals
ARITH = {"opencv": 0, "legacy": 1}
OK, INVALID_ARG, NO_VALID_POINTS, CAPACITY, PAIR_FAILED = 0, 1, 2, 5, 6
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
THRESHOLD = 10.0          # ObtainCandidatePoints' threshold here (the synthetic texture saturates gradient_: 20 leaves coarse levels empty)
CAP = 2048                # rows per key-point / descriptor / match set
STATS = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("n_valid", "<i4"), ("error", "<f4")])
BASE = dict(weights=0, sampler=0, schedule="early", jacobian=0, pattern="default", content="X", pairs="fwd", ransac="default")
PAIR_LISTS = {"fwd": [(0, 1), (2, 3), (4, 5), (6, 7)], "swap": [(1, 0), (3, 2), (5, 4), (7, 6)], "other": [(0, 3), (2, 5), (4, 7), (6, 1)]}
RANSAC_SETS = {"default": dict(), "loose": dict(confidence=0.5, max_hypotheses=300)}
KP_COUNTS = [40, 12, 25, 60]


def state(arith, **over):
    """BASE under an arithmetic set ("opencv" / "legacy"), with keys replaced"""
    st = dict(BASE, arith=arith)
    for k in over:
        if k not in BASE:
            raise KeyError(k)
    st.update(over)
    return st


class World:
    """The inputs of every action, rendered and derived once; nothing in here is written after __init__ (derived inputs are cached)."""

    def __init__(self, O, synth):
        self.O = O
        self.gray, self.depth = {}, {}
        for name, base in (("X", 3101), ("Y", 3201)):
            pairs = [synth.render_pair(W, H, *INTR, seed=base + i, with_depth=True, max_t=0.012, max_deg=0.6)[:3] for i in range(4)]
            g = np.stack([f for r, t, _ in pairs for f in (r, t)])
            d = np.stack([dep for _, _, dep in pairs for _ in (0, 1)])
            g.setflags(write=False)
            d.setflags(write=False)
            self.gray[name], self.depth[name] = g, d
        rng = np.random.default_rng(20310)
        tw = rng.uniform(-1.0, 1.0, (4, 6)) * np.array([0.01, 0.01, 0.01, 0.004, 0.004, 0.004])
        self.seeds = np.stack([O.se3_exp(t.astype(np.float32)) for t in tw])
        self.bad_seeds = self.seeds[:3].copy()
        self.bad_seeds[1, 5] = np.nan
        self.kps = [rng.uniform([6, 6], [W - 7, H - 7], (n, 2)).astype(np.float32) for n in KP_COUNTS]
        self.residuals = rng.normal(0, 40, 1500).astype(np.float32)
        self.ls = (rng.normal(0, 30, (200, 6)).astype(np.float32), rng.integers(-255, 256, 200).astype(np.float32),
                   rng.uniform(0, 1, 200).astype(np.float32))
        Jd = self.ls[0].astype(np.float64)
        self.system = ((Jd.T @ Jd).astype(np.float32), (Jd.T @ self.ls[1].astype(np.float64)).astype(np.float32))
        self.twist = np.array([0.01, -0.02, 0.015, 0.004, -0.003, 0.002], np.float32)
        self.odd = np.ascontiguousarray(self.gray["X"][0][:101, :67])
        self.odd16 = np.ascontiguousarray(self.depth["X"][0][:101, :67])
        self.traj_poses = np.stack([O.se3_exp((tw[i % 4] * (1 + i)).astype(np.float32)) for i in range(6)])
        self._cache = {}

    # ---- parameters --------------------------------------------------------------------------------------------------------------
    def oracle(self, st):
        return MR.MetricOracle(self.O, metric=bool(st["jacobian"]))

    def params(self, st, **over):
        kw = dict(n_levels=N_LEVELS, has_depth=1, arith=ARITH[st["arith"]], weights=st["weights"], sampler=st["sampler"])
        kw.update(SCHEDULES[st["schedule"]])
        kw.update(over)
        return self.O.default_params(W, H, *INTR, **kw)

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def in_arith(self, st, fn):
        """fn() with the oracle's per-stage functions in the state's arithmetic set"""
        prev = self.O.set_arith(ARITH[st["arith"]])
        try:
            return fn()
        finally:
            self.O.set_arith(prev)

    # ---- planes and tables ---------------------------------------------------------------------------------------------------------
    def planes(self, content, slot):
        """(images, (gx, gy) per level, depths) of a slot on every level, in the oracle's current arithmetic set"""
        return self.cached(("planes", MR.current_arith(self.O), content, slot), lambda: SR.frame_planes(self.O, self.params(state("opencv")), self.gray[content][slot],
                                                                              self.depth[content][slot]))

    def level(self, lvl):
        return self.O.level_intrinsics(self.params(state("opencv")), lvl)

    def dense_table(self, content, slot, lvl):
        p = self.params(state("opencv"))
        return self.cached(("dense", MR.current_arith(self.O), content, slot, lvl), lambda: self.O.dense_points(self.planes(content, slot)[2][lvl], self.level(lvl).w,
                                                                                      self.level(lvl).h, lvl, p.depth_scale))

    def candidate_table(self, content, slot, lvl, threshold=THRESHOLD):
        def make():
            imgs, grads, deps = self.planes(content, slot)
            L = self.level(lvl)
            return self.O.candidate_points(self.O.gradient_mag(*grads[lvl]), deps[lvl], threshold, grid=(L.w, L.h))[0]
        return self.cached(("cand", MR.current_arith(self.O), content, slot, lvl, threshold), make)

    def patch_table(self, content, slot, kp):
        return self.O.patch_points(kp, self.depth[content][slot], W, H)[0]

    # ---- alignments ----------------------------------------------------------------------------------------------------------------
    def align(self, st, a, b, seed=None, keep=False, tables=None, tables_key=None, **over):
        """seeded_ref.align of slots (a, b) under the state: (status, pose, trace), cached"""
        key = ("align", st["arith"], st["weights"], st["sampler"], st["schedule"], st["jacobian"], st["content"], a, b,
               None if seed is None else np.asarray(seed, np.float32).tobytes(), bool(keep), tables_key, tuple(sorted(over.items())))
        c = st["content"]
        return self.cached(key, lambda: SR.align(self.oracle(st), self.params(st, **over), self.gray[c][a], self.gray[c][b], self.depth[c][a],
                                                 seed=seed, keep=keep, tables=tables))

    # ---- detection -----------------------------------------------------------------------------------------------------------------
    def surf(self, content, slot, cap=CAP):
        return TR.detect_describe(self.gray[content][slot], None, cap)

    def orb(self, content, slot, pattern="default", cap=CAP):
        return TOR.detect_describe(self.gray[content][slot], None, cap, self.pattern(pattern))

    @staticmethod
    def pattern(name):
        return None if name == "default" else OK_.second_pattern()

    def ransac_inputs(self):
        """two pairs of (matches, kp_prev, kp_cur): symMatches of content X's pairs 0 and 1 under SURF, the current key points of 40 % of
        the matches moved to random places (so that more than one hypothesis is needed and need(k) depends on the confidence)"""
        def make():
            out = []
            rng = np.random.default_rng(77031)
            for a, b in PAIR_LISTS["fwd"][:2]:
                (kq, dq), (kt, dt) = self.surf("X", a), self.surf("X", b)
                sym = M.match(dq, dt, 0.65)[0]
                k0, k1 = TR.xy(kq), TR.xy(kt).copy()
                bad = rng.permutation(len(sym))[:int(0.4 * len(sym))]
                k1[sym["train_idx"][bad]] = np.stack([rng.uniform(0, W, bad.size), rng.uniform(0, H, bad.size)], 1).astype(np.float32)
                out.append((sym, k0, k1))
            return out
        return self.cached("ransac_inputs", make)


# ---- results as named byte strings -------------------------------------------------------------------------------------------------------
def stats_array(stats):
    """the per-pair dicts of the synchronous mirrors as STATS records"""
    out = np.zeros(len(stats), STATS)
    for i, s in enumerate(stats):
        out[i] = (s["status"], s["iterations"], s["n_valid"], np.float32(s["error"]))
    return out


def pair_out(poses, stats):
    """what a pose call returned: per pair its status, its pose and its uwt_stats"""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
    stats = np.ascontiguousarray(stats, STATS).reshape(-1)
    out = {}
    for i in range(len(stats)):
        out["pair%d.status" % i] = np.int32(stats[i]["status"]).tobytes()
        out["pair%d.pose" % i] = poses[i].tobytes()
        out["pair%d.stats" % i] = stats[i].tobytes()
    return out


def pair_want(results):
    """the same from seeded_ref.align results: everything of a pair that succeeds and of one refused for its seed, the status alone of a
    pair that fails inside the alignment (what is left in its pose and its counts is not part of the contract)"""
    out = {}
    for i, (status, pose, trace) in enumerate(results):
        out["pair%d.status" % i] = np.int32(status).tobytes()
        if status == OK or (status == INVALID_ARG and not trace):
            rec = np.zeros((), STATS)
            st = SR.stats_of(status, trace)
            rec["status"], rec["iterations"], rec["n_valid"] = st[:3]
            rec["error"] = np.uint32(st[3]).view(np.float32)
            out["pair%d.pose" % i] = np.asarray(pose, np.float32).tobytes()
            out["pair%d.stats" % i] = rec.tobytes()
    return out


def first_difference(got, want):
    """(key, byte offset) of the first expected output `got` does not have bit for bit, or None"""
    for k in want:
        g, w = got.get(k), want[k]
        if g is None:
            return k, -1
        if g != w:
            if len(g) != len(w):
                return k, min(len(g), len(w))
            return k, next(i for i in range(len(w)) if g[i] != w[i])
    return None


def rows(name, arrays):
    """a list of per-item arrays as outputs name0, name1, ..."""
    return {"%s%d" % (name, i): np.ascontiguousarray(a).tobytes() for i, a in enumerate(arrays)}


class Pending:
    """the results of an asynchronous call, read when collect() is called: nothing waits before"""

    def __init__(self, rig, fetch, wait=None):
        self.rig, self.fetch, self.wait = rig, fetch, wait

    def collect(self):
        (self.wait or self.rig.ctx.sync)()
        return self.fetch()


def collect(x):
    return x.collect() if isinstance(x, Pending) else x


# ---- the context a catalogue runs on (GPU only) ------------------------------------------------------------------------------------------
class Block:
    def __init__(self, t, nbytes):
        self.t, self.ptr, self.nbytes = t, t.data_ptr(), nbytes

    def read(self, dtype=np.uint8):
        return self.t[:self.nbytes].cpu().numpy().view(dtype)


class Pool:
    """Device memory for the asynchronous forms, made and zeroed once: taking a block launches nothing and waits for nothing (a torch
    allocation or fill between two calls would run on torch's stream and be followed by a device-wide wait).  Blocks rotate through
    the ring; it is far larger than what the results of a few outstanding calls take."""

    def __init__(self, torch, nbytes=96 << 20):
        self.t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.at, self.nbytes = 0, nbytes

    def take(self, nbytes):
        asked, nbytes = int(nbytes), (int(nbytes) + 255) & ~255
        if self.at + nbytes > self.nbytes:
            self.at = 0
        b = Block(self.t[self.at:self.at + nbytes], asked)
        self.at += nbytes
        return b


class Rig:
    """One long-lived context with content X resident and every plane prepared, and the device and pinned constants of the forms"""

    def __init__(self, capi, world, tuning=None):
        import torch
        self.capi, self.world, self.torch = capi, world, torch
        p = capi.default_params(W, H, *INTR, n_levels=N_LEVELS, has_depth=1, max_frames=MAX_FRAMES, max_pairs=MAX_PAIRS, **SCHEDULES["early"])
        self.ctx = capi.Context(p, tuning=tuning)
        self.base_params = {k: getattr(p, k) for k in ("first_level", "last_level", "max_iters", "early_exit", "weights", "sampler", "arith")}
        self.pinned = {}
        for c in ("X", "Y"):
            g, d = capi.pinned_empty(world.gray[c].shape, np.uint8), capi.pinned_empty(world.depth[c].shape, np.uint16)
            g[...], d[...] = world.gray[c], world.depth[c]
            self.pinned[c] = (g, d)
        self.h_results = [(capi.pinned_empty((MAX_PAIRS, 7), np.float32), capi.pinned_empty((MAX_PAIRS, 4), np.int32)) for _ in range(8)]
        self.h_next = 0
        self.const = {}
        self.pool = Pool(torch)
        self.load("X")

    def device(self, name, make):
        """a constant input in device memory, uploaded once (before any call it could interleave with: made on first use, waited for)"""
        if name not in self.const:
            self.ctx.sync()
            t = self.torch.from_numpy(np.ascontiguousarray(make()).view(np.uint8).reshape(-1).copy()).cuda()
            self.torch.cuda.synchronize()
            self.const[name] = t
        return self.const[name].data_ptr()

    def load(self, content, how="sync"):
        """`content` into slots 0..7 and every plane prepared (the baseline's "which planes have been prepared")"""
        if how == "sync":
            self.ctx.upload_frames(0, self.world.gray[content], self.world.depth[content])
        else:
            self.ctx.upload_frames_async(0, *self.pinned[content])
        self.ctx.build_pyramids(0, MAX_FRAMES)
        self.ctx.apply_gradient(0, MAX_FRAMES)

    def set_schedule(self, name):
        self.ctx.update_params(**SCHEDULES[name])

    def close(self):
        self.ctx.sync()
        self.ctx.close()


class Action:
    def __init__(self, name, run, expected, forms=("sync",), reaches=(), reads=(), outputs=None):
        self.name, self.run, self._expected, self.forms, self.reaches, self.reads = name, run, expected, tuple(forms), tuple(reaches), tuple(reads)
        self.outputs = outputs or {}   # {form: the prefixes of the outputs that form delivers}; a form not named delivers them all

    def expected(self, world, st, form=None):
        """every output's expectation, or those the given form delivers"""
        key = ("expected", self.name, st["arith"]) + tuple(st[k] for k in self.reads)
        want = world.cached(key, lambda: world.in_arith(st, lambda: self._expected(world, st)))
        if form in self.outputs:
            want = {k: v for k, v in want.items() if k.startswith(self.outputs[form])}
            assert want
        return want


ACTIONS = []


def action(name, forms=("sync",), reaches=(), reads=(), outputs=None):
    def add(pair):
        run, expected = pair()
        ACTIONS.append(Action(name, run, expected, forms, reaches, reads, outputs))
        return pair
    return add


def slots_of(pairs):
    return np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)


POSE_READS = ("weights", "sampler", "schedule", "jacobian", "content", "pairs")
DENSE_SYNC = ("uwt_estimate_pose_batch",)


# ---- dense alignment ---------------------------------------------------------------------------------------------------------------------
def dense(n, handoff=None):
    """estimate_pose_batch / track_batch_async / track_batch_host_async on the first n pairs of the state's list; handoff 0 / 1: the
    seeded entries from the world's seeds"""
    seeded = handoff is not None

    def run(rig, form, st):
        ctx, (ref, tgt) = rig.ctx, slots_of(PAIR_LISTS[st["pairs"]][:n])
        if form == "sync":
            if seeded:
                return pair_out(*_sync(ctx.estimate_pose_batch_seeded(ref, tgt, rig.world.seeds[:n], handoff)))
            return pair_out(*_sync(ctx.estimate_pose_batch(ref, tgt)))
        if form == "host":
            hp, hs = (a[:n] for a in rig.h_results[rig.h_next % len(rig.h_results)])   # (a ring: results are collected a few calls later)
            rig.h_next += 1
            ticket = ctx.track_batch_host_async(0, MAX_FRAMES, ref, tgt, hp, hs)
            return Pending(rig, lambda: pair_out(np.array(hp), np.array(hs).view(STATS).reshape(-1)), wait=lambda: ctx.wait_ticket(ticket))
        dp, ds = rig.pool.take(n * 28), rig.pool.take(n * 16)
        if seeded:
            ctx.track_batch_seeded_async(0, MAX_FRAMES, ref, tgt, dp.ptr, ds.ptr, d_seeds_ptr=rig.device("seeds", lambda: rig.world.seeds),
                                         handoff=handoff)
        else:
            ctx.track_batch_async(0, MAX_FRAMES, ref, tgt, dp.ptr, ds.ptr)
        return Pending(rig, lambda: pair_out(dp.read(np.float32)[:n * 7], ds.read(STATS)[:n]))

    def expected(world, st):
        return pair_want([world.align(st, a, b, world.seeds[i] if seeded else None, bool(handoff))
                          for i, (a, b) in enumerate(PAIR_LISTS[st["pairs"]][:n])])

    return run, expected


def _sync(res):
    poses, stats = res
    return poses, stats_array(stats)


for _n in (1, 3, 4):
    action("dense_%d" % _n, ("sync", "async") + (("host",) if _n == 3 else ()), DENSE_SYNC + ("uwt_track_batch_async",) +
           (("uwt_track_batch_host_async", "uwt_wait_ticket") if _n == 3 else ()), POSE_READS)(lambda n=_n: dense(n))
for _h in (0, 1):
    action("dense_seeded_h%d" % _h, ("sync", "async"), ("uwt_estimate_pose_batch_seeded", "uwt_track_batch_seeded_async",
                                                        "uwt_default_seed_options"), POSE_READS)(lambda h=_h: dense(3, h))


def dense_under(over):
    """the dense calls on three pairs under other weights or the other sampler: the action sets them (uwt_update_params), calls, and puts
    the state's own back — so the robust scale's histograms, scales and tickets run as a successor of every predecessor, refusals included,
    and in the asynchronous form (whose results are read later; the parameters go back behind the enqueued call)"""
    run_plain, expected_plain = dense(3)

    def run(rig, form, st):
        rig.ctx.update_params(**over)
        try:
            return run_plain(rig, form, st)
        finally:
            rig.ctx.update_params(weights=st["weights"], sampler=st["sampler"])

    def expected(world, st):
        return expected_plain(world, dict(st, **over))

    return run, expected


for _name, _over in (("dense_tukey", dict(weights=1)), ("dense_huber", dict(weights=2)), ("dense_bilinear", dict(sampler=1))):
    action(_name, ("sync", "async"), DENSE_SYNC + ("uwt_track_batch_async", "uwt_update_params", "uwt_get_params"),
           POSE_READS)(lambda o=_over: dense_under(o))


@action("pose_points", reaches=("uwt_estimate_pose_points",), reads=("weights", "sampler", "schedule", "jacobian", "content"))
def _pose_points():
    """uwt_estimate_pose_points of slots (0, 1) over every third row of the dense tables of the iterated levels"""
    def tables(world, st):
        q = SCHEDULES[st["schedule"]]
        return {l: world.dense_table(st["content"], 0, l)[::3] for l in range(q["last_level"], q["first_level"] + 1)}

    def run(rig, form, st):
        pose, stats = rig.ctx.estimate_pose_points(0, 1, tables(rig.world, st))
        return pair_out(pose, stats_array([stats]))

    def expected(world, st):
        return pair_want([world.align(st, 0, 1, tables=tables(world, st), tables_key="third")])
    return run, expected


# ---- the batched table calls -------------------------------------------------------------------------------------------------------------
def table_call(kind, variant):
    """kind "features" / "candidates"; variant "plain", "opt" (Huber over the bilinear sampler, the call's own) or "seeded" (handoff 1)"""
    n = 3
    opt = dict(weights=2, sampler=1) if variant == "opt" else {}
    seeded = variant == "seeded"

    def run(rig, form, st):
        ctx, world = rig.ctx, rig.world
        ref, tgt = slots_of(PAIR_LISTS[st["pairs"]][:n])
        kps = world.kps[:n]
        lead = (ref, tgt, kps) if kind == "features" else (ref, tgt)
        extra = {} if kind == "features" else dict(threshold=THRESHOLD)
        if form == "sync":
            if seeded:
                fn = ctx.estimate_pose_features_batch_seeded if kind == "features" else ctx.estimate_pose_candidates_batch_seeded
                return pair_out(*_sync(fn(*lead, seeds=world.seeds[:n], handoff=1, **extra)))
            fn = ctx.estimate_pose_features_batch if kind == "features" else ctx.estimate_pose_candidates_batch
            return pair_out(*_sync(fn(*lead, **extra, **({k: v for k, v in opt.items()}))))
        dp, ds = rig.pool.take(n * 28), rig.pool.take(n * 16)
        if seeded:
            fn = ctx.track_features_batch_seeded_async if kind == "features" else ctx.track_candidates_batch_seeded_async
            fn(*lead, dp.ptr, ds.ptr, d_seeds_ptr=rig.device("seeds", lambda: world.seeds), handoff=1, **extra)
        else:
            fn = ctx.track_features_batch_async if kind == "features" else ctx.track_candidates_batch_async
            fn(*lead, dp.ptr, ds.ptr, **extra, **opt)
        return Pending(rig, lambda: pair_out(dp.read(np.float32)[:n * 7], ds.read(STATS)[:n]))

    def expected(world, st):
        out = []
        ws = dict(weights=opt.get("weights", 0), sampler=opt.get("sampler", 0))
        for i, (a, b) in enumerate(PAIR_LISTS[st["pairs"]][:n]):
            seed = world.seeds[i] if seeded else None
            if kind == "features":
                over = dict(FEATURES, **ws)
                if st["jacobian"]:
                    over["z_factor"] = 1.0   # the live call's z_factor in metric mode (include/uwt.h "the metric Jacobian")
                pts = world.patch_table(st["content"], a, world.kps[i])
                out.append(world.align(st, a, b, seed, seeded, tables={0: pts}, tables_key=("patch", i), **over))
            else:
                q = SCHEDULES[st["schedule"]]
                tables = {l: world.candidate_table(st["content"], a, l) for l in range(q["last_level"], q["first_level"] + 1)}
                out.append(world.align(st, a, b, seed, seeded, tables=tables, tables_key="cand", **ws))
        return pair_want(out)

    return run, expected


_TABLE_REACH = {
    ("features", "plain"): ("uwt_estimate_pose_features_batch", "uwt_track_features_batch_async"),
    ("features", "opt"): ("uwt_estimate_pose_features_batch_opt", "uwt_track_features_batch_opt_async", "uwt_default_table_options"),
    ("features", "seeded"): ("uwt_estimate_pose_features_batch_seeded", "uwt_track_features_batch_seeded_async"),
    ("candidates", "plain"): ("uwt_estimate_pose_candidates_batch", "uwt_track_candidates_batch_async"),
    ("candidates", "opt"): ("uwt_estimate_pose_candidates_batch_opt", "uwt_track_candidates_batch_opt_async"),
    ("candidates", "seeded"): ("uwt_estimate_pose_candidates_batch_seeded", "uwt_track_candidates_batch_seeded_async"),
}
for (_k, _v), _r in _TABLE_REACH.items():
    # (the plain candidates call refuses a context with weights or the bilinear sampler: its expectation reads neither)
    action("%s_%s" % (_k, _v), ("sync", "async"), _r, ("schedule", "jacobian", "content", "pairs") if _k == "candidates" else
           ("jacobian", "content", "pairs"))(lambda k=_k, v=_v: table_call(k, v))


# ---- the point producers -----------------------------------------------------------------------------------------------------------------
@action("candidate_points", reaches=("uwt_obtain_candidate_points_batch", "uwt_obtain_candidate_points", "uwt_gradient_magnitude"),
        reads=("content",))
def _candidate_points():
    def run(rig, form, st):
        tabs, cnt = rig.ctx.obtain_candidate_points_batch(0, 4, 1, THRESHOLD)
        one, n = rig.ctx.obtain_candidate_points(5, 0, THRESHOLD)
        return dict(rows("batch", tabs), counts=np.asarray(cnt, np.int32).tobytes(), one=one.tobytes(), n=np.int32(n).tobytes(),
                    mag=rig.ctx.gradient_magnitude(2, 2).tobytes())

    def expected(world, st):
        c = st["content"]
        tabs = [world.candidate_table(c, s, 1) for s in range(4)]
        one = world.candidate_table(c, 5, 0)
        return dict(rows("batch", tabs), counts=np.array([len(t) for t in tabs], np.int32).tobytes(), one=one.tobytes(),
                    n=np.int32(len(one)).tobytes(), mag=world.O.gradient_mag(*world.planes(c, 2)[1][2]).tobytes())
    return run, expected


@action("patch_points", reaches=("uwt_obtain_patch_points_batch", "uwt_obtain_patch_points", "uwt_add_patch_points"), reads=("content",))
def _patch_points():
    def seeds_of(world, c):
        return world.dense_table(c, 0, 0)[::997][:50]

    def run(rig, form, st):
        w = rig.world
        tabs, cnt = rig.ctx.obtain_patch_points_batch([0, 2, 4], w.kps[:3])
        one, n = rig.ctx.obtain_patch_points(6, w.kps[3])
        add, na = rig.ctx.add_patch_points(0, seeds_of(w, st["content"]), 5)
        return dict(rows("batch", tabs), counts=np.asarray(cnt, np.int32).tobytes(), one=one.tobytes(), n=np.int32(n).tobytes(),
                    add=add.tobytes(), n_add=np.int32(na).tobytes())

    def expected(world, st):
        c = st["content"]
        tabs = [world.patch_table(c, s, world.kps[i]) for i, s in enumerate((0, 2, 4))]
        one = world.patch_table(c, 6, world.kps[3])
        add, na = world.O.add_patch_points(seeds_of(world, c), W, H, 5)
        return dict(rows("batch", tabs), counts=np.array([len(t) for t in tabs], np.int32).tobytes(), one=one.tobytes(),
                    n=np.int32(len(one)).tobytes(), add=add.tobytes(), n_add=np.int32(na).tobytes())
    return run, expected


# ---- the per-stage entries ---------------------------------------------------------------------------------------------------------------
def _evaluation(world, st, lvl, pose, sampler=0):
    """(J, r, idx, grid size) of slots (0, 1) at a level under a pose, from the oracle's stage functions"""
    c = st["content"]
    imgs, grads, deps = world.planes(c, 0)
    timg = world.planes(c, 1)[0]
    L = world.level(lvl)
    p = world.params(st)
    pts = world.dense_table(c, 0, lvl)
    J, r, idx = world.oracle(st).residual_jacobian_ex(imgs[lvl], timg[lvl], grads[lvl][0], grads[lvl][1], pts, world.O.warp(pts, pose, L), L,
                                                      p.z_factor, p.angle_factor, sampler)
    return J, r, idx, L.w * L.h


def _evaluation_out(out, weighted=False):
    v = out["valid"].astype(bool)
    d = dict(valid=out["valid"].tobytes(), n_valid=np.int32(out["n_valid"]).tobytes(), r=out["r"][v].tobytes(), J=out["J"][v].tobytes())
    if weighted:
        d.update(w=out["w"][v].tobytes(), inv_mad=np.float32(out["inv_mad"]).tobytes(), A=out["A"].astype(np.float32).tobytes(),
                 b=(-out["jtr"]).astype(np.float32).tobytes())
    else:
        d.update(sum_r2=np.int64(out["sum_r2"]).tobytes())
    return d


@action("residual_jacobian", reaches=("uwt_residual_jacobian", "uwt_level_info"), reads=("jacobian", "content"))
def _residual_jacobian():
    """uwt_residual_jacobian of slots (0, 1) on level 1 under the first seed, with the dump and without"""
    def run(rig, form, st):
        full = rig.ctx.residual_jacobian(0, 1, 1, rig.world.seeds[0], dump=True)
        bare = rig.ctx.residual_jacobian(0, 1, 1, rig.world.seeds[0], dump=False)
        return dict(_evaluation_out(full), bare_n_valid=np.int32(bare["n_valid"]).tobytes(), bare_sum_r2=np.int64(bare["sum_r2"]).tobytes())

    def expected(world, st):
        J, r, idx, ng = _evaluation(world, st, 1, world.seeds[0])
        valid = np.zeros(ng, np.uint8)
        valid[idx] = 1
        s2 = np.int64((r.astype(np.int64) ** 2).sum()).tobytes()
        return dict(valid=valid.tobytes(), n_valid=np.int32(len(r)).tobytes(), r=r.tobytes(), J=J.tobytes(), sum_r2=s2,
                    bare_n_valid=np.int32(len(r)).tobytes(), bare_sum_r2=s2)
    return run, expected


@action("residual_jacobian_weighted", reaches=("uwt_residual_jacobian_weighted", "uwt_update_params", "uwt_get_params"),
        reads=("jacobian", "content"))
def _residual_jacobian_weighted():
    """uwt_residual_jacobian_weighted of slots (0, 1) on level 1 at the identity under Huber weights: the action sets the weights, calls
    and puts the context's own back (the entry reads the context's weights; under identity weights it has nothing to add)"""
    def run(rig, form, st):
        rig.ctx.update_params(weights=2)
        try:
            out = rig.ctx.residual_jacobian_weighted(0, 1, 1, IDENTITY)
        finally:
            rig.ctx.update_params(weights=st["weights"])
        return _evaluation_out(out, weighted=True)

    def expected(world, st):
        J, r, idx, ng = _evaluation(world, st, 1, IDENTITY)
        valid = np.zeros(ng, np.uint8)
        valid[idx] = 1
        inv_mad = SCR.scale(r, SCR.HUBER)[3]
        Wt = SCR.weights(SCR.HUBER, r, inv_mad)
        A, b = world.O.normal_equations(J, r, Wt, world.params(st).gain)
        return dict(valid=valid.tobytes(), n_valid=np.int32(len(r)).tobytes(), r=r.tobytes(), J=J.tobytes(), w=Wt.tobytes(),
                    inv_mad=np.float32(inv_mad).tobytes(), A=np.asarray(A, np.float32).tobytes(), b=np.asarray(b, np.float32).tobytes())
    return run, expected


@action("stage_algebra", reaches=("uwt_warp", "uwt_robust_weights", "uwt_ls_accumulate", "uwt_ls_accumulate_sse", "uwt_solve_delta",
                                  "uwt_se3_exp", "uwt_se3_mul", "uwt_se3_matrix", "uwt_se3_handoff"))
def _stage_algebra():
    """warp, robust_weights, ls_accumulate (both forms), solve_delta and the se3 functions on fixed inputs"""
    def run(rig, form, st):
        ctx, w = rig.ctx, rig.world
        J, r, wt = w.ls
        e = ctx.se3_exp(w.twist)
        wts, med, mad = ctx.robust_weights(w.residuals, kind=1)
        A, b, err, n = ctx.ls_accumulate(J, r, wt, divide=True)
        A4, b4, err4, n4 = ctx.ls_accumulate_sse(J, r, wt, divide=False, count_quirk=True)
        d, Ai, ok = ctx.solve_delta(*w.system)
        return dict(warp=ctx.warp(1, w.dense_table("X", 0, 1), w.seeds[1]).tobytes(), weights=wts.tobytes(),
                    med=np.float32(med).tobytes(), mad=np.float32(mad).tobytes(), A=A.tobytes(), b=b.tobytes(), err=np.float32(err).tobytes(),
                    n=np.int32(n).tobytes(), A4=A4.tobytes(), b4=b4.tobytes(), err4=np.float32(err4).tobytes(), n4=np.int32(n4).tobytes(),
                    delta=d.tobytes(), inverse=Ai.tobytes(), solvable=np.int32(ok).tobytes(), exp=e.tobytes(),
                    mul=ctx.se3_mul(e, w.seeds[2]).tobytes(), matrix=ctx.se3_matrix(e).tobytes(), handoff=ctx.se3_handoff(e, 0).tobytes(),
                    handoff_t=ctx.se3_handoff(e, 1).tobytes())

    def expected(world, st):
        O = world.O
        J, r, wt = world.ls
        e = O.se3_exp(world.twist)
        ls, ls4 = O.ls_new(), O.ls_new()
        for i in range(len(r)):
            O.ls_update(ls, J[i], r[i], wt[i])
        for k in range(0, len(r), 4):
            O.ls_update4(ls4, J[k:k + 4].T, r[k:k + 4], wt[k:k + 4], quirk_plus6=True)
        A, b, err, n = O.ls_finish(ls, divide=True)
        A4, b4, err4, n4 = O.ls_finish(ls4, divide=False)
        Ai, ok = O.inv6(world.system[0])
        return dict(warp=O.warp(world.dense_table("X", 0, 1), world.seeds[1], world.level(1)).tobytes(),
                    weights=O.tukey_weights(world.residuals).tobytes(), med=np.float32(O.median_mat(world.residuals)).tobytes(),
                    mad=np.float32(O.mad(world.residuals)).tobytes(), A=np.asarray(A, np.float32).tobytes(), b=np.asarray(b, np.float32).tobytes(),
                    err=np.float32(err).tobytes(), n=np.int32(n).tobytes(), A4=np.asarray(A4, np.float32).tobytes(),
                    b4=np.asarray(b4, np.float32).tobytes(), err4=np.float32(err4).tobytes(), n4=np.int32(n4).tobytes(),
                    delta=O.solve_delta(*world.system).tobytes(), inverse=np.asarray(Ai, np.float32).tobytes(), solvable=np.int32(ok).tobytes(),
                    exp=e.tobytes(), mul=O.se3_mul(e, world.seeds[2]).tobytes(), matrix=np.asarray(O.se3_matrix(e), np.float32).tobytes(),
                    handoff=O.se3_handoff(e, 0).tobytes(), handoff_t=O.se3_handoff(e, 1).tobytes())
    return run, expected


@action("stage_images", reaches=("uwt_halve_u8", "uwt_halve_u16", "uwt_resize_half_u8", "uwt_resize_half_u16", "uwt_half_size", "uwt_scharr3"))
def _stage_images():
    """halve_*, resize_half_* (an odd size) and scharr3 on images of content X given by the caller (no slot is read)"""
    def run(rig, form, st):
        ctx, w = rig.ctx, rig.world
        gx, gy = ctx.scharr3(w.odd)
        return dict(h8=ctx.halve_u8(w.gray["X"][2]).tobytes(), h16=ctx.halve_u16(w.depth["X"][2]).tobytes(), r8=ctx.resize_half_u8(w.odd).tobytes(),
                    r16=ctx.resize_half_u16(w.odd16).tobytes(), gx=gx.tobytes(), gy=gy.tobytes())

    def expected(world, st):
        O = world.O
        gx, gy = O.scharr3(world.odd)
        return dict(h8=O.halve_u8(world.gray["X"][2]).tobytes(), h16=O.halve_u16(world.depth["X"][2]).tobytes(), r8=O.resize_half_u8(world.odd).tobytes(),
                    r16=O.resize_half_u16(world.odd16).tobytes(), gx=gx.tobytes(), gy=gy.tobytes())
    return run, expected


GN_ARGS = dict(k=0, max_iters=50, early_exit=0, epsilon=1e-3, gain=50.0, general=0)


@action("gn_update_records", reaches=("uwt_gn_update_records",))
def _gn_update_records():
    """uwt_gn_update_records in the block form and in the tail form on nine designed records"""
    count = 9

    def run(rig, form, st):
        out = {}
        for f in (0, 1):
            recs = GC.fold_records(count)[None]
            states, active, tickets = rig.ctx.gn_update_records(f, recs, [GR.state()], count, **GN_ARGS)
            out.update({"state%d" % f: states.tobytes(), "active%d" % f: np.int32(active).tobytes(), "tickets%d" % f: tickets.tobytes()})
        return out

    def expected(world, st):
        out = {}
        for f in (0, 1):
            s, active = GR.update(world.O, np.asarray(GR.state(), GR.STATE_DTYPE).reshape(-1)[0], GC.fold_records(count), count,
                                  arith=st["arith"], block_form=f == 0, **GN_ARGS)[:2]
            out.update({"state%d" % f: np.asarray(s, GR.STATE_DTYPE).reshape(1).tobytes(), "active%d" % f: np.int32(1 if active else 0).tobytes(),
                        "tickets%d" % f: np.zeros(1, np.uint32).tobytes()})
        return out
    return run, expected


# ---- matching and RANSAC -----------------------------------------------------------------------------------------------------------------
def _descriptor_pairs(world, norm):
    if norm == "l2":
        return [(world.surf("X", a)[1], world.surf("X", b)[1]) for a, b in PAIR_LISTS["fwd"][:2]]
    return [(world.orb("X", a)[1], world.orb("X", b)[1]) for a, b in PAIR_LISTS["fwd"][:2]]


def _packed(world, norm):
    """the fixed-stride form of the descriptor pairs: (query [P, CAP, dim], n_query, train, n_train)"""
    pairs = _descriptor_pairs(world, norm)
    dim, dt = pairs[0][0].shape[1], pairs[0][0].dtype
    q, t = np.zeros((len(pairs), CAP, dim), dt), np.zeros((len(pairs), CAP, dim), dt)
    nq, nt = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
    for i, (a, b) in enumerate(pairs):
        q[i, :len(a)], t[i, :len(b)], nq[i], nt[i] = a, b, len(a), len(b)
    return q, nq, t, nt


def matching(norm):
    def run(rig, form, st):
        ctx, w = rig.ctx, rig.world
        P = 2
        if form == "sync":
            pairs = _descriptor_pairs(w, norm)
            out = rows("matches", ctx.match_descriptors_batch(pairs, ratio=0.65, cap=CAP))
            if norm == "l2":
                out.update(rows("knn", ctx.knn_match_batch(pairs, cap=CAP)))
            return out
        dm, dc = rig.pool.take(P * CAP * 12), rig.pool.take(P * 4)
        if form == "async":
            ctx.match_descriptors_batch_async(dm.ptr, dc.ptr, packed=w.cached(("packed", norm), lambda: _packed(w, norm)), ratio=0.65)
        else:   # "device": both sets already in device memory
            q, nq, t, nt = w.cached(("packed", norm), lambda: _packed(w, norm))
            ctx.match_descriptors_device_async(P, q.shape[2], CAP, rig.device("q" + norm, lambda: q), rig.device("nq" + norm, lambda: nq),
                                               rig.device("t" + norm, lambda: t), rig.device("nt" + norm, lambda: nt), dm.ptr, dc.ptr, ratio=0.65,
                                               norm=rig.capi.NORM_L2 if norm == "l2" else rig.capi.NORM_HAMMING)

        def fetch():
            cnt = dc.read(np.int32)[:P]
            m = dm.read(M.MATCH)[:P * CAP].reshape(P, CAP)
            return rows("matches", [m[i, :cnt[i]] for i in range(P)])
        return Pending(rig, fetch)

    def expected(world, st):
        res = [M.match(a, b, 0.65) for a, b in _descriptor_pairs(world, norm)]
        out = rows("matches", [r[0] for r in res])
        if norm == "l2":
            out.update(rows("knn", [r[1] for r in res]))
        return out

    return run, expected


action("match_l2", ("sync", "async", "device"), ("uwt_match_descriptors_batch", "uwt_knn_match_batch", "uwt_match_descriptors_batch_async",
                                                 "uwt_match_descriptors_device_async"),
       outputs=dict(**{"async": ("matches",), "device": ("matches",)}))(lambda: matching("l2"))
action("match_hamming", ("sync", "async", "device"), ("uwt_match_descriptors_batch", "uwt_match_descriptors_batch_async",
                                                      "uwt_match_descriptors_device_async"))(lambda: matching("hamming"))


def _ransac_out(res):
    out = {}
    for i, (mask, good, info) in enumerate(res):
        out["mask%d" % i] = np.ascontiguousarray(mask, np.uint8).tobytes()
        out["good%d" % i] = np.ascontiguousarray(good, M.MATCH).tobytes()
        out["info%d" % i] = np.array([int(info[k]) for k in ("status", "n_inliers", "best_hypothesis", "hypotheses_run")], np.int32).tobytes()
        out["F%d" % i] = np.asarray(info["F"], np.float64).tobytes()
    return out


@action("ransac", ("sync", "async"), ("uwt_ransac_inliers_batch", "uwt_ransac_inliers_batch_async", "uwt_default_ransac_params"), ("ransac",))
def _ransac():
    """uwt_ransac_inliers_batch* on two pairs with 40 % outliers, under the state's parameter set (the asynchronous form reads the
    matches from device memory)"""
    def run(rig, form, st):
        ctx, w, capi = rig.ctx, rig.world, rig.capi
        pairs = w.ransac_inputs()
        params = capi.default_ransac_params(**RANSAC_SETS[st["ransac"]])
        if form == "sync":
            return _ransac_out(ctx.ransac_inliers_batch(pairs, params=params, cap=CAP, kp_cap=CAP))
        P = len(pairs)
        mt, nm = np.zeros((P, CAP), M.MATCH), np.zeros(P, np.int32)
        for i, (m, _, _) in enumerate(pairs):
            mt[i, :len(m)], nm[i] = m, len(m)
        dmask, dgood, dcnt, dinfo = rig.pool.take(P * CAP), rig.pool.take(P * CAP * 12), rig.pool.take(P * 4), rig.pool.take(P * capi.RANSAC_INFO.itemsize)
        ctx.ransac_inliers_batch_async(rig.device("ransac_m", lambda: mt), rig.device("ransac_n", lambda: nm), CAP, [(a, b) for _, a, b in pairs],
                                       dmask.ptr, dgood.ptr, dcnt.ptr, dinfo.ptr, params=params, kp_cap=CAP)

        def fetch():
            cnt = dcnt.read(np.int32)[:P]
            mask, good = dmask.read()[:P * CAP].reshape(P, CAP), dgood.read(M.MATCH)[:P * CAP].reshape(P, CAP)
            info = dinfo.read(capi.RANSAC_INFO)[:P]
            return _ransac_out([(mask[i, :nm[i]], good[i, :cnt[i]], info[i]) for i in range(P)])
        return Pending(rig, fetch)

    def expected(world, st):
        return _ransac_out([R.ransac(m, a, b, **RANSAC_SETS[st["ransac"]]) for m, a, b in world.ransac_inputs()])
    return run, expected


# ---- detection and description ---------------------------------------------------------------------------------------------------------
def _detected_out(res):
    out = {}
    for i, (kp, desc) in enumerate(res):
        out["kp%d" % i], out["desc%d" % i] = np.ascontiguousarray(kp).tobytes(), np.ascontiguousarray(desc).tobytes()
    return out


def detect(kind):
    """uwt_surf_ / uwt_orb_detect_describe_batch* on slots 1 and 4"""
    slots, row, dt = [1, 4], (64, np.float32) if kind == "surf" else (32, np.uint8), None

    def run(rig, form, st):
        ctx = rig.ctx
        if form == "sync":
            fn = ctx.surf_detect_describe_batch if kind == "surf" else ctx.orb_detect_describe_batch
            return _detected_out(fn(slots, cap=CAP))
        F, width = len(slots), row[0] * np.dtype(row[1]).itemsize
        dk, dd, dc = rig.pool.take(F * CAP * 32), rig.pool.take(F * CAP * width), rig.pool.take(F * 4)
        fn = ctx.surf_detect_describe_batch_async if kind == "surf" else ctx.orb_detect_describe_batch_async
        fn(slots, dk.ptr, dd.ptr, dc.ptr, cap=CAP)

        def fetch():
            cnt = dc.read(np.int32)[:F]
            kp = dk.read(S.KEYPOINT)[:F * CAP].reshape(F, CAP)
            desc = dd.read(row[1])[:F * CAP * row[0]].reshape(F, CAP, row[0])
            return _detected_out([(kp[i, :cnt[i]], desc[i, :cnt[i]]) for i in range(F)])
        return Pending(rig, fetch)

    def expected(world, st):
        if kind == "surf":
            return _detected_out([world.surf(st["content"], s) for s in slots])
        return _detected_out([world.orb(st["content"], s, st["pattern"]) for s in slots])

    return run, expected


action("surf_detect", ("sync", "async"), ("uwt_surf_detect_describe_batch", "uwt_surf_detect_describe_batch_async"), ("content",))(lambda: detect("surf"))
action("orb_detect", ("sync", "async"), ("uwt_orb_detect_describe_batch", "uwt_orb_detect_describe_batch_async"),
       ("content", "pattern"))(lambda: detect("orb"))


@action("surf_stages", reaches=("uwt_surf_describe_batch", "uwt_surf_integral", "uwt_surf_response_layer"), reads=("content",))
def _surf_stages():
    """surf_describe_batch at the first 60 key points the restatement detects on slot 3, surf_integral and one response layer of slot 3"""
    def kin(world, c):
        k = world.surf(c, 3)[0][:60].copy()
        k["dir_x"], k["dir_y"] = 0.25, -7.0   # the direction is recomputed
        return k

    def run(rig, form, st):
        ctx = rig.ctx
        kp, desc = ctx.surf_describe_batch([3], [kin(rig.world, st["content"])])[0]
        resp = ctx.surf_response_layer(3, 1, 2)
        return dict(kp=kp.tobytes(), desc=desc.tobytes(), integral=ctx.surf_integral(3).tobytes(), absent=np.isnan(resp).tobytes(),
                    response=resp[~np.isnan(resp)].tobytes())

    def expected(world, st):
        img = world.gray[st["content"]][3]
        kp, desc = S.describe(img, kin(world, st["content"]), S.default_params())
        I = S.integral(img)
        resp = S.response_layer(I, 1, 2)[0]
        return dict(kp=kp.tobytes(), desc=desc.tobytes(), integral=np.ascontiguousarray(I, np.uint32).tobytes(), absent=np.isnan(resp).tobytes(),
                    response=np.ascontiguousarray(resp[~np.isnan(resp)], np.float64).tobytes())
    return run, expected


@action("orb_stages", reaches=("uwt_orb_describe_batch", "uwt_orb_layer", "uwt_orb_fast_scores", "uwt_orb_harris", "uwt_orb_layer_size"),
        reads=("content", "pattern"))
def _orb_stages():
    """orb_describe_batch at the first 80 key points the restatement detects on slot 2, and layer 2, its FAST scores and the Harris
    measure at its candidates"""
    def kin(world, c):
        k = world.orb(c, 2)[0][:80].copy()
        k["dir_x"], k["dir_y"] = 0.25, -7.0
        return k

    def cand(world, c):
        L = OR.layer(world.gray[c][2], 2)
        ys, xs, Hm = OR.layer_candidates(L, OR.default_params())
        return L, np.stack([xs, ys], 1).astype(np.int32), Hm

    def run(rig, form, st):
        ctx = rig.ctx
        kp, desc = ctx.orb_describe_batch([2], [kin(rig.world, st["content"])])[0]
        xy = rig.world.cached(("orb_cand", st["content"]), lambda: cand(rig.world, st["content"]))[1]
        return dict(kp=kp.tobytes(), desc=desc.tobytes(), layer=ctx.orb_layer(2, 2).tobytes(), fast=ctx.orb_fast_scores(2, 2).tobytes(),
                    harris=ctx.orb_harris(2, 2, xy).tobytes())

    def expected(world, st):
        c = st["content"]
        p = OR.default_params()
        kp, desc = OR.describe(np.ascontiguousarray(world.gray[c][2]), kin(world, c), p, world.pattern(st["pattern"]))
        L, xy, Hm = world.cached(("orb_cand", c), lambda: cand(world, c))
        return dict(kp=kp.tobytes(), desc=desc.tobytes(), layer=L.tobytes(),
                    fast=np.ascontiguousarray(OR.fast_scores(L, p["edge_threshold"], p["fast_threshold"]), np.int32).tobytes(),
                    harris=np.ascontiguousarray(Hm, np.int64).tobytes())
    return run, expected


# ---- the chains --------------------------------------------------------------------------------------------------------------------------
INFO_FIELDS = ("status", "used_provided", "n_kp_prev", "n_kp_cur", "n_symmetric", "n_matches", "best_hypothesis", "hypotheses_run")
CHAIN_PAIRS = [(0, 1), (1, 0)]   # the second pair takes what frame 1 kept in the first: a hand-over from the previous call's io


def _chain_out(r, i, tag):
    return {tag + "info": np.array([int(r["info"][i][k]) for k in INFO_FIELDS], np.int32).tobytes(), tag + "good": r["good"][i].tobytes(),
            tag + "kept_prev": r["kept_prev"][i].tobytes(), tag + "kept_cur": r["kept_cur"][i].tobytes(),
            tag + "pose": np.ascontiguousarray(r["poses"][i], np.float32).tobytes(), tag + "stats": np.ascontiguousarray(r["stats"][i]).tobytes()}


def chain(kind, seeded):
    """uwt_tracking_batch* / uwt_tracking_orb_batch*: pair (0, 1) detected, then pair (1, 0) from what frame 1 kept (min_matches 90 so
    that the kept records are used); seeded: from the world's seeds, handoff 1.  Synchronous: two calls, the key points through the host;
    asynchronous: two calls enqueued back to back, the second reading the first one's kept_cur and n_matches in device memory."""
    MIN = 90

    def tparams(capi):
        return (capi.default_tracking_params if kind == "surf" else capi.default_tracking_orb_params)(min_matches=MIN)

    def run(rig, form, st):
        ctx, capi, w = rig.ctx, rig.capi, rig.world
        tp = tparams(capi)
        names = {("surf", False): ("tracking_batch", "tracking_batch_async"), ("surf", True): ("tracking_batch_seeded", "tracking_batch_seeded_async"),
                 ("orb", False): ("tracking_orb_batch", "tracking_orb_batch_async"),
                 ("orb", True): ("tracking_orb_batch_seeded", "tracking_orb_batch_seeded_async")}[(kind, seeded)]
        if form == "sync":
            fn, out, prev = getattr(ctx, names[0]), {}, None
            for k, (a, b) in enumerate(CHAIN_PAIRS):
                extra = dict(seeds=w.seeds[k:k + 1], handoff=1) if seeded else {}
                r = fn([a], [b], prev=prev, params=tp, cap=CAP, **extra)
                out.update(_chain_out(r, 0, "call%d." % k))
                prev = [r["kept_cur"][0]]
            return out
        fn, sets = getattr(ctx, names[1]), []
        for k, (a, b) in enumerate(CHAIN_PAIRS):
            s = dict(poses=rig.pool.take(28), stats=rig.pool.take(16), info=rig.pool.take(32), good=rig.pool.take(CAP * 12),
                     kept_prev=rig.pool.take(CAP * 32), kept_cur=rig.pool.take(CAP * 32), n_matches=rig.pool.take(4))
            io = {name: blk.ptr for name, blk in s.items()}
            if sets:
                io["prev_kp"], io["n_prev"] = sets[-1]["kept_cur"].ptr, sets[-1]["n_matches"].ptr
            extra = dict(d_seeds_ptr=rig.device("seeds", lambda: w.seeds) + 28 * k, handoff=1) if seeded else {}
            fn([a], [b], io, params=tp, cap=CAP, **extra)
            sets.append(s)

        def fetch():
            out = {}
            for k, s in enumerate(sets):
                n = int(s["n_matches"].read(np.int32)[0])
                r = dict(info=s["info"].read(capi.TRACKING_INFO)[:1], good=[s["good"].read(M.MATCH)[:n]], kept_prev=[s["kept_prev"].read(S.KEYPOINT)[:n]],
                         kept_cur=[s["kept_cur"].read(S.KEYPOINT)[:n]], poses=s["poses"].read(np.float32)[:7].reshape(1, 7),
                         stats=s["stats"].read(STATS)[:1])
                out.update(_chain_out(r, 0, "call%d." % k))
            return out
        return Pending(rig, fetch)

    def expected(world, st):
        c = st["content"]
        out, prev = {}, None
        for k, (a, b) in enumerate(CHAIN_PAIRS):
            if kind == "surf":
                fe = TR.front_end(world.gray[c][a], world.gray[c][b], prev, min_matches=MIN, cap=CAP)
            else:
                fe = TOR.front_end(world.gray[c][a], world.gray[c][b], prev, min_matches=MIN, cap=CAP, pattern=world.pattern(st["pattern"]))
            over = dict(FEATURES)
            if st["jacobian"]:
                over["z_factor"] = 1.0
            kp = TR.xy(fe["kept_prev"])[:200]
            status, pose, trace = world.align(st, a, b, world.seeds[k] if seeded else None, seeded, tables={0: world.patch_table(c, a, kp)},
                                              tables_key=("chain", kind, st["pattern"], k), **over)
            want = pair_want([(status, pose, trace)])
            tag = "call%d." % k
            out.update({tag + "info": np.array([int(fe["info"][f]) for f in INFO_FIELDS], np.int32).tobytes(), tag + "good": fe["good"].tobytes(),
                        tag + "kept_prev": fe["kept_prev"].tobytes(), tag + "kept_cur": fe["kept_cur"].tobytes()})
            if "pair0.pose" in want:
                out.update({tag + "pose": want["pair0.pose"], tag + "stats": want["pair0.stats"]})
            prev = fe["kept_cur"]
        return out

    return run, expected


action("tracking", ("sync", "async"), ("uwt_tracking_batch", "uwt_tracking_batch_async", "uwt_default_tracking_params"),
       ("jacobian", "content"))(lambda: chain("surf", False))
action("tracking_seeded", ("sync", "async"), ("uwt_tracking_batch_seeded", "uwt_tracking_batch_seeded_async"),
       ("jacobian", "content"))(lambda: chain("surf", True))
action("tracking_orb", ("sync", "async"), ("uwt_tracking_orb_batch", "uwt_tracking_orb_batch_async", "uwt_default_tracking_orb_params"),
       ("jacobian", "content", "pattern"))(lambda: chain("orb", False))
action("tracking_orb_seeded", ("sync", "async"), ("uwt_tracking_orb_batch_seeded", "uwt_tracking_orb_batch_seeded_async"),
       ("jacobian", "content", "pattern"))(lambda: chain("orb", True))


# ---- outputs and the map -----------------------------------------------------------------------------------------------------------------
def _quality(rec):
    return np.array([int(rec[k]) for k in WR.QUALITY_FIELDS], np.int64).tobytes()


@action("warp_image", ("sync", "async"), ("uwt_warp_image_batch", "uwt_warp_image_batch_async"), ("content",))
def _warp_image():
    """uwt_warp_image_batch* of pairs (0, 1) and (4, 5) on level 1 under two of the world's seeds"""
    pairs, lvl = [(0, 1), (4, 5)], 1

    def out_of(warped, valid, diff, quality):
        out = {}
        for i in range(len(pairs)):
            out.update({"warped%d" % i: warped[i].tobytes(), "valid%d" % i: valid[i].tobytes(), "absdiff%d" % i: diff[i].tobytes(),
                        "quality%d" % i: _quality(quality[i])})
        return out

    def run(rig, form, st):
        ctx, w = rig.ctx, rig.world
        ref, tgt = slots_of(pairs)
        if form == "sync":
            r = ctx.warp_image_batch(ref, tgt, w.seeds[:2], lvl=lvl)
            return out_of(r["warped"], r["valid"], r["absdiff"], r["quality"])
        L = ctx.level_info(lvl)
        assert L.pitch == L.img_w
        n, P = L.img_w * L.img_h, len(pairs)
        s = dict(warped=rig.pool.take(P * n), valid=rig.pool.take(P * n), absdiff=rig.pool.take(P * n),
                 quality=rig.pool.take(P * rig.capi.WARP_QUALITY.itemsize))
        ctx.warp_image_batch_async(ref, tgt, rig.device("seeds", lambda: w.seeds), {k: v.ptr for k, v in s.items()}, lvl=lvl)
        return Pending(rig, lambda: out_of(*[s[k].read()[:P * n].reshape(P, n) for k in ("warped", "valid", "absdiff")],
                                           s["quality"].read(rig.capi.WARP_QUALITY)[:P]))

    def expected(world, st):
        c = st["content"]
        refs = [WR.dense_reference(world.O, world.params(st), lvl, world.planes(c, a)[0][lvl], world.planes(c, b)[0][lvl],
                                   world.planes(c, a)[2][lvl], world.seeds[i]) for i, (a, b) in enumerate(pairs)]
        return out_of([r["warped"] for r in refs], [r["valid"] for r in refs], [r["absdiff"] for r in refs], [r["quality"] for r in refs])
    return run, expected


@action("warp_explicit", reaches=("uwt_obtain_image_transformed", "uwt_warp_mosaic"), reads=("content",))
def _warp_explicit():
    """uwt_obtain_image_transformed over the dense table of slot 2 on level 1 under a seed, and uwt_warp_mosaic of the result"""
    lvl = 1

    def table(world, c):
        return WR.dense_table(world.O, world.params(state("opencv")), lvl, world.planes(c, 2)[2][lvl], world.seeds[3])

    def run(rig, form, st):
        _, pts, wp = table(rig.world, st["content"])
        out, valid = rig.ctx.obtain_image_transformed(2, lvl, pts, wp)
        return dict(image=out.tobytes(), valid=valid.tobytes(), mosaic=rig.ctx.warp_mosaic(2, 3, lvl, out).tobytes())

    def expected(world, st):
        c = st["content"]
        _, pts, wp = table(world, c)
        img1, img2 = world.planes(c, 2)[0][lvl], world.planes(c, 3)[0][lvl]
        out = np.zeros(img1.shape, np.uint8)
        valid = WR.obtain_image_transformed(img1, pts, wp, out)
        return dict(image=out.tobytes(), valid=np.ascontiguousarray(valid, np.uint8).tobytes(), mosaic=WR.mosaic(img1, img2, out).tobytes())
    return run, expected


def cloud(name, **over):
    """uwt_point_cloud_batch* of slots 0, 3, 6 under an accumulated trajectory"""
    slots = [0, 3, 6]

    def out_of(points, info, call):
        return dict(points=np.ascontiguousarray(points).tobytes(), info=np.array([[int(r[k]) for k in CR.INFO_FIELDS] for r in info], np.int64).tobytes(),
                    call=np.array([int(call[k]) for k in CR.INFO_FIELDS], np.int64).tobytes())

    def traj(world):
        return world.O.accumulate_trajectory(world.traj_poses[:3])

    def run(rig, form, st):
        ctx, capi, w = rig.ctx, rig.capi, rig.world
        p = capi.default_cloud_params(**over)
        if form == "sync":
            r = ctx.point_cloud_batch(slots, traj(w), p)
            return out_of(r["points"], r["info"], r["call"])
        F = len(slots)
        cap = F * (-(-(W * H) // max(int(p.stride), 1)))
        dp, di = rig.pool.take(cap * 16), rig.pool.take((F + 1) * capi.CLOUD_INFO.itemsize)
        ctx.point_cloud_batch_async(slots, rig.device("cloud_traj", lambda: traj(w)), dp.ptr, cap, di.ptr, p)

        def fetch():
            info = di.read(capi.CLOUD_INFO)[:F + 1]
            return out_of(dp.read(capi.CLOUD_POINT)[:int(info[F]["written"])], info[:F], info[F])
        return Pending(rig, fetch)

    def expected(world, st):
        c = st["content"]
        q = dict(mode=0, stride=100, skip_invalid=0)
        q.update(over)
        t = traj(world)
        frames = [(world.dense_table(c, s, 0), t[f], world.gray[c][s]) for f, s in enumerate(slots)]
        pts, info, call = CR.batch_cloud(world.O, frames, world.level(0), st["arith"], q["mode"], q["stride"], q["skip_invalid"])
        F = CR.INFO_FIELDS
        return out_of(pts[:call[5]], [dict(zip(F, r)) for r in info], dict(zip(F, call)))

    return run, expected


for _name, _over in (("cloud_mode0", {}), ("cloud_mode1", dict(mode=1, stride=37)), ("cloud_skip", dict(stride=37, skip_invalid=1))):
    action(_name, ("sync", "async"), ("uwt_point_cloud_batch", "uwt_point_cloud_batch_async", "uwt_default_cloud_params"),
           ("content",))(lambda n=_name, o=_over: cloud(n, **o))


@action("cloud_points", reaches=("uwt_point_cloud_points",), reads=("content",))
def _cloud_points():
    """uwt_point_cloud_points on the candidate table of slot 4 in mode 1"""
    def run(rig, form, st):
        pts = rig.world.candidate_table(st["content"], 4, 0)
        out, n, status = rig.ctx.point_cloud_points(4, pts, rig.world.seeds[2], rig.capi.default_cloud_params(mode=1, stride=3))
        return dict(points=out.tobytes(), n=np.int64(n).tobytes(), status=np.int32(status).tobytes())

    def expected(world, st):
        c = st["content"]
        rec, n_sel = CR.frame_cloud(world.O, world.candidate_table(c, 4, 0), world.seeds[2], world.level(0), st["arith"], 1, 3, 0, world.gray[c][4], 0)
        return dict(points=rec.tobytes(), n=np.int64(len(rec)).tobytes(), status=np.int32(OK).tobytes())
    return run, expected


def sweep(source):
    """uwt_sweep_depth_batch* on level 1: reference slot 0 with view slot 1 and reference slot 4 with view slot 5, 16 hypotheses, into
    buffers of the caller (no depth plane of a slot is written)"""
    jobs, lvl, n_hyp = [(0, 1), (4, 5)], 1, 16
    over = dict(lvl=lvl, source=source, threshold=THRESHOLD)

    def inputs(world):
        p = world.params(state("opencv"))
        codes = DR.hypotheses(0.5, 3.0, p.depth_scale, n_hyp)
        assert codes is not None
        return codes, np.stack([world.seeds[0], world.seeds[2]]).reshape(2, 1, 7)

    def out_of(depth, cost, outcome, info):
        out = {}
        for j in range(len(jobs)):
            out.update({"depth%d" % j: np.ascontiguousarray(depth[j], np.uint16).tobytes(), "cost%d" % j: np.ascontiguousarray(cost[j], np.uint16).tobytes(),
                        "outcome%d" % j: np.ascontiguousarray(outcome[j], np.uint8).tobytes(),
                        "info%d" % j: np.array(DR.info_tuple(info[j]), np.int64).tobytes()})
        return out

    def run(rig, form, st):
        ctx, capi, w = rig.ctx, rig.capi, rig.world
        codes, poses = inputs(w)
        p = capi.default_sweep_params(n_views=1, n_hyp=n_hyp, **over)
        refs, views = [a for a, _ in jobs], [[b] for _, b in jobs]
        if form == "sync":
            r = ctx.sweep_depth(refs, views, poses, codes, p)
            return out_of(r["depth"], r["cost"], r["outcome"], r["info"])
        L = ctx.level_info(lvl)
        assert L.pitch == L.img_w
        n, J = L.img_w * L.img_h, len(jobs)
        s = dict(depth=rig.pool.take(J * n * 2), cost=rig.pool.take(J * n * 2), outcome=rig.pool.take(J * n), info=rig.pool.take(J * capi.SWEEP_INFO.itemsize))
        ctx.sweep_depth_async(refs, views, rig.device("sweep_poses", lambda: poses), codes, {k: v.ptr for k, v in s.items()}, p)
        return Pending(rig, lambda: out_of(s["depth"].read(np.uint16)[:J * n].reshape(J, n), s["cost"].read(np.uint16)[:J * n].reshape(J, n),
                                           s["outcome"].read()[:J * n].reshape(J, n), s["info"].read(capi.SWEEP_INFO)[:J]))

    def expected(world, st):
        c = st["content"]
        codes, poses = inputs(world)
        res = [DR.sweep(world.O, world.params(st), world.planes(c, a)[0][lvl], [world.planes(c, b)[0][lvl]], poses[j], codes, **over)
               for j, (a, b) in enumerate(jobs)]
        return out_of([r["depth"] for r in res], [r["cost"] for r in res], [r["outcome"] for r in res], [r["info"] for r in res])

    return run, expected


for _s in (0, 1):
    action("sweep_source%d" % _s, ("sync", "async"), ("uwt_sweep_depth_batch", "uwt_sweep_depth_batch_async", "uwt_default_sweep_params"),
           ("content",))(lambda s=_s: sweep(s))


@action("trajectory", ("sync", "async"), ("uwt_accumulate_trajectory", "uwt_accumulate_trajectory_scan", "uwt_accumulate_trajectory_device_async",
                                          "uwt_accumulate_trajectory_device_from_async", "uwt_predict_seeds", "uwt_predict_seeds_device_async"),
        outputs=dict(sync=("traj", "scan", "seeds"), **{"async": ("first", "second", "seeds")}))
def _trajectory():
    """accumulate_trajectory (sequential, and the scan on two poses, where no regrouping is possible), its device forms — the second
    behind the first one's last row — and predict_seeds"""
    def run(rig, form, st):
        ctx, w = rig.ctx, rig.world
        tp = w.traj_poses
        if form == "sync":
            return dict(traj=ctx.accumulate_trajectory(tp, start=w.seeds[0], t_scale=40.0, reference_axes=True).tobytes(),
                        scan=ctx.accumulate_trajectory(tp[:2], start=w.seeds[0], scan=True).tobytes(),
                        seeds=ctx.predict_seeds(tp[:4], tp[1:5]).tobytes())
        d_poses = rig.device("traj_poses", lambda: tp)
        a, b, s = rig.pool.take(3 * 28), rig.pool.take(3 * 28), rig.pool.take(4 * 28)
        ctx.accumulate_trajectory_device_async(d_poses, 3, a.ptr, start=w.seeds[0])
        ctx.accumulate_trajectory_device_from_async(d_poses + 3 * 28, 3, a.ptr + 2 * 28, b.ptr)
        ctx.predict_seeds_device_async(4, d_poses, d_poses + 28, s.ptr)
        return Pending(rig, lambda: dict(first=a.read(np.float32)[:21].tobytes(), second=b.read(np.float32)[:21].tobytes(),
                                         seeds=s.read(np.float32)[:28].tobytes()))

    def expected(world, st):
        O, tp = world.O, world.traj_poses
        whole = O.accumulate_trajectory(tp, start=world.seeds[0])
        return dict(traj=O.accumulate_trajectory(tp, start=world.seeds[0], t_scale=40.0, reference_axes=True).tobytes(),
                    scan=O.accumulate_trajectory(tp[:2], start=world.seeds[0]).tobytes(), seeds=SR.predict_seeds(O, tp[:4], tp[1:5]).tobytes(),
                    first=whole[:3].tobytes(), second=whole[3:].tobytes())
    return run, expected


@action("planes", ("sync", "deferred"), reaches=("uwt_get_plane", "uwt_build_pyramids", "uwt_apply_gradient", "uwt_set_frame",
                                                  "uwt_plane_device_ptr", "uwt_stream", "uwt_set_deferred"), reads=("content",))
def _planes():
    """uwt_set_frame of slot 7 with its own content, the stage calls on it, and the planes read back on level 2; "deferred": the stage
    calls under uwt_set_deferred(1) — they return once enqueued, the read-backs deliver"""
    def run(rig, form, st):
        ctx, capi, c = rig.ctx, rig.capi, st["content"]
        if form == "deferred":
            ctx.set_deferred(True)
        try:
            ctx.set_frame(7, rig.world.gray[c][7], rig.world.depth[c][7])
            ctx.build_pyramids(7, 1)
            ctx.apply_gradient(7, 1)
            assert ctx.plane_device_ptr(7, 2, capi.PLANE_IMAGE) and ctx.stream()
            return {name: ctx.get_plane(7, 2, plane).tobytes() for name, plane in (("image", capi.PLANE_IMAGE), ("depth", capi.PLANE_DEPTH),
                                                                                   ("gx", capi.PLANE_GRADX), ("gy", capi.PLANE_GRADY))}
        finally:
            if form == "deferred":
                ctx.set_deferred(False)

    def expected(world, st):
        imgs, grads, deps = world.planes(st["content"], 7)
        return dict(image=imgs[2].tobytes(), depth=deps[2].tobytes(), gx=grads[2][0].tobytes(), gy=grads[2][1].tobytes())
    return run, expected


BY_NAME = {a.name: a for a in ACTIONS}
assert len(BY_NAME) == len(ACTIONS)


# ---- excursions --------------------------------------------------------------------------------------------------------------------------
class Excursion:
    """A predecessor that changes something, works under it and puts it back: enter(rig), the work (actions in their synchronous form
    under the state `altered` makes of the baseline, each compared with its expectation there), leave(rig).  `altered`: the keys of the
    documented state — or of the call's own arguments — that differ while the work runs.  tests/test_history_cpu.py requires that some
    action's expectation under the altered state differs from its baseline one: otherwise the excursion could leave nothing behind that a
    successor would show."""

    def __init__(self, name, altered, work, enter=None, leave=None, reaches=(), forms=None):
        self.name, self.altered, self.work, self.enter, self.leave, self.reaches = name, altered, tuple(work), enter, leave, tuple(reaches)
        self.forms = forms or {}

    def state(self, arith):
        return state(arith, **self.altered)


TUNING_DEFAULT_FIELDS = ("split", "split_min", "split_min_px", "stream_bytes", "tail_update", "target_blocks", "coarse", "coarse_batch_px",
                         "coarse_weighted", "overlap_gradients", "first_poll", "chained", "speculation", "fused_stages", "pyramid_batch",
                         "typed_loads")


def _tuning(**over):
    def enter(rig):
        rig.saved_tuning = {k: getattr(rig.ctx.get_tuning(), k) for k in TUNING_DEFAULT_FIELDS}
        rig.ctx.set_tuning(**over)

    def leave(rig):
        rig.ctx.set_tuning(**rig.saved_tuning)
    return enter, leave


def _params(**over):
    def enter(rig):
        rig.ctx.update_params(**over)

    def leave(rig):
        rig.ctx.update_params(**rig.base_params)
    return enter, leave


def _content(how):
    def enter(rig):
        rig.load("Y", how)

    def leave(rig):
        rig.load("X", how)
    return enter, leave


def _grow(rig):
    """one call of every family with a growable block at a larger size than the catalogue's actions use: each DevBuf grows"""
    ctx, w = rig.ctx, rig.world
    big = 4096
    ctx.surf_detect_describe_batch([0], cap=big)
    ctx.orb_detect_describe_batch([0], cap=big)
    pairs = _descriptor_pairs(w, "l2")[:1]
    ctx.match_descriptors_batch(pairs, cap=big)
    ctx.ransac_inliers_batch(w.ransac_inputs()[:1], cap=big, kp_cap=big)
    ctx.tracking_batch([0], [1], cap=big)
    ctx.obtain_candidate_points_batch(0, 8, 0, THRESHOLD)
    ctx.robust_weights(np.tile(w.residuals, 40))
    # the image warp, the map and the sweep are sized by level, batch and stride: level 0 with every pair / slot, stride 1 (the actions use
    # level 1, two or three of them, strides of 37 and 100); and the candidate tables of four pairs under a threshold that keeps more rows
    ref, tgt = slots_of(PAIR_LISTS["fwd"])
    ctx.warp_image_batch(ref, tgt, w.seeds, lvl=0)
    ctx.point_cloud_batch(list(range(MAX_FRAMES)), w.O.accumulate_trajectory(np.tile(w.traj_poses, (2, 1))[:MAX_FRAMES]),
                          rig.capi.default_cloud_params(stride=1))
    codes = DR.hypotheses(0.5, 3.0, ctx.params.depth_scale, 16)
    ctx.sweep_depth(ref, tgt.reshape(-1, 1), w.seeds.reshape(4, 1, 7), codes, rig.capi.default_sweep_params(n_views=1, n_hyp=16, lvl=0, source=0))
    ctx.estimate_pose_candidates_batch(ref, tgt, threshold=1.0)


EXCURSIONS = []
_DENSE_WORK = ("dense_3", "dense_seeded_h1")
_SWAP = dict(pairs="swap")   # the work under a launch-shape excursion runs the exchanged list: what it leaves in the work areas is not X's
for _name, _altered, _work, _pair, _reach in [
    ("metric", dict(jacobian=1), _DENSE_WORK + ("features_plain", "residual_jacobian"), None, ("uwt_set_jacobian", "uwt_get_jacobian")),
    ("other_arith", dict(), _DENSE_WORK, None, ("uwt_update_params",)),
    ("tukey", dict(weights=1), _DENSE_WORK, _params(weights=1), ("uwt_update_params",)),
    ("huber", dict(weights=2), _DENSE_WORK, _params(weights=2), ("uwt_update_params",)),
    ("bilinear", dict(sampler=1), _DENSE_WORK, _params(sampler=1), ("uwt_update_params",)),
    ("fixed_schedule", dict(schedule="fixed"), _DENSE_WORK + ("dense_4",), _params(**SCHEDULES["fixed"]), ("uwt_update_params",)),
    ("tuning_split", _SWAP, ("dense_4",), _tuning(split_min_px=1, split_min=2), ("uwt_set_tuning", "uwt_get_tuning")),
    ("tuning_coarse_batch_px0", _SWAP, ("dense_4",), _tuning(coarse_batch_px=0), ("uwt_set_tuning",)),
    ("tuning_chained1", _SWAP, ("dense_4",), _tuning(chained=1), ("uwt_set_tuning",)),
    ("tuning_chained0", _SWAP, ("dense_4",), _tuning(chained=0), ("uwt_set_tuning",)),
    ("tuning_tail_update2", _SWAP, ("dense_4",), _tuning(tail_update=2, chained=0), ("uwt_set_tuning",)),
    ("tuning_speculation0", _SWAP, ("dense_4",), _tuning(speculation=0), ("uwt_set_tuning",)),
    ("tuning_fused_stages0", _SWAP, ("dense_4", "planes"), _tuning(fused_stages=0), ("uwt_set_tuning",)),
    ("tuning_overlap_gradients3", _SWAP, ("dense_4",), _tuning(overlap_gradients=3), ("uwt_set_tuning",)),
    ("orb_pattern", dict(pattern="other"), ("orb_detect", "orb_stages"), None, ("uwt_orb_set_pattern",)),
    ("ransac_loose", dict(ransac="loose"), ("ransac",), None, ()),
    ("content_y_upload", dict(content="Y"), ("dense_3", "candidates_plain", "surf_detect"), _content("sync"), ("uwt_upload_frames",)),
    ("content_y_upload_async", dict(content="Y"), ("dense_3", "candidates_plain", "orb_detect"), _content("async"),
     ("uwt_upload_frames_async", "uwt_host_alloc", "uwt_host_free")),
    ("pairs_other", dict(pairs="other"), ("dense_4",), None, ()),
    ("pairs_shorter", dict(pairs="other"), ("dense_1",), None, ()),
    ("pairs_longer", dict(pairs="swap"), ("dense_4",), None, ()),
    ("pairs_exchanged", dict(pairs="swap"), ("dense_3",), None, ()),
]:
    EXCURSIONS.append(Excursion(_name, _altered, _work, *(_pair or (None, None)), reaches=_reach))


def _special(name):
    return next(e for e in EXCURSIONS if e.name == name)


def _metric_enter(rig):
    rig.ctx.set_jacobian("metric")
    assert rig.ctx.get_jacobian() == rig.capi.JACOBIAN_METRIC


_special("metric").enter, _special("metric").leave = _metric_enter, lambda rig: rig.ctx.set_jacobian("reference")
_special("orb_pattern").enter = lambda rig: rig.ctx.orb_set_pattern(OK_.second_pattern())
_special("orb_pattern").leave = lambda rig: rig.ctx.orb_set_pattern(None)


def _other_arith_state(arith):
    return state("legacy" if arith == "opencv" else "opencv")


_special("other_arith").state = _other_arith_state
_special("other_arith").enter = lambda rig: rig.ctx.update_params(arith=1 - rig.base_params["arith"])
_special("other_arith").leave = lambda rig: rig.ctx.update_params(**rig.base_params)


def _deferred_work(rig):
    """two stage calls that return once enqueued, then a dense call on what they prepared"""
    rig.ctx.build_pyramids(0, MAX_FRAMES)
    rig.ctx.apply_gradient(0, MAX_FRAMES)


def _guards_leave(rig):
    assert rig.ctx.debug_check_guards() == (0, "")
    rig.ctx.debug_guards(0)


EXCURSIONS += [
    Excursion("deferred", _SWAP, ("dense_3",), lambda rig: (rig.ctx.set_deferred(True), _deferred_work(rig)), lambda rig: rig.ctx.set_deferred(False),
              reaches=("uwt_set_deferred",)),
    Excursion("debug_guards", _SWAP, ("dense_4", "features_plain", "orb_detect", "ransac"), lambda rig: rig.ctx.debug_guards(4096), _guards_leave,
              reaches=("uwt_debug_guards", "uwt_debug_check_guards")),
    Excursion("grow_every_family", _SWAP, ("dense_3",), _grow, None),
]
EXCURSION_BY_NAME = {e.name: e for e in EXCURSIONS}
assert len(EXCURSION_BY_NAME) == len(EXCURSIONS)


def run_excursion(rig, exc, arith):
    """enter, the work compared under the altered state, leave.  Returns the first difference as (action, key, offset) or None."""
    st = exc.state(arith)
    bad = None
    if exc.enter:
        exc.enter(rig)
    try:
        for name in exc.work:
            a = BY_NAME[name]
            d = first_difference(collect(a.run(rig, "sync", st)), a.expected(rig.world, st, "sync"))
            if d and not bad:
                bad = (name,) + d
    finally:
        if exc.leave:
            exc.leave(rig)
    return bad


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
class Refusal:
    """A predecessor that fails as the header documents: run(rig, arith) makes the call, asserts the status (and, where one pair fails,
    the other pairs' results) and returns None, or a description of what was not as documented."""

    def __init__(self, name, run, reaches=()):
        self.name, self.run, self.reaches = name, run, tuple(reaches)


def _refused(rig, status, fn):
    try:
        fn()
    except rig.capi.UwtError as e:
        return None if e.status == status else "status %d, not %d" % (e.status, status)
    return "the call was not refused"


def _slot_out_of_range(rig, arith):
    dp, ds = rig.pool.take(3 * 28), rig.pool.take(3 * 16)
    return (_refused(rig, INVALID_ARG, lambda: rig.ctx.estimate_pose_batch([0, 2, MAX_FRAMES], [1, 3, 5])) or
            _refused(rig, INVALID_ARG, lambda: rig.ctx.track_batch_async(0, MAX_FRAMES, [0, 2, 4], [1, 3, MAX_FRAMES], dp.ptr, ds.ptr)) or
            _refused(rig, INVALID_ARG, lambda: rig.ctx.surf_detect_describe_batch([MAX_FRAMES])))


def _seeds_overlap_outputs(rig, arith):
    dp, ds = rig.pool.take(3 * 28), rig.pool.take(3 * 16)
    return _refused(rig, INVALID_ARG, lambda: rig.ctx.track_batch_seeded_async(0, MAX_FRAMES, [0, 2, 4], [1, 3, 5], dp.ptr, ds.ptr, d_seeds_ptr=dp.ptr,
                                                                               handoff=1))


def _too_many_pairs(rig, arith):
    return _refused(rig, CAPACITY, lambda: rig.ctx.estimate_pose_batch([0, 2, 4, 6, 0], [1, 3, 5, 7, 1]))


def _cap_above_max_rows(rig, arith):
    return _refused(rig, CAPACITY, lambda: rig.ctx.surf_detect_describe_batch([0], cap=rig.capi.UWT_MATCH_MAX_ROWS + 1))


def _under(fn, **over):
    """a refusal under other weights: the parameters set, the refusal, the baseline's back (a failed pair must leave the robust scale's
    histograms as clean as a pair that ran)"""
    def run(rig, arith):
        rig.ctx.update_params(**over)
        try:
            return fn(rig, arith, **over)
        finally:
            rig.ctx.update_params(**rig.base_params)
    return run


def _nan_seed(rig, arith, **over):
    """a NaN seed on pair 1 of three: UWT_ERR_PAIR_FAILED, that pair refused, the others as seeded from their own seeds"""
    w, st = rig.world, state(arith, **over)
    try:
        poses, stats = rig.ctx.estimate_pose_batch_seeded([0, 2, 4], [1, 3, 5], w.bad_seeds, 1, raise_on_pair_failure=True)
        return "the call did not fail"
    except rig.capi.UwtError as e:
        if e.status != PAIR_FAILED:
            return "status %d" % e.status
    poses, stats = rig.ctx.estimate_pose_batch_seeded([0, 2, 4], [1, 3, 5], w.bad_seeds, 1)
    want = pair_want([w.align(st, a, b, w.bad_seeds[i], True) for i, (a, b) in enumerate(PAIR_LISTS["fwd"][:3])])
    d = first_difference(pair_out(poses, stats_array(stats)), want)
    return None if d is None else "%s at %d" % d


def _zero_depth_pair(rig, arith, **over):
    """pair 1's reference frame under an all-zero depth plane (the depth an alignment reads is its reference's): no point of the pair is
    valid, UWT_ERR_PAIR_FAILED, the other pairs as ever; the slot's depth is put back"""
    w, st, ctx = rig.world, state(arith, **over), rig.ctx
    ctx.upload_frames(2, w.gray["X"][2:3], np.zeros((1, H, W), np.uint16))
    ctx.build_pyramids(2, 1)
    ctx.apply_gradient(2, 1)
    try:
        poses, stats = ctx.estimate_pose_batch([0, 2, 4], [1, 3, 5])
    finally:
        ctx.upload_frames(2, w.gray["X"][2:3], w.depth["X"][2:3])
        ctx.build_pyramids(2, 1)
        ctx.apply_gradient(2, 1)
    if stats[1]["status"] != NO_VALID_POINTS:
        return "pair 1: status %d" % stats[1]["status"]
    want = pair_want([w.align(st, a, b) for a, b in PAIR_LISTS["fwd"][:3]])
    want = {k: v for k, v in want.items() if not k.startswith("pair1.")}
    d = first_difference(pair_out(poses, stats_array(stats)), want)
    return None if d is None else "%s at %d" % d


def _few_matches(rig, arith):
    """a chain pair with fewer than 8 matches (a frame against itself turned upside down under a RANSAC distance no pair meets is not
    needed: a flat target has no key point): UWT_ERR_PAIR_FAILED for that pair, the other pair's front end as ever"""
    w, ctx, capi = rig.world, rig.ctx, rig.capi
    ctx.upload_frames(3, np.full((1, H, W), 128, np.uint8), w.depth["X"][3:4])
    try:
        r = ctx.tracking_batch([0, 2], [1, 3], cap=CAP)
    finally:
        ctx.upload_frames(3, w.gray["X"][3:4], w.depth["X"][3:4])
        ctx.build_pyramids(3, 1)
        ctx.apply_gradient(3, 1)
    if r["status"] != PAIR_FAILED:
        return "status %d" % r["status"]
    if int(r["info"][1]["n_matches"]) >= 8 or int(r["stats"][1]["status"]) == OK:
        return "pair 1: %d matches, status %d" % (int(r["info"][1]["n_matches"]), int(r["stats"][1]["status"]))
    want = BY_NAME["tracking"].expected(w, state(arith))
    want = {k[len("call0."):]: v for k, v in want.items() if k.startswith("call0.")}
    # (the catalogue's chain runs under min_matches 90, this call under the default 110: neither is read by a pair without previous key points)
    d = first_difference(_chain_out(r, 0, ""), want)
    return None if d is None else "%s at %d" % d


REFUSALS = [
    Refusal("slot_out_of_range", _slot_out_of_range),
    Refusal("seeds_overlap_outputs", _seeds_overlap_outputs),
    Refusal("too_many_pairs", _too_many_pairs),
    Refusal("cap_above_max_rows", _cap_above_max_rows),
    Refusal("nan_seed_on_one_pair", _nan_seed),
    Refusal("zero_depth_pair", _zero_depth_pair),
    Refusal("chain_pair_with_few_matches", _few_matches),
    Refusal("nan_seed_under_huber", _under(_nan_seed, weights=2)),
    Refusal("zero_depth_pair_under_tukey", _under(_zero_depth_pair, weights=1)),
]
REFUSAL_BY_NAME = {r.name: r for r in REFUSALS}


# ---- predecessors ------------------------------------------------------------------------------------------------------------------------
def predecessors():
    """every (kind, name, form) a successor is run behind, in catalogue order: every action in every form, every excursion, every refusal"""
    out = [("action", a.name, f) for a in ACTIONS for f in a.forms]
    out += [("excursion", e.name, None) for e in EXCURSIONS]
    out += [("refusal", r.name, None) for r in REFUSALS]
    return out


# ---- the random walk ---------------------------------------------------------------------------------------------------------------------
ALL_PAIRS = sorted(set(p for l in PAIR_LISTS.values() for p in l))


def dense_subset(pairs):
    """a dense call on an explicit pair list (the walk draws 1 to 4 of the twelve pairs of PAIR_LISTS): (run, expected) as dense()"""
    pairs = [tuple(int(v) for v in p) for p in pairs]
    n = len(pairs)

    def run(rig, form, st):
        ctx, (ref, tgt) = rig.ctx, slots_of(pairs)
        if form == "sync":
            return pair_out(*_sync(ctx.estimate_pose_batch(ref, tgt)))
        if form == "host":
            hp, hs = (a[:n] for a in rig.h_results[rig.h_next % len(rig.h_results)])
            rig.h_next += 1
            ticket = ctx.track_batch_host_async(0, MAX_FRAMES, ref, tgt, hp, hs)
            return Pending(rig, lambda: pair_out(np.array(hp), np.array(hs).view(STATS).reshape(-1)), wait=lambda: ctx.wait_ticket(ticket))
        dp, ds = rig.pool.take(n * 28), rig.pool.take(n * 16)
        ctx.track_batch_async(0, MAX_FRAMES, ref, tgt, dp.ptr, ds.ptr)
        return Pending(rig, lambda: pair_out(dp.read(np.float32)[:n * 7], ds.read(STATS)[:n]))

    def expected(world, st):
        return world.in_arith(st, lambda: pair_want([world.align(st, a, b) for a, b in pairs]))

    return run, expected


def random_walk(rig, arith, steps, seed, log=None):
    """`steps` random steps on one context: an action in a random form, a dense call on a random batch of 1 to 4 pairs, an excursion or a
    refusal; the results of an asynchronous step are collected one to three steps later.  Returns the list of failures."""
    rng = np.random.default_rng(seed)
    st, world = state(arith), rig.world
    failures, due = [], []

    def settle(now):
        for item in [d for d in due if d[0] <= now]:
            due.remove(item)
            _, what, pending, want = item
            d = first_difference(collect(pending), want)
            if d:
                failures.append("%s: output %s differs at byte %d" % ((what,) + d))

    for step in range(steps):
        settle(step)
        u = rng.random()
        if u < 0.55:
            a = ACTIONS[int(rng.integers(len(ACTIONS)))]
            form = a.forms[int(rng.integers(len(a.forms)))]
            what, res, want = "step %d: %s (%s)" % (step, a.name, form), a.run(rig, form, st), a.expected(world, st, form)
        elif u < 0.75:
            pairs = [ALL_PAIRS[i] for i in rng.permutation(len(ALL_PAIRS))[:int(rng.integers(1, MAX_PAIRS + 1))]]
            form = ("sync", "async", "host")[int(rng.integers(3))]
            run, expected = dense_subset(pairs)
            what, res, want = "step %d: dense %r (%s)" % (step, pairs, form), run(rig, form, st), expected(world, st)
        elif u < 0.9:
            e = EXCURSIONS[int(rng.integers(len(EXCURSIONS)))]
            bad = run_excursion(rig, e, arith)
            what, res, want = "step %d: excursion %s" % (step, e.name), None, None
            if bad:
                failures.append("%s: work %s, output %s differs at byte %d" % ((what,) + bad))
        else:
            r = REFUSALS[int(rng.integers(len(REFUSALS)))]
            bad = r.run(rig, arith)
            what, res, want = "step %d: refusal %s" % (step, r.name), None, None
            if bad:
                failures.append("%s: %s" % (what, bad))
        if log:
            log(what)
        if isinstance(res, Pending):
            due.append((step + int(rng.integers(1, 4)), what, res, want))
        elif res is not None:
            d = first_difference(res, want)
            if d:
                failures.append("%s: output %s differs at byte %d" % ((what,) + d))
    settle(steps + 4)
    return failures


SIZES = dict(actions=len(ACTIONS), action_forms=sum(len(a.forms) for a in ACTIONS), excursions=len(EXCURSIONS), refusals=len(REFUSALS))

# exports no action, excursion or refusal reaches, each with its reason (lifecycle, profiling, pure host functions that take no context,
# ingest: the only reasons tests/test_history_cpu.py accepts)
NOT_IN_MATRIX = {
    "uwt_abi_version": "pure host function", "uwt_source_id": "pure host function", "uwt_status_string": "pure host function",
    "uwt_default_params": "pure host function", "uwt_ransac_iterations": "pure host function", "uwt_keypoint_angle_deg": "pure host function",
    "uwt_default_surf_params": "pure host function", "uwt_default_orb_params": "pure host function", "uwt_orb_level_quota": "pure host function",
    "uwt_orb_default_pattern": "pure host function", "uwt_sweep_hypotheses": "pure host function",
    "uwt_create": "lifecycle", "uwt_destroy": "lifecycle", "uwt_last_error": "lifecycle", "uwt_sync": "lifecycle",
    "uwt_profile_enable": "profiling", "uwt_profile_read": "profiling", "uwt_profile_read_levels": "profiling", "uwt_profile_clock": "profiling",
    "uwt_ingest_create": "ingest", "uwt_ingest_destroy": "ingest", "uwt_ingest_maps": "ingest", "uwt_ingest_undistort": "ingest",
    "uwt_ingest_calculate_roi": "ingest", "uwt_ingest_frame": "ingest",
}
# reached by the tests' own machinery rather than by a catalogue entry
REACHED_BY_THE_HARNESS = {"uwt_debug_window_open": "test_every_entry_closes_the_window reads it after every entry"}


def reached():
    names = set(REACHED_BY_THE_HARNESS)
    for x in ACTIONS + EXCURSIONS + REFUSALS:
        names.update(x.reaches)
    return names


def make_world():
    from oracle import oracle
    oracle.build()
    return World(oracle, importlib.import_module("uw-slam_amd.synth"))
