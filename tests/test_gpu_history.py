"""Call-history independence (INTEGRATION.md "what a result depends on"): a call's result depends on its arguments and on the context
state the header names, never on what ran before it on the same context.  Every comparison is bit for bit against the CPU restatements
(tests/history_cases.py: no expectation comes from a GPU run).

test_successor_after_every_predecessor[S]   one long-lived context per test; for every predecessor P of the catalogue, in order — every
                                            action in every form, every excursion, every refusal, S itself included, and for every form of S — run P, run S with
                                            no wait in between, compare S (and P, when it is an action) with its expectation
test_random_walk[seed]                      200 random steps on one context, asynchronous results collected up to three steps later
test_every_entry_closes_the_window[A]       a fixed-schedule uwt_track_batch_async leaves its early-preparation window open (asserted
                                            through uwt_debug_window_open); after A it is closed
"""
import importlib

import pytest

import history_cases as HC

pytestmark = pytest.mark.gpu

# the catalogue this file was written against (tests/test_history_cpu.py holds the same literals): a changed catalogue changes them here
assert HC.SIZES == dict(actions=43, action_forms=77, excursions=25, refusals=9), HC.SIZES
N_PREDECESSORS = 111
assert len(HC.predecessors()) == N_PREDECESSORS


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def world():
    return HC.make_world()


@pytest.fixture
def rig(capi, world, arith):
    r = HC.Rig(capi, world)
    yield r
    r.close()


def run_predecessor(rig, arith, kind, name, form):
    """Enqueues / runs predecessor P.  Returns (pending or results or None, expectation or None, failure or None)."""
    if kind == "action":
        a = HC.BY_NAME[name]
        return a.run(rig, form, HC.state(arith)), a.expected(rig.world, HC.state(arith), form), None
    if kind == "excursion":
        bad = HC.run_excursion(rig, HC.EXCURSION_BY_NAME[name], arith)
        return None, None, None if bad is None else "work under the excursion: %s, output %s differs at byte %d" % bad
    bad = HC.REFUSAL_BY_NAME[name].run(rig, arith)
    return None, None, bad


@pytest.mark.parametrize("successor", [a.name for a in HC.ACTIONS])
def test_successor_after_every_predecessor(rig, arith, successor):
    S = HC.BY_NAME[successor]
    st = HC.state(arith)
    failures, ran = [], 0
    for s_form in S.forms:                       # every predecessor in front of every form of the successor
        ran_form = 0
        for kind, name, form in HC.predecessors():
            p, want_p, bad = run_predecessor(rig, arith, kind, name, form)
            s = S.run(rig, s_form, st)           # no wait between P and S
            got_s = HC.collect(s)
            d = HC.first_difference(got_s, S.expected(rig.world, st, s_form))
            if d:
                failures.append("S = %s (%s) behind P = %s %s (%s): output %s differs at byte %d" % ((successor, s_form, kind, name, form) + d))
            if p is not None:                    # P's results are read after S's
                d = HC.first_difference(HC.collect(p), want_p)
                if d:
                    failures.append("P = %s (%s) in front of S = %s: output %s differs at byte %d" % ((name, form, successor) + d))
            if bad:
                failures.append("P = %s %s in front of S = %s: %s" % (kind, name, successor, bad))
            ran_form += 1
        assert ran_form == N_PREDECESSORS * 1
        ran += ran_form
    assert not failures, "%d of %d pairs:\n%s" % (len(failures), ran, "\n".join(failures[:20]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walk(rig, arith, seed):
    failures = HC.random_walk(rig, arith, 200, seed)
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:20]))


def test_declared_symbols_are_the_ones_called(rig, arith, capi, monkeypatch):
    """what tests/test_history_cpu.py counts as reached is what the catalogue calls: every symbol an entry declares is called by it"""
    called = set()

    class Recording:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("uwt_"):
                called.add(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(capi, "_lib", Recording(capi.lib()))
    for a in HC.ACTIONS:
        called.clear()
        for form in a.forms:
            HC.collect(a.run(rig, form, HC.state(arith)))
        assert set(a.reaches) <= called, (a.name, sorted(set(a.reaches) - called))
    for e in HC.EXCURSIONS:
        called.clear()
        assert HC.run_excursion(rig, e, arith) is None
        assert set(e.reaches) - {"uwt_host_alloc", "uwt_host_free"} <= called, (e.name, sorted(set(e.reaches) - called))   # (pinned once, by the rig)


# ---- the early-preparation window -------------------------------------------------------------------------------------------------------
# entries after which the window may stay open, with the reason (include/uwt.h at uwt_track_batch_async)
WINDOW_EXEMPT = {
    ("action", "dense_1", "async"): "uwt_track_batch_async re-opens the window",
    ("action", "dense_3", "async"): "uwt_track_batch_async re-opens the window",
    ("action", "dense_4", "async"): "uwt_track_batch_async re-opens the window",
    ("action", "dense_3", "host"): "uwt_track_batch_host_async is uwt_track_batch_async and two copies of its results: it re-opens the window",
    ("action", "dense_seeded_h0", "async"): "uwt_track_batch_seeded_async re-opens the window",
    ("action", "dense_seeded_h1", "async"): "uwt_track_batch_seeded_async re-opens the window",
    # (dense_tukey / dense_huber / dense_bilinear put the parameters back behind their call: uwt_update_params closes the window)
    # refused on its arguments before anything is enqueued, read back or changed: the context is as the batch call left it
    # (include/uwt.h at uwt_debug_window_open: "a call refused on its arguments alone ... may leave it as it was")
    ("refusal", "too_many_pairs", None): "UWT_ERR_CAPACITY before the lists are looked at",
    ("refusal", "cap_above_max_rows", None): "UWT_ERR_CAPACITY before a work area is reserved",
}


@pytest.fixture(scope="module")
def window_rig(capi, world):
    # (overlap_gradients 3 forces the side stream at any batch size; chained 0: four pairs run as a batch, the flow that records the window)
    r = HC.Rig(capi, world, tuning=dict(overlap_gradients=3, chained=0))
    yield r
    r.close()


@pytest.mark.one_arith
@pytest.mark.parametrize("kind,name,form", HC.predecessors(), ids=lambda v: str(v))
def test_every_entry_closes_the_window(window_rig, arith, kind, name, form):
    rig, ctx = window_rig, window_rig.ctx
    rig.set_schedule("fixed")
    ref, tgt = HC.slots_of(HC.PAIR_LISTS["fwd"])
    dp, ds = rig.pool.take(4 * 28), rig.pool.take(4 * 16)
    ctx.track_batch_async(0, HC.MAX_FRAMES, ref, tgt, dp.ptr, ds.ptr)
    assert ctx.debug_window_open(), "the call left no window: the test would pass vacuously"
    p, _, _ = run_predecessor(rig, arith, kind, name, form)   # (results are compared by the tests above, not here)
    still_open = ctx.debug_window_open()
    HC.collect(p) if p is not None else ctx.sync()
    rig.set_schedule("early")
    if (kind, name, form) not in WINDOW_EXEMPT:   # (an exempt entry may leave either state: a batch of one or two pairs records no window)
        assert not still_open, "%s %s (%s) left the window open" % (kind, name, form)
