"""The scalar tail of a Gauss-Newton iteration on records the test chose (uwt_gn_update_records): both fold forms — the block form
k_gn_update / update_compute and the ticket-gated wave form tail_fold_wave — and behind them update_solve_wave with the wave forms of the
solve and the exponential, bit for bit against the plain restatement tests/gn_update_ref.py, under both arithmetic sets.  The inputs are
those tests/test_gn_update_cpu.py shows to be discriminating (tests/gn_update_cases.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gn_update_cases as GC
import gn_update_ref as R

pytestmark = pytest.mark.gpu

SMALL = (64.0, 64.0, 31.5, 23.5)
ARGS = dict(k=0, max_iters=50, early_exit=0, epsilon=1e-3, gain=50.0, general=0)
FORMS = [(0, 0), (1, 0), (1, 3)]   # (form, records of stride past the count)


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()  # raises if libuwt_hip.so is missing: no fallback
    assert m.PAIR_STATE_DTYPE == R.STATE_DTYPE
    return m


@pytest.fixture
def ctx(capi, arith):
    c = capi.Context(capi.default_params(64, 48, *SMALL, max_frames=2, max_pairs=1, n_levels=3, first_level=2, last_level=0))
    yield c
    c.close()


def run(ctx, form, pad, pair_records, states, count, pair_base=0, lead_states=None, **kw):
    """One call over pairs whose records are pair_records[i] (count x 64 each): stride = count + pad, records past the count NaN patterns,
    rows below pair_base NaN records and lead_states.  Returns (states of the pairs, active); the rows below pair_base and the ticket
    words are checked here."""
    args = {**ARGS, **kw}
    stride = count + pad
    lead = np.zeros(pair_base, R.STATE_DTYPE) if lead_states is None else lead_states
    recs = np.full((pair_base + len(pair_records), stride, R.REC_WORDS), GC.NAN_WORD, np.uint32)
    for i, r in enumerate(pair_records):
        assert r.shape == (count, R.REC_WORDS)
        recs[pair_base + i, :count] = r
    st_in = np.concatenate([lead, np.asarray(states, R.STATE_DTYPE).reshape(-1)])
    out, active, tickets = ctx.gn_update_records(form, recs, st_in, count, pair_base=pair_base, **args)
    assert not tickets.any()                                            # zero before the call, zero again after it
    assert out[:pair_base].tobytes() == lead.tobytes()                  # rows below pair_base travel untouched
    return out[pair_base:], active


def expect(O, arith, form, pair_records, states, count, **kw):
    args = {**ARGS, **kw}
    res = [R.update(O, np.asarray(states, R.STATE_DTYPE).reshape(-1)[i], r, count, arith=arith, block_form=form == 0, **args)
           for i, r in enumerate(pair_records)]
    return np.array([r[0] for r in res], R.STATE_DTYPE), sum(1 for r in res if r[1])


def same_bits(got, exp, what):
    got, exp = np.asarray(got, R.STATE_DTYPE).reshape(-1), np.asarray(exp, R.STATE_DTYPE).reshape(-1)
    for i in range(len(exp)):
        assert got[i].tobytes() == exp[i].tobytes(), (what, i, got[i], exp[i])


def check_all_forms(ctx, O, arith, pair_records, states, count, what, forms=FORMS, **kw):
    exp, active = expect(O, arith, 1, pair_records, states, count, **kw)
    for form, pad in forms:
        got, act = run(ctx, form, pad, pair_records, states, count, **kw)
        same_bits(got, exp, (what, form, pad))
        assert act == active, (what, form, pad)
    return exp, active


# ---------------------------------------------------------------- fold

@pytest.mark.parametrize("count", GC.FOLD_COUNTS)
def test_fold_both_forms_bit_for_bit(ctx, O, arith, count):
    recs = GC.fold_records(count)
    for general in (0, 1):
        exp, active = check_all_forms(ctx, O, arith, [recs], [R.state()], count, "fold", general=general)
        assert active == 1 and np.isfinite(exp[0]["pose"]).all()


@pytest.mark.parametrize("count,hostile", [(2, 1), (9, 1), (150, 1), (9, 2), (33, 2), (160, 2)])
def test_fold_integer_slots_word_55_probe_words_and_wraps(ctx, O, arith, count, hostile):
    recs = GC.fold_records(count, hostile=hostile)
    exp, _ = check_all_forms(ctx, O, arith, [recs], [R.state()], count, "hostile", general=0)
    _, _, n, sr2 = R.fold(recs, count, 0)
    assert exp[0]["n_valid"] == n and (n < 0 if hostile == 1 else 0 < n < 1 << 20) and sr2 > 1 << 53
    check_all_forms(ctx, O, arith, [recs], [R.state()], count, "hostile general", general=1)


# ---------------------------------------------------------------- solve and exp behind either fold

def test_solve_cases_one_record_and_nine(ctx, O, arith):
    cases = GC.solve_cases()
    names = [(n, p) for n in cases for p in range(len(GC.PRIOR_POSES))]
    states = np.array([R.state(pose=GC.PRIOR_POSES[p]) for _, p in names], R.STATE_DTYPE)
    for general in (0, 1):                    # b with the gain, and without
        results = []
        for split in (False, True):
            recs = [GC.system_records(cases[n][0], cases[n][1], err_num=321.5, split=split) for n, _ in names]
            exp, active = check_all_forms(ctx, O, arith, recs, states, 9 if split else 1, "solve", general=general)
            assert active == len(names)       # a singular system is a step too (delta = 0)
            results.append(exp)
        same_bits(results[0], results[1], "one record against nine")
        for (n, p), st in zip(names, results[0]):
            assert st["iters"] == 1 and st["n_valid"] == 100 and not st["level_done"]
            if cases[n][2] is not None and p < len(GC.UNIT_POSES):
                assert np.array_equal(st["pose"], np.float32(GC.PRIOR_POSES[p])), n     # the pose as it came


def test_exp_cases_one_record_and_nine(ctx, O, arith):
    cases = GC.exp_cases()
    states = np.array([R.state(pose=prior) for _, _, prior in cases], R.STATE_DTYPE)
    for split in (False, True):
        recs = [GC.system_records(np.eye(6), -xi.astype(np.float64), split=split) for _, xi, _ in cases]
        exp, active = check_all_forms(ctx, O, arith, recs, states, 9 if split else 1, "exp", gain=1.0)
        assert active == len(cases)
        for (name, xi, prior), st in zip(cases, exp):
            assert st["pose"].tobytes() == O.se3_mul(prior, O.se3_exp(xi)).tobytes(), name


# ---------------------------------------------------------------- exit logic

def test_exit_logic_every_clause(ctx, O, arith):
    recs = [GC.system_records(np.eye(6), [1, 1, 1, 0, 0, 0], n_valid=128, sum_r2=512, err_num=256.0)]   # error 4, or 2 from slot 29
    pose = GC.OFF_UNIT_POSE

    def case(what, last, done, forms=FORMS, st=None, records=recs, **kw):
        st = R.state(pose=pose, last_error=last) if st is None else st
        exp, active = check_all_forms(ctx, O, arith, records, [st], 1, what, forms=forms, **{**dict(early_exit=1, epsilon=0.5), **kw})
        assert bool(exp[0]["level_done"]) == done and active == (0 if done else 1), what
        if done:
            assert np.array_equal(exp[0]["pose"], np.float32(pose)), what
        return exp[0]

    assert case("first", 50000.0, False)["error"] == 4.0
    assert case("error == last_error", 4.0, True)["last_error"] == 4.0
    case("k == max_iters - 1", 50000.0, True, k=49)
    case("k == max_iters - 2", 50000.0, False, k=48)
    case("|error - last| == epsilon", 4.5, False)
    case("|error - last| one float below epsilon", np.nextafter(np.float32(4.5), np.float32(0)), True)
    case("epsilon one float above |error - last|", 4.5, True, epsilon=np.nextafter(np.float32(0.5), np.float32(1)))
    case("early_exit = 0 ignores all three", 4.0, False, early_exit=0, k=49, epsilon=100.0)
    g = case("general: error from slot 29, b without gain", 50000.0, False, general=1)
    assert g["error"] == 2.0 and g["pose"].tobytes() == O.se3_mul(np.float32(pose), np.float32([0, 0, 0, 1, -1, -1, -1])).tobytes()
    junk = [GC.system_records(np.eye(6), [1, 1, 1, 0, 0, 0], n_valid=128, sum_r2=512, err_num=np.nan)]
    i = case("identity kind: slot 29 ignored", 50000.0, False, records=junk, general=0)
    assert i["error"] == 4.0 and i["pose"].tobytes() == O.se3_mul(np.float32(pose), np.float32([0, 0, 0, 1, -50, -50, -50])).tobytes()
    empty = [GC.system_records(np.eye(6), np.ones(6), n_valid=0)]
    e = case("no valid point", 50000.0, True, records=empty)
    assert e["status"] == 2 and e["iters"] == 1 and e["n_valid"] == 0 and e["error"] == 0 and e["last_error"] == 50000.0
    # a pair that arrives finished: the block form returns it as it came.  (The tail form's callers draw no ticket for such a pair —
    # their blocks leave before the record — so the stage kernel, which draws one for every pair, has nothing to say about it.)
    for st in (R.state(pose=pose, level_done=1, iters=7, n_valid=5, error=3.0), R.state(pose=pose, status=2, iters=1)):
        got, active = run(ctx, 0, 0, recs, [st], 1, early_exit=1)
        assert got[0].tobytes() == st.tobytes() and active == 0


# ---------------------------------------------------------------- a batch behind a pair_base

def test_batch_of_pairs_behind_a_pair_base(ctx, O, arith):
    count = 33
    meaningful = [1, 9, 17, 33, 20]
    pair_records = []
    for i, m in enumerate(meaningful):
        recs = np.zeros((count, R.REC_WORDS), np.uint32)        # +0.0 / 0 records behind the meaningful ones
        recs[:m] = GC.fold_records(m, seed=5 + i)
        pair_records.append(recs)
    pair_records[4][:, 54] = 0                                  # pair 4: no valid point
    states = np.array([R.state(pose=GC.PRIOR_POSES[i % 3], last_error=1e30 if i != 2 else 0.0, iters=i) for i in range(5)], R.STATE_DTYPE)
    lead = np.array([R.state(pose=(9, 9, 9, 9, 9, 9, 9), iters=77), R.state(level_done=1, status=3)], R.STATE_DTYPE)
    kw = dict(early_exit=1, general=0)
    exp, active = expect(O, arith, 1, pair_records, states, count, **kw)
    assert active == 3 and [int(s["level_done"]) for s in exp] == [0, 0, 1, 0, 1]       # pair 2 stops on its error, pair 4 on n == 0
    for form, pad in FORMS:
        got, act = run(ctx, form, pad, pair_records, states, count, pair_base=2, lead_states=lead, **kw)
        same_bits(got, exp, ("batch", form, pad))
        assert act == active
        for i in range(5):
            alone, a1 = run(ctx, form, pad, [pair_records[i]], [states[i]], count, **kw)
            assert alone[0].tobytes() == got[i].tobytes() and a1 == (0 if exp[i]["level_done"] else 1)


# ---------------------------------------------------------------- non-finite sums

def test_non_finite_sums(ctx, O, arith):
    """+Inf in a sum of A, NaN in a sum of J^T r (tests/test_gn_update_cpu.py: the restatement and the oracle agree on both): the NaN
    mask and the bits of every finite field"""
    from test_gn_update_cpu import nonfinite_cases
    for name, (A, jtr) in nonfinite_cases().items():
        recs = [GC.system_records(A, jtr)]
        exp, _ = expect(O, arith, 1, recs, [R.state(pose=GC.OFF_UNIT_POSE)], 1)
        for form, pad in FORMS:
            got, active = run(ctx, form, pad, recs, [R.state(pose=GC.OFF_UNIT_POSE)], 1)
            assert active == 1
            for field in R.STATE_DTYPE.names:
                g, e = np.atleast_1d(got[0][field]), np.atleast_1d(exp[0][field])
                if g.dtype.kind == "f":
                    assert np.array_equal(np.isnan(g), np.isnan(e)), (name, form, field, g, e)
                    ok = ~np.isnan(e)
                    assert g[ok].tobytes() == e[ok].tobytes(), (name, form, field, g, e)
                else:
                    assert np.array_equal(g, e), (name, form, field)


# ---------------------------------------------------------------- arguments

@pytest.mark.one_arith
def test_bad_arguments_are_refused_and_leave_the_outputs_alone(capi, ctx):
    lib = capi.lib()
    recs = np.zeros((3, 4, R.REC_WORDS), np.uint32)
    st = np.zeros(3, R.STATE_DTYPE)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def call(form=0, n_pairs=3, pair_base=0, stride=4, count=4, records=recs, states=st):
        out = np.full(3, 0x5a, np.uint8).repeat(R.STATE_DTYPE.itemsize).view(R.STATE_DTYPE)
        tickets = np.full(3, 0x5a5a5a5a, np.uint32)
        active = C.c_int32(-7)
        rc = lib.uwt_gn_update_records(ctx._h, form, n_pairs, pair_base, stride, count, None if records is None else P(records, C.c_uint32),
                                       None if states is None else P(states, capi.PairState), 0, 50, 1, C.c_float(1e-3), C.c_float(50.0), 0,
                                       P(out, capi.PairState), C.byref(active), P(tickets, C.c_uint32))
        untouched = active.value == -7 and (tickets == 0x5a5a5a5a).all() and (out.view(np.uint8) == 0x5a).all()
        return rc, untouched

    assert call() == (0, False)
    bad = [dict(form=2), dict(form=-1), dict(n_pairs=0), dict(pair_base=-1), dict(n_pairs=1025), dict(pair_base=1024, n_pairs=1),
           dict(count=0), dict(count=161, stride=161), dict(stride=3, count=4), dict(form=0, stride=4, count=3), dict(form=1, stride=257, count=4),
           dict(records=None), dict(states=None)]
    for kw in bad:
        assert call(**kw) == (capi.ERR_INVALID_ARG, True), kw
    assert call(form=1, stride=4, count=3) == (0, False)
