"""CPU tests of the Gauss-Newton update's restatement (tests/gn_update_ref.py) and of the inputs the GPU tests feed to
uwt_gn_update_records (tests/gn_update_cases.py): the restatement against references of higher precision (math.fsum, exact rationals,
numpy's f64 solve, scipy's expm), and the inputs against the wrong kernels they are meant to catch.

Tolerances are those of tests/test_oracle.py: the solve rtol 2e-2, atol 1e-6 * |ref|max (test_inv6_matches_numpy_and_singular_is_zero),
the exponential 2e-6 * max(1, |ref|) and unit norm to 1e-6 (test_se3_exp_matches_expm), the composition 5e-6 * max(1, |ref|)
(test_se3_mul_matches_matrix_product).  No new case needed more.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import linalg

import gn_update_cases as GC
import gn_update_ref as R
from test_oracle import hat6

ARGS = dict(k=0, max_iters=50, early_exit=0, epsilon=1e-3, gain=50.0)


def bits(st):
    return np.asarray(st).tobytes()


# ---------------------------------------------------------------- fold

@pytest.mark.parametrize("count", GC.FOLD_COUNTS)
def test_fold_is_a_sum_and_its_inputs_tell_the_orders_apart(O, arith, count):
    recs = GC.fold_records(count)
    f = recs.view(np.float64)
    mags = set()
    differs = {"sequential": 0, "swap12": 0, "reversed": 0}
    for slot in list(range(R.N_SUMS)) + [29]:
        vals = [float(f[q, slot]) for q in range(count)]
        got = R.fold_values(vals)
        assert abs(float(got) - math.fsum(vals)) <= (count - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in vals)   # the standard bound
        mags.update(math.frexp(v)[1] for v in vals)
        assert count < 3 or (min(vals) < 0 < max(vals))
        for order in differs:
            differs[order] += R.fold_values(vals, order).tobytes() != got.tobytes()
    if count >= 17:
        assert max(mags) - min(mags) >= 55   # ~2^60 between the smallest and the largest value
    # the inputs prove something only if a wrong order shows: in the sums ...
    # (up to 8 records every part is one record and the stated order IS the record order: the sequential fold can differ from 9 on;
    # below that the final pass taken from part 7 down stands for a wrong order)
    if count >= 3:
        assert differs["reversed"] >= 1
    assert differs["sequential"] >= 1 if count >= 9 else differs["sequential"] == 0
    if count >= 10:
        assert differs["swap12"] >= 1
    # ... and in what the entry returns (the sums pass through (float) before the solve: the cancelling pairs keep the difference large)
    for general in (0, 1):
        st, step = R.update(O, R.state(), recs, count, general=general, arith=arith, **ARGS)
        assert step and np.isfinite(st["pose"]).all() and np.isfinite(st["error"])
        wrong = (["reversed"] if count >= 3 else []) + (["sequential"] if count >= 9 else []) + (["swap12"] if count >= 10 else [])
        for order in wrong:
            assert bits(R.update(O, R.state(), recs, count, general=general, arith=arith, order=order, **ARGS)[0]) != bits(st), order


@pytest.mark.one_arith
@pytest.mark.parametrize("count,hostile", [(2, 1), (9, 1), (150, 1), (9, 2), (33, 2), (160, 2)])
def test_fold_of_the_integer_slots(count, hostile):
    recs = GC.fold_records(count, hostile=hostile)
    _, _, n, sr2 = R.fold(recs, count, 0)
    low = [int(w) for w in recs[:, 54]]
    total = sum(low)
    assert (recs[:, 55] == 0xffffffff).all() and recs[:, 60:].any()
    assert total > (1 << 31) if hostile == 1 else total > (1 << 32)
    wrapped = total & 0xffffffff
    assert n == (wrapped - (1 << 32) if wrapped >> 31 else wrapped)       # through uint32, then int
    exact = sum(int(v) for v in recs.view(np.uint64)[:, 28])
    assert sr2 == exact and exact > (1 << 53) and float(exact) != exact    # the (double) of the tail rounds it
    # the same records read with word 55 as part of the count would fold to the same low word: the cast at the end makes the mask in
    # the loop redundant — nothing can tell the two apart, and this pins that
    assert sum(int(v) for v in recs.view(np.uint64)[:, 27]) & 0xffffffff == wrapped


# ---------------------------------------------------------------- solve

def exact_rank(A, rows=6):
    M = [[Fraction(float(v)) for v in row[:rows]] for row in np.asarray(A)[:rows]]
    rank = 0
    for c in range(rows):
        p = next((r for r in range(rank, rows) if M[r][c] != 0), None)
        if p is None:
            continue
        M[rank], M[p] = M[p], M[rank]
        for r in range(rank + 1, rows):
            fct = M[r][c] / M[rank][c]
            M[r] = [a - fct * b for a, b in zip(M[r], M[rank])]
        rank += 1
    return rank


def test_solve_cases_are_what_they_claim_and_solve_matches_numpy(O, arith):
    cases = GC.solve_cases()
    assert GC.EPS10 == np.float32(10 * 2.0 ** -23)
    for name, (A, jtr, singular_at) in cases.items():
        assert np.array_equal(A, A.T), name
        trace, at = R.lu_trace(A)
        assert at == singular_at, name
        b = (-50.0 * jtr.astype(np.float64)).astype(np.float32)
        d = R.solve(O, A, b, arith)
        assert d.tobytes() == O.solve_delta(A, b).tobytes(), name    # the oracle's own dispatch on the arithmetic set
        if singular_at is not None:
            assert d.tobytes() == np.zeros(6, np.float32).tobytes(), name
            assert not O.solve6(A, b)[1] and not O.inv6(A)[1]
        else:
            ref = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))
            assert np.allclose(d, ref, rtol=2e-2, atol=1e-6 * np.abs(ref).max()), (name, d, ref)
    for i in range(6):
        A = cases["rank_%d" % i][0]
        assert np.array_equal(A, np.round(A)) and np.abs(A).max() <= 64
        assert exact_rank(A) == i and exact_rank(A, i) == i      # rank i, carried by the leading i x i minor
    assert all(t[1] >= 2 for t in R.lu_trace(GC.TIES)[0][:5])                          # a tie for the pivot in every column
    assert all(t[0] != c for c, t in enumerate(R.lu_trace(GC.SWAPS)[0][:5]))           # a swap at every column
    for pos in (2, 5):
        assert R.lu_trace(cases["threshold_at_%d" % pos][0])[0][pos][2] == GC.EPS10
        assert R.lu_trace(cases["threshold_below_%d" % pos][0])[0][pos][2] == np.nextafter(GC.EPS10, np.float32(0))
    A = cases["jtj_0"][0]
    assert 1e5 < A[0, 0] / A[3, 3] < 1e7


def test_update_on_one_record_and_on_nine_is_the_same_step(O, arith):
    for name, (A, jtr, singular_at) in GC.solve_cases().items():
        for pose in GC.PRIOR_POSES:
            st0 = R.state(pose=pose)
            one, step1 = R.update(O, st0, GC.system_records(A, jtr), 1, general=0, arith=arith, **ARGS)
            nine, step9 = R.update(O, st0, GC.system_records(A, jtr, split=True), 9, general=0, arith=arith, **ARGS)
            assert step1 and step9 and bits(one) == bits(nine), name
            assert one["iters"] == 1 and one["n_valid"] == 100
            if singular_at is not None and tuple(pose) in [tuple(np.float32(p)) for p in GC.UNIT_POSES]:
                assert np.array_equal(one["pose"], np.array(pose, np.float32)), name    # delta = 0: the step is the identity
            if singular_at is None:
                assert not np.array_equal(one["pose"], np.array(pose, np.float32)), name
    # a singular system under a perturbed elimination — the pivot test below the row swap instead of above it changes nothing in the
    # result (zeros either way); what the rank cases do catch is a test that is not taken by every column alike: rank_3's step would
    # then not be the identity
    A, jtr, _ = GC.solve_cases()["rank_3"]
    assert np.linalg.matrix_rank(A.astype(np.float64)) == 3


# ---------------------------------------------------------------- exp and composition

def quat_norm2_of_product(a, b):
    """sn of se3_mul in f32: the squared norm of the Hamilton product, as the kernels add it"""
    f = np.float32
    ax, ay, az, aw = [f(v) for v in a[:4]]
    bx, by, bz, bw = [f(v) for v in b[:4]]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    return x * x + y * y + z * z + w * w


@pytest.mark.one_arith
def test_exp_cases_hit_their_thetas_and_match_expm(O):
    cases = GC.exp_cases()
    thetas = {float(GC.theta_of(xi[3:])) for _, xi, _ in cases}
    assert thetas == {float(t) for t in GC.theta_targets()} and len(thetas) == 17
    assert max(np.abs(xi[:3]).max() for _, xi, _ in cases) == 1e3 and min(np.abs(xi[:3]).max() for _, xi, _ in cases) == 0
    renorm = set()
    for name, xi, prior in cases:
        got = O.se3_exp(xi)
        ref = linalg.expm(hat6(xi.astype(np.float64)))
        assert np.allclose(O.se3_matrix(got).astype(np.float64), ref, atol=2e-6 * max(1.0, np.abs(ref).max())), name
        assert abs(np.linalg.norm(got[:4].astype(np.float64)) - 1) < 1e-6, name
        new = O.se3_mul(prior, got)
        prod = O.se3_matrix(prior).astype(np.float64) @ O.se3_matrix(got).astype(np.float64)
        assert np.allclose(O.se3_matrix(new), prod, atol=5e-6 * max(1.0, np.abs(prod).max())), name
        renorm.add(bool(quat_norm2_of_product(prior, got) != np.float32(1)))
    assert renorm == {False, True}    # both sides of "sn != 1.f"
    for p in GC.UNIT_POSES:
        assert quat_norm2_of_product(np.float32(p), np.float32([0, 0, 0, 1])) == np.float32(1)
    assert quat_norm2_of_product(np.float32(GC.OFF_UNIT_POSE), np.float32([0, 0, 0, 1])) != np.float32(1)


def test_identity_system_hands_the_twist_to_exp_unchanged(O, arith):
    """A = I, gain 1: delta = -jtr exactly under either set, so a record chooses the argument of exp freely"""
    for name, xi, prior in GC.exp_cases():
        recs = GC.system_records(np.eye(6), -xi.astype(np.float64))
        st, step = R.update(O, R.state(pose=prior), recs, 1, k=0, max_iters=50, early_exit=0, epsilon=1e-3, gain=1.0, general=0, arith=arith)
        assert step and st["pose"].tobytes() == O.se3_mul(prior, O.se3_exp(xi)).tobytes(), name
        nine, _ = R.update(O, R.state(pose=prior), GC.system_records(np.eye(6), -xi.astype(np.float64), split=True), 9, k=0, max_iters=50,
                           early_exit=0, epsilon=1e-3, gain=1.0, general=0, arith=arith)
        assert bits(nine) == bits(st), name


# ---------------------------------------------------------------- exit test (src/Tracker.cpp:508) and the two kinds of records

@pytest.mark.one_arith
def test_exit_test_at_equality(O):
    recs = GC.system_records(np.eye(6), [1, 1, 1, 0, 0, 0], n_valid=128, sum_r2=512, err_num=256.0)    # error 4 (identity kind), 2 (general)
    run = lambda last, **kw: R.update(O, R.state(last_error=last), recs, 1, arith="opencv", **{**dict(ARGS, early_exit=1, epsilon=0.5, general=0), **kw})
    st, step = run(50000.0)
    assert step and st["error"] == 4.0 and st["last_error"] == 4.0 and not st["level_done"] and st["iters"] == 1
    st, step = run(4.0)                                         # error == last_error
    assert not step and st["level_done"] == 1 and st["last_error"] == 4.0 and st["status"] == 0
    assert not run(50000.0, k=49)[1] and run(50000.0, k=48)[1]  # k == max_iters - 1
    assert run(4.5)[1]                                          # |error - last| == epsilon: not below it
    assert not run(np.nextafter(np.float32(4.5), np.float32(0)))[1]
    assert not run(4.5, epsilon=np.nextafter(np.float32(0.5), np.float32(1)))[1]
    st, step = run(4.0, early_exit=0, k=49)                     # early_exit = 0: none of the three
    assert step and not st["level_done"] and st["last_error"] == 4.0
    st, step = run(50000.0, general=1)
    assert st["error"] == 2.0 and np.array_equal(st["pose"][4:], -np.ones(3, np.float32))    # b = -jtr, no gain
    st, step = run(50000.0, general=0)
    assert st["error"] == 4.0 and np.array_equal(st["pose"][4:], -50 * np.ones(3, np.float32))
    st, step = R.update(O, R.state(pose=GC.OFF_UNIT_POSE), GC.system_records(np.eye(6), np.ones(6), n_valid=0), 1, general=0, arith="opencv", **ARGS)
    assert not step and st["status"] == 2 and st["level_done"] == 1 and st["iters"] == 1 and st["n_valid"] == 0
    assert np.array_equal(st["pose"], np.float32(GC.OFF_UNIT_POSE)) and st["error"] == 0 and st["last_error"] == 50000.0
    done = R.state(level_done=1, iters=7)
    assert bits(R.update(O, done, recs, 1, general=0, arith="opencv", block_form=True, **ARGS)[0]) == bits(done)


# ---------------------------------------------------------------- non-finite sums

def nonfinite_cases():
    A = np.eye(6) * 4.0
    A[0, 1] = A[1, 0] = np.inf
    jtr = np.arange(1.0, 7.0)
    jn = jtr.copy()
    jn[2] = np.nan
    return {"inf_in_A": (A, jtr), "nan_in_jtr": (np.eye(6) * 4.0, jn)}


def test_restatement_and_oracle_agree_on_non_finite_sums(O, arith):
    for name, (A, jtr) in nonfinite_cases().items():
        A32 = A.astype(np.float32)
        with np.errstate(all="ignore"):
            b = (-50.0 * jtr).astype(np.float32)
            mine, theirs = R.solve(O, A32, b, arith), O.solve_delta(A32, b)
        assert np.array_equal(np.isnan(mine), np.isnan(theirs)), name
        ok = ~np.isnan(mine)
        assert mine[ok].tobytes() == theirs[ok].tobytes(), name
