"""tests/table_f32_ref.py without a device: its fused multiply-add rounds once (against exact rational arithmetic, on random operands and
on operands built to sit on an f32 rounding midpoint, where rounding through f64 goes wrong), rows go to the threads the kernel gives
them, and the f32 chains leave sums that differ from the f64 sums by no more than four roundings per thread — so the GPU test that
uses it tells the f32 form from the f64 form."""
from fractions import Fraction

import numpy as np

import table_f32_ref as TF

ARITH_INDEPENDENT = True


def rn32(x):
    """a Fraction rounded to the nearest float32, ties to the even mantissa"""
    c = np.float32(float(x))
    cands = {float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))}
    return min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))


def test_fma32_rounds_once():
    f = np.float32
    u = f(2.0) ** -23
    a0, b0 = f(2.0) ** -12 * (f(1) + u), f(2.0) ** -12 * (f(1) - u)      # a0 * b0 = 2^-24 - 2^-70: just below half an ulp of 1
    tie = [(a0, b0, f(1) + u), (-a0, b0, -(f(1) + u)), (a0, b0, f(1)), (f(2.0) ** -24, f(1), f(1) + u), (f(2.0) ** -24, f(1), f(1))]
    through_f64 = np.float32(np.float64(a0) * np.float64(b0) + np.float64(f(1) + u))
    assert TF.fma32(a0, b0, f(1) + u) == f(1) + u and through_f64 == f(1) + f(2) * u          # the case rounding twice gets wrong
    rng = np.random.default_rng(3)
    a = (rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(f)
    b = (rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(f)
    c = np.where(rng.random(4000) < 0.3, -(a * b), rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(f)   # cancellation too
    a, b, c = (np.concatenate([x, np.array([t[i] for t in tie], f)]) for i, x in enumerate((a, b, c)))
    got = TF.fma32(a, b, c)
    for i in range(len(a)):
        want = rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert float(got[i]) == want, (i, a[i], b[i], c[i], got[i], want)


def test_rows_threads_and_sums():
    rng = np.random.default_rng(11)
    n_rows = 1610
    idx = np.sort(rng.choice(n_rows, 1400, replace=False))
    J = rng.normal(0, 30, (len(idx), 6)).astype(np.float32)
    r = rng.integers(-255, 256, len(idx)).astype(np.float32)
    acc = TF.thread_sums(J, r, idx, n_rows)
    assert acc.shape == (2, 256, 27)
    # thread 5 of block 1 owns rows 1029, 1285, 1541 (1797 is past the table): its chain, written out
    want = np.zeros(27, np.float32)
    for q in (1029, 1285, 1541, 1797):
        at = np.flatnonzero(idx == q)
        if len(at):
            row, res = J[at[0]], r[at[0]]
            for s, (i, j) in enumerate(TF.PAIRS):
                want[s] = TF.fma32(row[i], row[j], want[s])
            for i in range(6):
                want[21 + i] = TF.fma32(row[i], res, want[21 + i])
    assert np.array_equal(acc[1, 5].view(np.uint32), want.view(np.uint32)) and want.any()
    # a block's sum takes every thread's value once, whatever the start of its segments
    vals = rng.normal(0, 1, 256).astype(np.float32)
    for s in (0, 13, 14, 26):
        assert abs(TF.block_sum(vals, s) - vals.astype(np.float64).sum()) <= 256 * 2.0 ** -53 * np.abs(vals).sum()
    # against the f64 sums of the same rows: within four f32 roundings per thread of the magnitudes, and not equal
    S = np.array(TF.sums(J, r, idx, n_rows))
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    exact = np.array([(Jd[:, i] * Jd[:, j]).sum() for i, j in TF.PAIRS] + [(Jd[:, i] * rd).sum() for i in range(6)])
    mag = np.array([np.abs(Jd[:, i] * Jd[:, j]).sum() for i, j in TF.PAIRS] + [np.abs(Jd[:, i] * rd).sum() for i in range(6)])
    assert (np.abs(S - exact) <= 4 * 2.0 ** -24 * mag).all() and (S.astype(np.float32) != exact.astype(np.float32)).any()
    A, b = TF.normal_equations(J, r, idx, n_rows, 50.0)
    assert np.array_equal(A, A.T) and A[0, 1] == np.float32(S[1]) and b[2] == np.float32(-(50.0 * S[23]))
