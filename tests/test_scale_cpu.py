"""The robust scale stage on designed residual histograms, CPU side: the plain restatement (tests/scale_ref.py) against the oracle
and against exact arithmetic; every case of tests/scale_cases.py reaches what it was written for; and the set of cases tells the
rule from its near misses (mutants), in the scale and in the normal equations the pose-level GPU comparisons see."""
from fractions import Fraction

import numpy as np
import pytest

import scale_cases as S
import scale_ref as R

ARITH_INDEPENDENT = True       # residuals, medians and weights do not depend on the arithmetic set; the sums are only compared with themselves
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def evals(O):
    """{(case id, level): (J, r, idx)} of every case, once"""
    out = {}
    for c in S.CASES:
        for lvl in range(S.SIZES[c.size][3]):
            out[(c.id, lvl)] = S.evaluate(O, c, lvl)[:3]
    return out


# ---------------------------------------------------------------- reach

def test_every_case_reaches_its_target_on_every_level(O, evals):
    for c in S.CASES:
        for lvl in range(S.SIZES[c.size][3]):
            J, r, idx = evals[(c.id, lvl)]
            assert np.array_equal(r, S.level_map(c, lvl).reshape(-1)[idx].astype(F)), (c, lvl)      # r == q on the valid pixels
            med, dmed, mad, inv_mad, n = R.scale(r, c.kind)
            assert (med, dmed) == tuple(c.target), (c, lvl, med, dmed)
            assert c.n is None or n == c.n, (c, lvl, n)
            if c.n is None and not c.has_depth:
                w, h = S.SIZES[c.size][:2]
                assert n == ((w >> lvl) - 1) * ((h >> lvl) - 1)         # row 0 and column 0 never count


def test_every_family_has_its_twins_and_every_listed_branch_a_case():
    ids = {c.id for c in S.CASES}
    assert len(ids) == len(S.CASES)
    for fam in S.FAMILIES:
        mine = [c for c in S.CASES if c.family == fam]
        assert any(c.size == "twin" for c in mine) and any(np.ndim(c.depth) == 0 and c.depth is not None for c in mine), fam
    t = {(c.kind, ) + tuple(c.target) for c in S.CASES if c.n != 0}
    tuk = {x[2] for x in t if x[0] == S.TUKEY and x[1] == 0}
    hub = {x[2] for x in t if x[0] == S.HUBER}
    for d in range(7, 255, 8):                      # both sides of every lane boundary of the deviation walk
        assert {d, d + 1} <= tuk and {d, d + 1} <= hub, d
    for d in range(255, 510, 8):
        assert {d, d + 1} <= hub or d + 1 > 510, d
    assert {509, 510} <= hub and max(hub) == S.HUBER_DMED_LIMIT == R.DEV_CLAMP[S.HUBER]     # the limit found: 510, not 255
    assert max(x[2] for x in t if x[0] == S.TUKEY) == S.TUKEY_DMED_LIMIT == R.DEV_CLAMP[S.TUKEY]
    tm = {x[1] for x in t if x[0] == S.TUKEY}
    hm = {x[1] for x in t if x[0] == S.HUBER}
    for m in range(7, 255, 8):
        assert {m, m + 1} <= tm, m
    for m in range(-248, 255, 8):
        assert {m, m + 1} <= hm, m
    assert 255 in tm and {-255, 255} <= hm
    for n in (0, 1, 2, 3, 1000, 1001):
        assert any(c.n == n for c in S.CASES), n


@pytest.mark.parametrize("kind", [S.TUKEY, S.HUBER], ids=["tukey", "huber"])
def test_weight_sweep_reaches_every_deviation_and_every_residual_value(O, kind):
    for c in S.sweep_cases(kind):
        J, r, idx, ng = S.evaluate(O, c, 0)
        assert np.array_equal(r, S.level_map(c, 0).reshape(-1)[idx].astype(F))
        assert set(r.astype(int).tolist()) == set(range(-255, 256)) and r.size == 63 * 47
        assert R.scale(r, kind)[:2] == tuple(c.target) == (0, int(c.name[1:]))


# ---------------------------------------------------------------- the restatement against the oracle

def test_restatement_equals_the_oracle_on_every_case(O, evals):
    for c in S.CASES:
        for lvl in range(S.SIZES[c.size][3]):
            J, r, idx = evals[(c.id, lvl)]
            med, dmed, mad, inv_mad, n = R.scale(r, c.kind)
            if n == 0:
                # MedianMat of nothing leaves its -1 and the reference divides by zero further on (src/Tracker.cpp:499-502); the
                # project's rule for an evaluation without a valid pixel is scale 1 and status 2, which the alignment tests compare
                assert O.median_mat(r) == -1.0 and mad == 1 and inv_mad == 1
                continue
            if c.kind == S.TUKEY:
                assert O.median_mat(r) == med and F(O.mad(r)) == R.C_MAD * F(dmed), (c, lvl)
                want = O.tukey_weights(r)
            else:
                want = O.huber_weights(r)
            assert np.array_equal(bits(R.weights(c.kind, r, inv_mad)), bits(want)), (c, lvl)


@pytest.mark.parametrize("kind", [S.TUKEY, S.HUBER], ids=["tukey", "huber"])
def test_restatement_equals_the_oracle_on_the_weight_sweep(O, kind):
    for c in S.sweep_cases(kind):
        r = S.evaluate(O, c, 0)[1]
        want = O.tukey_weights(r) if kind == S.TUKEY else O.huber_weights(r)
        assert np.array_equal(bits(R.weights(kind, r, R.scale(r, kind)[3])), bits(want)), c


# ---------------------------------------------------------------- the restatement against exact arithmetic

def rn(x, nbits):
    """the rational x rounded to the nearest binary float of nbits significant bits, ties to even (normal range)"""
    x = Fraction(x)
    if x == 0:
        return x
    s, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (e - nbits + 1)
    k = x / ulp
    f = k.numerator // k.denominator
    rem = k - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return s * f * ulp


def fr(x):
    return Fraction(float(x))


def inv_mads(limit):
    out = {}
    for d in range(limit + 1):
        mad = R.C_MAD * F(d) if d else F(1)
        assert fr(mad) == (rn(fr(R.C_MAD) * d, 24) if d else 1)
        out[d] = F(np.float64(1.0) / np.float64(mad))
        assert fr(out[d]) == rn(rn(1 / fr(mad), 53), 24), d       # the correctly rounded double reciprocal, rounded to f32
    return out


def test_inv_mad_and_huber_quotient_are_correctly_rounded():
    """every (|r|, dmed) of integer residuals: dmed 0..510, |r| 1..255"""
    k = fr(R.HUBER_K)
    n_quot = 0
    for d, inv in inv_mads(510).items():
        for a in range(1, 256):
            ax = abs(F(a) * inv)
            assert fr(ax) == rn(a * fr(inv), 24)
            w = R.huber_weight(F(-a), inv)
            assert w.dtype == F and w == R.huber_weight(F(a), inv)
            if fr(ax) <= k:
                assert w == 1
            else:
                assert fr(w) == rn(k / fr(ax), 24), (d, a)          # the IEEE quotient k / ax
                n_quot += 1
    assert n_quot > 10000          # the quotient is used wherever |r| > 1.345 MAD


def test_tukey_steps_are_correctly_rounded():
    """every (|r|, dmed) of integer residuals under Tukey: dmed 0..255, |r| 0..255"""
    b = fr(R.TUKEY_B)
    bb = F(R.TUKEY_B * R.TUKEY_B)
    assert fr(bb) == rn(b * b, 24)
    inv_b2 = rn(rn(1 / fr(bb), 53), 24)
    n_in = n_out = 0
    for d, inv in inv_mads(255).items():
        for a in range(0, 256):
            w = R.tukey_weight(F(a), inv)
            assert w.dtype == F and w == R.tukey_weight(F(-a), inv)
            x = rn(a * fr(inv), 24)
            if x <= b:
                y = rn(rn(x * x, 24) * inv_b2, 24)
                t = rn(rn(1 - y, 53), 24)
                assert fr(w) == rn(t * t, 24), (d, a)
                n_in += 1
            else:
                assert w == 0
                n_out += 1
    assert n_in > 10000 and n_out > 1000           # both sides of the cut-off |x| <= b


def test_weighted_terms_are_the_stated_products():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        r, w, gain = F(rng.integers(-255, 256)), F(rng.random()), F(50.0)
        rw, e = R.weighted_terms(r, w, gain)
        assert rw.dtype == F and fr(rw) == rn(rn(fr(r) * fr(gain), 24) * fr(w), 24)
        assert e.dtype == np.float64 and fr(e) == fr(r) * rn(fr(r) * fr(w), 24)         # the f64 product is exact


# ---------------------------------------------------------------- discrimination

MUTANTS = ["ge", "n_plus_1", "no_carry", "not_smallest", "no_neg_sat", "no_dev_clamp", "high_side", "low_side", "zero_twice", "mad0_kept",
           "n0_not_special"]


def crossing(v, m, mut):
    """the wave form of "first bin whose cumulative count exceeds m": 64 lanes of 8 bins, the lane totals carried by a scan, every lane
    reporting its first crossing and the smallest report winning — with the mutations ge, no_carry, not_smallest"""
    reports = []
    before = 0
    for lane in range(64):
        cum = 0 if mut == "no_carry" else before
        for k in range(8):
            cum += v[lane * 8 + k]
            if (F(cum) >= m) if mut == "ge" else (F(cum) > m):
                reports.append(lane * 8 + k)
                break
        before += sum(v[lane * 8:lane * 8 + 8])
    if not reports:
        return None
    return max(reports) if mut == "not_smallest" else min(reports)


def rule(h, kind, mut=None):
    """(med, dmed, inv_mad) from the 511 signed bins h[q + 255], as uwt_kernels.h states the rule, with one mutation"""
    n = int(sum(h))
    m = F((n + 1) // 2 if mut == "n_plus_1" else n // 2)
    tukey = kind == S.TUKEY
    if tukey:
        v = [0] * 512
        v[0] = h[255] if mut == "no_neg_sat" else sum(h[:256])
        for t in range(1, 256):
            v[t] = h[t + 255]
        idx = crossing(v, m, mut)
        med = 255 if idx is None else idx
    else:
        idx = crossing(list(h) + [0], m, mut)
        med = 255 if idx is None else idx - 255
    dmax = 255 if tukey and mut != "no_dev_clamp" else 510
    v = [0] * 512
    for d in range(min(dmax, 511)):
        lo, hi = med - d, med + d
        if -255 <= lo <= 255:
            v[d] += h[lo + 255]
        elif mut == "low_side" and lo < -255:
            v[d] += h[0]
        if (d > 0 or mut == "zero_twice") and -255 <= hi <= 255:
            v[d] += h[hi + 255]
        elif mut == "high_side" and hi > 255:
            v[d] += h[510]
    idx = crossing(v, m, mut)
    dmed = dmax if idx is None else idx
    mad = R.C_MAD * F(dmed)
    if (n == 0 and mut != "n0_not_special") or (mad == 0 and mut != "mad0_kept"):
        mad = F(1)
    with np.errstate(divide="ignore"):
        return med, dmed, F(np.float64(1.0) / np.float64(mad))


def histogram(r):
    h = [0] * 511
    for v, c in zip(*np.unique(np.rint(r).astype(int), return_counts=True)):
        h[int(v) + 255] += int(c)
    return h


def test_every_mutant_of_the_rule_is_killed_in_the_scale_and_in_the_normal_equations(O, evals):
    lvl = 1
    hists = {c.id: histogram(evals[(c.id, lvl)][1]) for c in S.CASES}
    for c in S.CASES:                                   # the unmutated wave form is the restatement
        med, dmed, mad, inv_mad, n = R.scale(evals[(c.id, lvl)][1], c.kind)
        got = rule(hists[c.id], c.kind)
        assert got[2].tobytes() == inv_mad.tobytes() and (n == 0 or got[:2] == (med, dmed)), c
    killed = {}
    for mut in MUTANTS:
        killed[mut] = []
        for c in S.CASES:
            inv = rule(hists[c.id], c.kind)[2]
            inv_m = rule(hists[c.id], c.kind, mut)[2]
            if inv_m.tobytes() == inv.tobytes():
                continue
            J, r, idx = evals[(c.id, lvl)]
            with np.errstate(all="ignore"):
                A0, b0 = O.normal_equations(J, r, R.weights(c.kind, r, inv))
                A1, b1 = O.normal_equations(J, r, R.weights(c.kind, r, inv_m))
            if A0.tobytes() != A1.tobytes() or b0.tobytes() != b1.tobytes():
                killed[mut].append(c.id)
            elif mut == "n0_not_special":
                assert r.size == 0
                killed[mut].append(None)
    # Two mutants cannot show in a pose.  n == 0: there is no pixel to weight; the scale is read directly by the per-stage GPU
    # comparison (inv_mad).  The low side counted below -255: a bin d with med - d < -255 lies behind the crossing whatever it
    # holds (scale_cases.py: the values <= med exceed n / 2 and all deviate by less than such a d), so the mutant computes the same
    # function; what the check guards is the read outside the 511 bins, not a value.
    assert killed.pop("n0_not_special") and killed.pop("low_side") == []
    for mut, ids in killed.items():
        assert ids, mut
