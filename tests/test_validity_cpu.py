"""The designed cases of the warp and validity stage (tests/validity_cases.py) on the CPU: the numpy restatement
(tests/validity_ref.py) equals the oracle bit for bit on every case, the exact cases equal rational arithmetic, every case reaches the
classes it declares, and every deliberate mistake in the restatement (validity_ref.MUTANTS) is noticed by a NAMED case.  Twelve of the
thirteen named cases also go to the device (tests/test_gpu_validity.py), which then cannot pass with that mistake in a kernel; the
thirteenth, `iz < 0` -> `<= 0`, is noticed only by table_minus_inf (z2 = -inf, legacy set), a case the device is not given: no device
test tells the two comparisons apart, and for finite z2 nothing can (1 / z2 is never a zero).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import metric_ref as MR
import validity_cases as VC
import validity_ref as VR

ARITH = {"opencv": VR.OPENCV, "legacy": VR.LEGACY}
FACTORS = ((1.0, 1.0), (0.5, 1.25))

_eval = {}


def evaluated(O, case, arith, lvl):
    """(warp, evaluation) of the restatement on one level of a case, made once"""
    key = (case.name, arith, lvl)
    if key not in _eval:
        L, i1, i2, gx, gy, pts = VC.level_inputs(O, case, lvl)
        wp = VR.warp(pts, case.pose, L, ARITH[arith])
        _eval[key] = (wp, VR.evaluate(i1, i2, gx, gy, pts, wp, L, ARITH[arith]))
    return _eval[key]


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.name)
def test_restatement_equals_oracle(O, arith, case):
    """warp (NaN payloads apart), residual_jacobian, residual_jacobian_ex with the bilinear sampler and non-unit factors, and the metric
    mode against tests/metric_ref.py over the oracle: the valid set, r and J bit for bit on every level"""
    for lvl in VC.levels_of(case):
        L, i1, i2, gx, gy, pts = VC.level_inputs(O, case, lvl)
        wp, ev = evaluated(O, case, arith, lvl)
        wo = O.warp(pts, case.pose, L)
        assert VR.same_bits(wp, wo, nan_equal=True), (case.name, lvl)
        J, r, idx = O.residual_jacobian(i1, i2, gx, gy, pts, wo, L)
        Jr, rr, ir = VR.compressed(ev)
        assert np.array_equal(idx, ir) and VR.same_bits(J, Jr) and VR.same_bits(r, rr), (case.name, lvl)
        for zf, af in FACTORS:
            for sampler in (0, 1):
                for metric in (False, True):
                    J, r, idx = MR.MetricOracle(O, metric).residual_jacobian_ex(i1, i2, gx, gy, pts, wo, L, zf, af, sampler)
                    Jr, rr, ir = VR.compressed(VR.evaluate(i1, i2, gx, gy, pts, wp, L, ARITH[arith], zf, af, sampler, metric))
                    assert np.array_equal(idx, ir) and VR.same_bits(J, Jr) and VR.same_bits(r, rr), (case.name, lvl, zf, af, sampler, metric)


def exact_warp(pts, pose, L):
    """(u, v, z2) of every row in rational arithmetic from the float32 inputs (None where z2 == 0)"""
    T = [[Fraction(float(t)) for t in row] for row in VR.rigid_matrix(pose)]
    fx, fy, cx, cy, ifx, ify = (Fraction(float(v)) for v in (L.fx, L.fy, L.cx, L.cy, L.invfx, L.invfy))
    out = []
    for x, y, z, w in ([Fraction(float(v)) for v in row] for row in pts):
        P = ((x - cx) * ifx * z, (y - cy) * ify * z, z, w)
        o = [sum(T[k][j] * P[j] for j in range(4)) for k in range(3)]
        out.append(None if o[2] == 0 else ((o[0] * fx / o[2] + cx) * w, (o[1] * fy / o[2] + cy) * w, o[2]))
    return out


@pytest.mark.parametrize("case", [c for c in VC.CASES if "exact" in c.tags], ids=lambda c: c.name)
def test_exact_cases_equal_rational_arithmetic(O, arith, case):
    """on the cases built to be exact, u, v and z2 of BOTH arithmetic sets are the rational numbers: no operation of the warp rounds"""
    for lvl in VC.levels_of(case):
        L, _, _, _, _, pts = VC.level_inputs(O, case, lvl)
        wp, _ = evaluated(O, case, arith, lvl)
        for i, want in enumerate(exact_warp(pts, case.pose, L)):
            assert want is not None
            got = tuple(Fraction(float(v)) for v in wp[i, :3])
            assert got == want, (case.name, lvl, i, wp[i], [float(v) for v in want])


@pytest.mark.parametrize("case", VC.CASES, ids=lambda c: c.name)
def test_case_reaches_its_classes(O, arith, case):
    assert set(case.reach) <= set(VC.levels_of(case))
    for lvl, classes in case.reach.items():
        L, _, _, _, _, pts = VC.level_inputs(O, case, lvl)
        wp, ev = evaluated(O, case, arith, lvl)
        got = VC.classify(wp, ev, L, pts)
        assert all(got[k] > 0 for k in classes), (case.name, lvl, {k: got[k] for k in classes})


def test_every_class_is_reached_on_levels_0_and_2(O, arith):
    """the classes the stage's shortcuts turn on, each on a level of whole rows and on the coarsest level (beyond_grid exists on 46 x 35's
    level 2 alone; the float32 below one half needs cx = 0, which only level 0 has; tiny_z2 needs an integer principal point)"""
    seen = {0: set(), 2: set()}
    for case in VC.NORMAL:
        for lvl in set(VC.levels_of(case)) & {0, 2}:
            L, _, _, _, _, pts = VC.level_inputs(O, case, lvl)
            got = VC.classify(*evaluated(O, case, arith, lvl), L, pts)
            seen[lvl] |= {k for k, n in got.items() if n}
    both = {"u_eq_0", "u_eq_iw", "v_eq_0", "v_eq_ih", "clamp_x", "clamp_y", "tie_x", "tie_y", "lt_half_x", "lt_half_y", "last_cell_x",
            "first_cell_x", "z2_neg_valid", "z2_zero_inf", "z2_zero_nan", "sentinel", "none_valid", "one_column_valid"}
    assert both | {"below_half", "tiny_z2", "x1_fraction"} <= seen[0], sorted((both | {"below_half", "tiny_z2"}) - seen[0])
    assert both | {"beyond_grid"} <= seen[2], sorted((both | {"beyond_grid"}) - seen[2])


def test_range_cases_are_ordinary_on_the_oracle(O, arith):
    """what IEEE arithmetic gives where the kernels' reciprocal is in doubt: with tz = 1.5e38 every pixel is valid, 1 / z2 is subnormal
    and the Jacobian's first column is fx * iz * gx — non-zero wherever the gradient is"""
    case = VC.BY_NAME["range_tz_1p5e38"]
    L, i1, _, gx, _, pts = VC.level_inputs(O, case, 0)
    wp, ev = evaluated(O, case, arith, 0)
    assert ev["valid"].all() and (wp[:, 2] == np.float32(1.5e38)).all()
    assert (ev["iz"] > 0).all() and (ev["iz"] < np.float32(2.0 ** -126)).all()
    g = gx.reshape(-1)[ev["iy1"] * L.iw + ev["ix1"]]
    assert np.array_equal(ev["J"][:, 0] != 0, g != 0) and np.count_nonzero(g) > 1500
    assert np.abs(ev["J"][g != 0, 0]).min() > 2.0 ** -126        # normal-range numbers, not the noise of an underflow


def outputs_differ(ev, em):
    """a mutant's evaluation differs from the restatement's in something an implementation shows: the valid set, or on the valid rows
    r, J, the sample or the reference pixel"""
    if not np.array_equal(ev["valid"], em["valid"]):
        return True
    v = ev["valid"]
    return not (VR.same_bits(ev["J"][v], em["J"][v]) and VR.same_bits(ev["r"][v], em["r"][v]) and
                all(np.array_equal(ev[k][v], em[k][v]) for k in ("ix2", "iy2", "ix1", "iy1")))


def mutant_differs(O, case, arith, lvl, mut):
    L, i1, i2, gx, gy, pts = VC.level_inputs(O, case, lvl)
    _, ev = evaluated(O, case, arith, lvl)
    wm = VR.warp(pts, case.pose, L, ARITH[arith], mut=mut)
    return outputs_differ(ev, VR.evaluate(i1, i2, gx, gy, pts, wm, L, ARITH[arith], mut=mut))


# mutant: (the case that must notice it, the level, the arithmetic set or None for both)
KILLERS = {
    "gt0_to_ge0": ("eight_px_neg", 0, None),              # u == 0 on column 8 with v inside
    "lt_iw_to_le_iw": ("one_px_pos", 0, None),            # u == iw on column 47 with v inside
    "iw_is_gw": ("flip_z_shift", 2, None),                # 46 x 35, level 2: u in [11, 12) is inside the image, outside the grid
    "iw_is_ih": ("half_px_pos", 0, None),                 # u in [36, 48) is valid in a 48 x 36 image
    "round_half_even": ("half_px_neg", 0, None),          # 0.5 -> 1, 2.5 -> 3: to even gives 0, 2
    "floor_of_f32_sum": ("below_half", 0, None),          # 0.49999997 + 0.5 rounds to 1.0 in float32
    "no_upper_clamp": ("half_px_pos", 0, None),           # 47.5 rounds to 48 = iw
    "clamp_to_gw": ("two_px_pos", 2, None),               # 10.5 rounds to 11: an image column, not a grid column
    "iz_lt0_to_le0": ("table_minus_inf", 0, "legacy"),    # 1 / -inf = -0 is kept by `< 0`; see the case
    "iz_abs": ("tz_-8", 0, None),                         # z2 < 0 and valid: iz is 0, not |1 / z2|
    "sentinel_w_ignored": ("half_px_blocks", 0, None),    # a zero-depth row given w = 1 picks the translation up and lands inside
    "x1y1_rounded": ("table_fraction", 0, None),          # (3.75, 2.5) reads pixel (3, 2)
    "u_times_w_dropped": ("flip_z", 0, None),             # a sentinel row lands on (2 cx, 2 cy), inside, before u *= w
}
# z2_ne0_removed is EQUIVALENT — proof.  Let z2 == +-0.  u is formed as ((o0 * fx) / z2 + cx) * w in IEEE float32.  A quotient by zero is
# +-infinity (numerator non-zero or infinite) or NaN (numerator zero or NaN); adding the finite cx to either leaves it infinite or NaN;
# multiplying by w leaves it infinite or NaN (infinity * 0 = NaN).  NaN fails `u > 0`; -infinity fails `u > 0`; +infinity fails
# `u < cols`.  So the four bounds comparisons, which are evaluated first (:450), already reject every row with z2 == 0, for every
# float32 input whatsoever, and the fifth condition (:451) never decides.  test_the_equivalent_mutant below runs it over every case.
EQUIVALENT = ("z2_ne0_removed",)


def test_mutant_table_is_complete():
    assert set(KILLERS) | set(EQUIVALENT) == set(VR.MUTANTS) and not set(KILLERS) & set(EQUIVALENT)


@pytest.mark.parametrize("mut", sorted(KILLERS))
def test_mutant_is_killed_by_its_named_case(O, arith, mut):
    name, lvl, only = KILLERS[mut]
    if only is not None and only != arith:
        assert not mutant_differs(O, VC.BY_NAME[name], arith, lvl, mut)   # (recorded: the other set cannot see it)
        return
    assert mutant_differs(O, VC.BY_NAME[name], arith, lvl, mut), (mut, name, lvl)


def test_the_equivalent_mutant(O, arith):
    """z2 != 0 removed changes nothing on any case, the z2 == 0 classes included (the proof stands above)"""
    zeros = 0
    for case in VC.CASES:
        for lvl in VC.levels_of(case):
            wp, _ = evaluated(O, case, arith, lvl)
            zeros += int(np.count_nonzero(wp[:, 2] == 0))
            assert not mutant_differs(O, case, arith, lvl, "z2_ne0_removed"), (case.name, lvl)
    assert zeros > 1000


def test_refusal_rule_is_the_header_s(O, arith):
    """the bounds the cases are built around are include/uwt.h's, and tests/seeded_ref.py refuses a seed exactly beyond them"""
    import os
    import re
    import seeded_ref as SR
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwt.h")).read()
    val = {k: float.fromhex(re.search(r"#define %s (0x1p-?\d+)" % k, hdr).group(1)) for k in ("UWT_TRANSLATION_MAX", "UWT_DEPTH_MAX", "UWT_DEPTH_MIN")}
    assert (val["UWT_TRANSLATION_MAX"], val["UWT_DEPTH_MAX"], val["UWT_DEPTH_MIN"]) == (VC.TRANSLATION_MAX, VC.DEPTH_MAX, VC.DEPTH_MIN)
    assert float(SR.TRANSLATION_MAX) == VC.TRANSLATION_MAX
    want = {"tz_2p125": None, "tz_m2p125": None, "tz_2p125_next": "seed", "tz_2p126": "seed", "tz_1p5e38": "seed", "tz_m1p5e38": "seed",
            "ds_lo_in": None, "ds_lo_out": "create", "ds_2p-137": "create", "ds_2p-140": "create", "ds_hi_in": None, "ds_hi_out": "create",
            "zero_num_lo_in": None, "zero_num_2p-137": "create", "zero_num_2p-140": "create"}
    assert {c.range_tag: VC.refusal(c) for c in VC.RANGE} == want
    assert all(VC.refusal(c) is None for c in VC.NORMAL)
    for case in VC.RANGE:
        if VC.refusal(case) == "create":
            continue
        ref, tgt, dep = VC.frames_of(case)
        st, pose, tr = SR.align(O, VC.oracle_params(O, case), ref, tgt, dep, seed=case.pose, keep=True)
        if VC.refusal(case) == "seed":
            assert (st, tr) == (SR.ERR_INVALID_ARG, []) and np.array_equal(pose, SR.IDENTITY)
        else:
            assert st != SR.ERR_INVALID_ARG and len(tr) >= 1
