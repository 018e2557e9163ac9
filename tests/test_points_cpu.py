"""The designed cases of the sparse point producers (tests/points_cases.py) on the CPU: the numpy restatement (tests/points_ref.py) equals
the oracle bit for bit on every case, every case reaches the classes it declares, the classes the issue names occur in the catalogue, and
every deliberate mistake of points_ref.MUTANTS is noticed by a NAMED case (the table is printed: pytest -s).  tests/test_gpu_points.py
gives every named case to the device, which then cannot pass with that mistake in a kernel.  No GPU."""
import math

import numpy as np
import pytest

import points_cases as PC
import points_ref as PR

ARITH_INDEPENDENT = True   # integer magnitudes, one float64 comparison, float32 products of exact operands: no arithmetic set involved

W0, H0 = 64, 48            # the level 0 of the key-point sets and the point tables
PATCHES = PC.patch_sets(W0, H0)
PATCH_BY_NAME = {p.name: p for p in PATCHES}
TABLE_LEVELS = ((64, 48), (16, 12))
TABLES = {wh: PC.table_sets(*wh) for wh in TABLE_LEVELS}


def kp_depth():
    return PC.depths_of("g64x48")[0]


# ---- the restatement is the oracle ------------------------------------------------------------------------------------------------------
def test_magnitude_equals_oracle_and_reaches_its_classes(O):
    """on every frame of every geometry, every level; and level 0 of every geometry reaches all eight classes of the magnitude step"""
    for geom, (w, h, nl, slots, _) in PC.GEOMS.items():
        for s in range(slots):
            for l, img in enumerate(O.pyramid(PC.frames_of(geom)[s], nl)):
                gx, gy = O.scharr3(img)
                assert PR.gradient_magnitude(gx, gy).tobytes() == O.gradient_mag(gx, gy).tobytes(), (geom, s, l)
                if l == 0:
                    got = PC.magnitude_classes(gx, gy)
                    assert all(got[k] > 0 for k in PC.MAGNITUDE_CLASSES), (geom, s, got)
    # the two saturation classes give the values the issue states: 127.5 -> 128 and 255
    gx = np.array([3000, -256, 300, 252, 258, 288], np.int16)
    gy = np.array([0, 0, -300, 0, 18, -36], np.int16)
    assert PR.gradient_magnitude(gx, gy).tolist() == [128, 128, 255, 126, 136, 146] == O.gradient_mag(gx, gy).tolist()   # 136.5, 145.5


@pytest.mark.parametrize("case", PC.CANDIDATES, ids=lambda c: c.name)
def test_candidates_equal_oracle_and_reach_their_classes(O, case):
    frames, t = PC.candidate_inputs(O, case)
    assert t is not None and math.isfinite(t)
    for mag, dep, grid in frames:
        rows, n = PR.candidate_points(mag, dep, t, grid, case.lvl, case.n)
        want, nw = O.candidate_points(mag, dep, t, grid=grid)
        assert n == nw and PR.same_bits(rows, want), case.name
        again, _ = PR.candidate_points(mag, dep, t, grid, case.lvl, case.n)
        assert PR.same_bits(rows, again)                     # deterministic
    got, m = PC.candidate_classes(O, case)
    assert all(got[k] for k in case.reach), (case.name, {k: got[k] for k in case.reach})
    if case.kind in ("eq", "below", "above"):                # the magnitude the threshold sits on is in the pivot frame's grid
        mag, _, (gw, gh) = PC.level_planes(O, case.geom, case.pivot)[case.lvl]
        assert (mag[:gh, :gw] == m).any()


def test_the_classes_the_catalogue_must_hold(O):
    """not merely intended: the three equalities (on a power-of-two pixel count and on one whose mean is not dyadic), every cell selected,
    the empty last band, one band, m below, at and above 1024, two column blocks, the grid below the image with a mean it moves"""
    seen = {}
    for case in PC.CANDIDATES:
        got, _ = PC.candidate_classes(O, case)
        for k, v in got.items():
            if v:
                seen.setdefault(k, set()).add(case.name)
    need = ("thres_eq_m", "thres_below_m", "thres_above_m", "all_cells", "no_cell", "empty_last_band", "bands_1", "m_lt_1024", "m_eq_1024",
            "m_gt_1024_ragged", "two_column_blocks", "grid_lt_image", "pitch_gt_iw", "beyond_grid_moves_mean", "depth_zero_byte_on_selected",
            "depth_all_selected_on_zero", "depth_lo_zero_hi_not", "depth_hi_zero_lo_not", "depth_lo_ne_hi", "slots_from_1", "slots_from_2", "eight_frames")
    assert not [k for k in need if k not in seen]
    for eq in ("thres_eq_m", "thres_below_m", "thres_above_m"):
        assert any(n.startswith("g128x64_l0") for n in seen[eq]) and any(n.startswith("g46x35_l0") for n in seen[eq]), eq
    assert seen["dyadic_mean"] >= {"g128x64_l0_eq"} and seen["mean_not_dyadic"] >= {"g46x35_l0_eq"}
    # the counts themselves
    for name, cells in (("g128x64_l0_all", 128 * 64), ("g46x35_l2_all", 11 * 8), ("g40x90_l0_all", 40 * 90), ("g272x24_l0_all", 272 * 24)):
        case = PC.CAND_BY_NAME[name]
        (mag, dep, grid), = PC.candidate_inputs(O, case)[0]
        assert PR.candidate_points(mag, dep, PC.threshold_of(O, case), grid)[1] == cells == grid[0] * grid[1]
    assert PR.bands_of(40, 90, 1) == (11, 9) and 10 * 9 >= 90
    assert PR.bands_of(8, 6, 1)[0] == 1 and PR.bands_of(160, 96, 1)[0] * 160 == 1920 and PR.bands_of(128, 64, 1)[0] * 128 == 1024


@pytest.mark.parametrize("ps", PATCHES, ids=lambda p: p.name)
@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
def test_patch_points_equal_oracle_and_reach_their_classes(O, ps, depth):
    dep = kp_depth() if depth else None
    rows, n = PR.patch_points(ps.kp, dep, W0, H0)
    want, nw = O.patch_points(ps.kp, dep, W0, H0)
    assert n == nw and PR.same_bits(rows, want)
    assert PR.same_bits(rows, PR.patch_points(ps.kp, dep, W0, H0)[0])
    for cap in sorted({0, 1, max(n - 1, 0), n, n + 7}):       # below, at and above the full count
        r, nr = PR.patch_points(ps.kp, dep, W0, H0, cap=cap)
        w_, nw_ = O.patch_points(ps.kp, dep, W0, H0, cap=cap)
        assert nr == nw_ == n and PR.same_bits(r, w_) and len(r) == min(cap, n)
    got = PC.patch_classes(ps.kp, kp_depth(), W0, H0)
    assert all(got[k] for k in ps.reach), (ps.name, {k: got[k] for k in ps.reach})


def test_key_point_edge_values_and_depths(O):
    """every x and y of the issue's list occurs, each with each; the depth set lands on its five values, read at ((int)y, (int)x)"""
    kp = PATCH_BY_NAME["edges"].kp
    assert {float(v) for v in kp[:, 0]} == {0, 0.5, 4.5, 5, 5.5, W0 - 6, W0 - 5.5, W0 - 1, W0 - 0.5} and len(kp) == 81
    assert {float(v) for v in kp[:, 1]} == {0, 0.5, 4.5, 5, 5.5, H0 - 6, H0 - 5.5, H0 - 1, H0 - 0.5}
    d = kp_depth()
    on = PATCH_BY_NAME["on_depths"].kp
    assert [int(d[int(y), int(x)]) for x, y in on] == list(PC.KP_DEPTHS)
    rows, n = PR.patch_points(on, d, W0, H0)
    assert n == 4 * 121 and [float(z) for z in rows[::121, 2]] == [float(np.float32(v) * np.float32(0.0002)) for v in (1, 32767, -32768, -1)]
    for name, make in PC.REFUSED_KEYPOINTS.items():           # what the host refuses is outside the domain 0 <= x < w, 0 <= y < h
        bad = np.array(make(W0, H0), np.float32)
        assert not all(0 <= x < W0 and 0 <= y < H0 for x, y in bad), name
    for ps in PATCHES:
        assert all((x >= 0) and (x < W0) and (y >= 0) and (y < H0) for x, y in ps.kp), ps.name


@pytest.mark.parametrize("wh", TABLE_LEVELS, ids=lambda wh: "%dx%d" % wh)
def test_add_patch_points_equal_oracle_and_reach_their_classes(O, wh):
    w, h = wh
    for tb in TABLES[wh]:
        got = PC.table_classes(tb.pts, w, h)
        assert all(got[k] for k in tb.reach), (tb.name, got)
        for ps in tb.patch_sizes:
            rows, n = PR.add_patch_points(tb.pts, w, h, ps)
            want, nw = O.add_patch_points(tb.pts, w, h, patch_size=ps)
            assert n == nw and PR.same_bits(rows, want), (tb.name, ps)
            for cap in sorted({0, len(tb.pts) // 2, len(tb.pts), (len(tb.pts) + n) // 2, n, n + 3}):   # inside the clone, inside the cells
                r, nr = PR.add_patch_points(tb.pts, w, h, ps, cap=cap)
                w_, nw_ = O.add_patch_points(tb.pts, w, h, patch_size=ps, cap=cap)
                assert nr == nw_ == n and PR.same_bits(r, w_), (tb.name, ps, cap)


# ---- every mistake is noticed by a named case -------------------------------------------------------------------------------------------
def cand_differs(O, name, mut):
    case = PC.CAND_BY_NAME[name]
    frames, t = PC.candidate_inputs(O, case)
    for mag, dep, grid in frames:
        a = PR.candidate_points(mag, dep, t, grid, case.lvl, case.n)
        b = PR.candidate_points(mag, dep, t, grid, case.lvl, case.n, mut=mut)
        if a[1] != b[1] or not PR.same_bits(a[0], b[0]):
            return True
    return False


def mag_differs(O, name, mut):
    geom, slot = name
    gx, gy = O.scharr3(PC.frames_of(geom)[slot])
    return PR.gradient_magnitude(gx, gy).tobytes() != PR.gradient_magnitude(gx, gy, mut).tobytes()


def patch_differs(O, name, mut):
    name, depth, cap = name
    dep = kp_depth() if depth else None
    a = PR.patch_points(PATCH_BY_NAME[name].kp, dep, W0, H0, cap)
    b = PR.patch_points(PATCH_BY_NAME[name].kp, dep, W0, H0, cap, mut=mut)
    return a[1] != b[1] or not PR.same_bits(a[0], b[0])


def table_differs(O, name, mut):
    wh, name, ps, cap = name
    tb = {t.name: t for t in TABLES[wh]}[name]
    a = PR.add_patch_points(tb.pts, wh[0], wh[1], ps, cap)
    b = PR.add_patch_points(tb.pts, wh[0], wh[1], ps, cap, mut=mut)
    return a[1] != b[1] or not PR.same_bits(a[0], b[0])


# mutant: (which producer, the named case that must notice it)
KILLERS = {
    "ge_for_gt": (cand_differs, "g128x64_l0_eq"),                 # the cells holding m itself: m > m fails, m >= m holds
    "compare_f32": (cand_differs, "g128x64_l0_below"),            # the double below m rounds to m in float32
    "mean_over_pitch": (cand_differs, "g46x35_l0_eq"),            # 46 columns in rows of 48: the smaller mean lets the m cells in
    "mean_over_grid": (cand_differs, "g46x35_l2_below"),          # image 12 x 9 over a grid of 11 x 8, magnitudes in column 11 and row 8
    "half_up": (mag_differs, ("g64x48", 0)),                      # 255 + 18: 136.5 -> 136
    "saturate_after": (mag_differs, ("g64x48", 0)),               # 5760 beside 0: 128, not 255
    "depth_low_byte_of_pixel": (cand_differs, "g64x48_l0_all_slot1"),   # 0x0100: byte x is zero for even x, the low byte always
    "z_scaled_by_level": (cand_differs, "g64x48_l2_frac_slot3"),
    "y_major": (cand_differs, "g128x64_l0_eq"),
    "band_row_lost": (cand_differs, "g40x90_l0_all"),
    "band_row_doubled": (cand_differs, "g40x90_l0_all"),
    "i_ge_0": (patch_differs, ("edges", False, None)),
    "i_le_w": (patch_differs, ("edges", False, None)),
    "upper_lt": (patch_differs, ("edges", False, None)),
    "depth_unsigned": (patch_differs, ("on_depths", True, None)),
    "d_le_0_skips": (patch_differs, ("on_depths", True, None)),
    "kp_201_used": (patch_differs, ("n201", False, None)),
    "patch_y_outer": (patch_differs, ("asymmetric", False, None)),
    "rint_for_roundf": (table_differs, ((64, 48), "ties", 5, None)),
    "centre_kept": (table_differs, ((64, 48), "borders", 3, None)),
    "centre_by_unrounded": (table_differs, ((64, 48), "fractions", 5, None)),
    "count_clipped_at_cap": (table_differs, ((16, 12), "n257", 3, 300)),
}


def test_mutant_table_is_complete():
    assert set(KILLERS) == set(PR.MUTANTS)      # `floor` for the truncating cast is equivalent: the proof stands in points_ref.py


@pytest.mark.parametrize("mut", sorted(KILLERS))
def test_mutant_is_killed_by_its_named_case(O, mut):
    fn, name = KILLERS[mut]
    assert fn(O, name, mut), (mut, name)


def test_print_the_table_of_which_case_notices_which(O):
    """every candidate case against every candidate mutant, and the other producers' named cases: printed, and no mutant left unnoticed"""
    cand_muts = [m for m, (fn, _) in KILLERS.items() if fn is cand_differs]
    noticed = {m: [c.name for c in PC.CANDIDATES if cand_differs(O, c.name, m)] for m in cand_muts}
    for m, (fn, name) in KILLERS.items():
        if fn is not cand_differs:
            noticed[m] = [repr(name)] if fn(O, name, m) else []
    print()
    for m in sorted(noticed):
        print("%-24s %3d case(s): %s" % (m, len(noticed[m]), ", ".join(noticed[m][:6]) + (" ..." if len(noticed[m]) > 6 else "")))
    assert all(noticed[m] for m in noticed)
    for m in cand_muts:
        assert KILLERS[m][1] in noticed[m]


def test_the_truncating_cast_is_floor_under_i_gt_0():
    """the equivalent mutant, run as well as proved: floor for (int) changes no row of any key-point set or table"""
    import unittest.mock as mock
    with mock.patch.object(np, "trunc", np.floor):
        floored = [PR.patch_points(ps.kp, None, W0, H0) for ps in PATCHES]
        tabs = [PR.add_patch_points(tb.pts, 64, 48, ps) for tb in TABLES[(64, 48)] for ps in tb.patch_sizes]
    assert any((ps.kp[:, 0] - 5 < 0).any() and (ps.kp[:, 0] % 1 != 0).any() for ps in PATCHES)
    for ps, f in zip(PATCHES, floored):
        a = PR.patch_points(ps.kp, None, W0, H0)
        assert a[1] == f[1] and PR.same_bits(a[0], f[0])
    for (tb, ps), f in zip([(tb, ps) for tb in TABLES[(64, 48)] for ps in tb.patch_sizes], tabs):
        a = PR.add_patch_points(tb.pts, 64, 48, ps)
        assert a[1] == f[1] and PR.same_bits(a[0], f[0])
