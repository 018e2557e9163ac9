"""Designed inputs for the warp and validity stage.  A helper of the tests, not a test.

The geometry is chosen so that the warp is exact arithmetic in both arithmetic sets and the test, not chance, decides where a pixel
lands: the rotation is the identity or a flip by 180 degrees (a diagonal matrix of +-1), fx and fy are powers of two, cx and cy are
dyadic, depth_scale is 2^-12 and every depth code is a power of two, so every depth is a power of two and

    u = cx + fx (R00 (col - cx) / fx z + tx) / (R22 z + tz)        — for the identity and tz = 0:   u = col + fx tx / z.

Level l has fx / 2^l and cx_l = (cx + 0.5) / 2^l - 0.5 (dyadic again), and a depth plane made of 4 x 4 blocks of one code each keeps
whole blocks through the pyramid's 2 x 2 means (a partial cell of an odd size averages equal codes), so the same holds on levels 1, 2.

A Case names its size, intrinsics, depth plane, depth_scale and pose, says in `why` which classes it is there for, and DECLARES in
`reach` the classes it must reach on the levels it names; tests/test_validity_cpu.py holds it to that.  Classes (classify()):

    u_eq_0, u_eq_iw, v_eq_0, v_eq_ih   a coordinate exactly on a bound of the test 0 < u < iw, 0 < v < ih (the row is invalid)
    clamp_x, clamp_y                   valid with u >= iw - 0.5 (v >= ih - 0.5): the sample index is clamped from iw to iw - 1
    tie_x, tie_y                       valid with a fraction of exactly .5
    lt_half_x, lt_half_y               valid with 0 < u < 0.5: rounds to column 0
    below_half                         valid with u == 0.5 - 2^-25, the float32 below one half (u + 0.5 rounds to 1 in float32)
    beyond_grid                        valid and sampled in an image column >= the point grid's width (46 x 35, level 2: 12 > 11)
    last_cell_x, first_cell_x          valid with u in [iw - 1, iw) / (0, 1): the bilinear sampler's clamped "+ 1" and its first cell
    z2_neg_valid                       valid with z2 < 0: 1 / z2 is clamped to 0
    z2_zero_inf, z2_zero_nan           z2 == 0 with an infinite / a NaN quotient
    tiny_z2                            valid with 0 < z2 <= 2^-20
    sentinel                           rows with w = 0 (a depth code that is 0 or negative as a short)
    none_valid, one_column_valid       no valid row / every valid row lies in one grid column
    x1_fraction                        valid table rows whose reference position has a fraction >= .5 (truncation != rounding)
    z2_inf                             valid with an infinite z2 (1 / z2 is a signed zero)
    zero_numerators                    valid at the principal point: X = Y = 0, both numerators exact zeros, u = cx and v = cy whatever z2

`tags`: "exact" — u, v, z2 are checked against rational arithmetic; "range" — operands at or beyond the ends of the dense warp's domain
(include/uwt.h "the dense warp's division": 2^-126 <= |z2| <= 2^126), each with a tag of its own in `range_tag` so that results are
reported apart; refusal() says which of them the library refuses and where, the others lie just inside a bound and must agree bit for
bit; "table" — explicit rows instead of a dense grid; "cpu_only" — not given to the device (include/uwt.h does not define the result)."""
from collections import namedtuple

import numpy as np

f32 = np.float32
N_LEVELS = 3
SIZES = {"48x36": (48, 36),      # rows of whole groups of four on all three levels
         "46x35": (46, 35),      # ragged on all three; level 2: image 12 x 9, grid 11 x 8
         "48x4": (48, 4)}        # level 2 is a single row
INTRINSICS = {"A": (32.0, 32.0, 24.0, 18.0),     # fx == fy; levels 1, 2: cx 11.75 / 5.625, cy 8.75 / 4.125
              "B": (32.0, 16.0, 23.0, 17.5),     # fx != fy, integer cx: X == 0 on column 23; level 2: cx 5.375, cy 4.0
              "C": (32.0, 32.0, 0.0, 0.0),       # the principal point on pixel (0, 0): u is the quotient itself on level 0
              "R": (32.0, 32.0, 24.0, 1.5)}      # for 48 x 4: cy 1.5 / 0.5 / 0.0
DEPTH_SCALE = 2.0 ** -12
TRANSLATION_MAX, DEPTH_MAX, DEPTH_MIN = 2.0 ** 125, 2.0 ** 100, 2.0 ** -100   # include/uwt.h: UWT_TRANSLATION_MAX, UWT_DEPTH_MAX, UWT_DEPTH_MIN
IDENT, FLIP_X, FLIP_Y, FLIP_Z = (0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)   # qx qy qz qw

Case = namedtuple("Case", "name size intr depth depth_scale pose tags range_tag reach why table")


def image(w, h, k):
    """frame k of a size: a fixed integer texture with non-zero gradients nearly everywhere (the geometry never reads it)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return ((x * (37 + 6 * k) + y * (91 - 10 * k) + (x * y) * (13 + k) + ((x * x) >> 2) + ((y * y * y) >> 3) * (k + 1)) % 251).astype(np.uint8)


def depth_plane(kind, w, h):
    if kind is None:
        return None
    y, x = np.mgrid[0:h, 0:w]
    bx, by = x // 4, y // 4
    if kind == "blocks":       # z = 0.5, 1, 2, 4 on level 0 (0.125 .. 1 on level 2) in 4 x 4 blocks, with blocks of zeros cut in
        d = 2048 << ((bx + by) % 4)
        return np.where((bx + 2 * by) % 7 == 3, 0, d).astype(np.uint16)
    if kind == "sentinel":     # codes >= 32768 (negative through at<short>) and zeros only: every row is the w = 0 sentinel
        return np.where((bx + by) % 2 == 0, 0, 32768 + 4096 * ((bx + by) % 4)).astype(np.uint16)
    raise KeyError(kind)


def pose(q, tx=0.0, ty=0.0, tz=0.0):
    return np.array(list(q) + [tx, ty, tz], f32)


def shift(intr, kx, ky, q=IDENT, tz=0.0):
    """a translation of kx / 4 level-0 pixels in x and ky / 4 in y at depth 1 (tx = kx * 0.25 / fx: a dyadic number)"""
    fx, fy = INTRINSICS[intr][:2]
    return pose(q, kx * 0.25 / fx, ky * 0.25 / fy, tz)


def _dense(name, size, intr, depth, p, reach, why, tags=("exact",), range_tag=None, depth_scale=DEPTH_SCALE):
    return Case(name, size, intr, depth, depth_scale, np.asarray(p, f32), tuple(tags), range_tag, reach, why, None)


def _cases():
    c = []
    # ---- half-pixel shifts of either sign -------------------------------------------------------------------------------------------
    # z = 1 everywhere, u = col + kx / 4 on level 0, + kx / 8 on level 1, + kx / 16 on level 2
    c.append(_dense("half_px_pos", "48x36", "A", None, shift("A", 2, 2),
                    {0: ("tie_x", "tie_y", "clamp_x", "clamp_y", "last_cell_x", "first_cell_x"), 2: ("lt_half_x", "lt_half_y", "last_cell_x")},
                    "u = col + 0.5 on level 0: every pixel a tie, column 47 -> 47.5 rounds to 48 and is clamped; + 0.125 on level 2"))
    c.append(_dense("half_px_neg", "46x35", "B", None, shift("B", -2, -2),
                    {0: ("tie_x", "tie_y", "first_cell_x"), 2: ("first_cell_x",)},
                    "u = col - 0.5: column 0 leaves, column 1 is the tie 0.5 -> 1 (half AWAY from zero; to even would give 0)"))
    c.append(_dense("quarter_px_pos", "46x35", "B", None, shift("B", 1, 1),
                    {0: ("lt_half_x", "lt_half_y", "first_cell_x", "last_cell_x"), 2: ("lt_half_x",)},
                    "u = col + 0.25: column 0 lands in (0, 0.5) and samples column 0"))
    c.append(_dense("two_px_pos", "46x35", "B", None, shift("B", 8, 8),
                    {0: ("u_eq_iw", "v_eq_ih"), 1: ("u_eq_iw",), 2: ("tie_x", "tie_y", "beyond_grid")},
                    "+ 2 / 1 / 0.5 columns and rows; level 2 (image 12 x 9, grid 11 x 8): column 10 -> 10.5 samples image column 11, which the "
                    "grid does not have"))
    c.append(_dense("eight_px_neg", "48x36", "A", None, shift("A", -32, -32),
                    {0: ("u_eq_0", "v_eq_0"), 1: ("u_eq_0", "v_eq_0"), 2: ("u_eq_0", "v_eq_0")},
                    "u = col - 8 / - 4 / - 2: column 8 / 4 / 2 lands on u == 0 exactly, and likewise the rows"))
    c.append(_dense("one_px_pos", "48x36", "A", None, shift("A", 4, 0),
                    {0: ("u_eq_iw",), 2: ("first_cell_x",)},
                    "u = col + 1: column 47 lands on u == iw exactly while v stays inside"))
    c.append(_dense("one_row_pos", "48x36", "B", None, shift("B", 0, 4),
                    {0: ("v_eq_ih",)},
                    "v = row + 1: row 35 lands on v == ih exactly while u stays inside"))
    c.append(_dense("whole_width", "48x36", "A", None, shift("A", 4 * 48, 0),
                    {0: ("u_eq_iw", "none_valid"), 1: ("u_eq_iw", "none_valid"), 2: ("u_eq_iw", "none_valid")},
                    "u = col + 48 / 24 / 12 = col + iw: column 0 on the bound, nothing valid on any level"))
    c.append(_dense("width_less_quarter", "48x36", "A", None, shift("A", 4 * 48 - 1, 0),
                    {0: ("one_column_valid", "clamp_x"), 1: ("one_column_valid", "clamp_x"), 2: ("one_column_valid", "clamp_x")},
                    "one step short of the whole width: u = col + iw - 1/4 (1/8, 1/16): column 0 alone is valid (but for row 0, where v == 0), and clamped"))
    c.append(_dense("whole_height", "46x35", "B", None, shift("B", 0, 4 * 35),
                    {0: ("v_eq_ih", "none_valid")},
                    "v = row + 35 = row + ih on level 0"))
    c.append(_dense("whole_height_levels", "48x36", "A", None, shift("A", 0, 4 * 36),
                    {0: ("v_eq_ih", "none_valid"), 1: ("v_eq_ih", "none_valid"), 2: ("v_eq_ih", "none_valid")},
                    "v = row + 36 / 18 / 9 = row + ih on every level"))
    c.append(_dense("half_px_blocks", "48x36", "B", "blocks", shift("B", 2, 2),
                    {0: ("tie_x", "tie_y", "sentinel", "clamp_x", "u_eq_iw"), 2: ("tie_x", "sentinel", "u_eq_iw")},
                    "u = col + 0.5 / z with z = 0.5, 1, 2, 4: shifts of 1, 0.5, 0.25, 0.125 side by side; the zero blocks are sentinel rows, "
                    "which a product that gave them w = 1 would move into the image"))
    c.append(_dense("half_px_blocks_ragged", "46x35", "A", "blocks", shift("A", -2, 2),
                    {0: ("tie_x", "tie_y", "sentinel", "u_eq_0"), 1: ("sentinel",), 2: ("tie_x", "sentinel")},
                    "the same on ragged rows, the other sign"))
    c.append(_dense("sentinel_plane", "48x36", "A", "sentinel", shift("A", 2, 2),
                    {0: ("sentinel", "none_valid"), 1: ("sentinel", "none_valid"), 2: ("sentinel", "none_valid")},
                    "every depth code is 0 or >= 32768: every row is (0, 0, 1, 0), warps to u = v = 0 and is invalid"))
    # ---- tz: z2 = z + tz --------------------------------------------------------------------------------------------------------------
    # level 0 has z = 0.5, 1, 2, 4; level 1 half of that; level 2 a quarter: 0.125, 0.25, 0.5, 1
    for k, tz in enumerate((-0.5, -1.0, -2.0, -4.0)):
        lv = {0: ("z2_zero_inf", "z2_zero_nan", "sentinel") + (("z2_neg_valid",) if k else ())}
        if tz >= -1.0:
            lv[2] = ("z2_zero_inf", "z2_neg_valid", "sentinel")
        c.append(_dense("tz_%g" % tz, "48x36", "B", "blocks", pose(IDENT, 0, 0, tz), lv,
                        "z2 == 0 exactly on the blocks of z = %g: +-inf off column 23 and off row 17.5, 0 / 0 = NaN in u on column 23 (cx); "
                        "shallower blocks have z2 < 0 and land inside (u = cx + (col - cx) z / z2)" % -tz, tags=()))
    c.append(_dense("tz_-1_ragged", "46x35", "A", "blocks", pose(IDENT, 0, 0, -1.0),
                    {0: ("z2_zero_inf", "z2_zero_nan", "z2_neg_valid", "sentinel"), 2: ("z2_zero_inf", "z2_neg_valid")},
                    "the same on ragged rows, cx = 24 the integer column", tags=()))
    c.append(_dense("tz_-8", "48x36", "A", "blocks", pose(IDENT, 0, 0, -8.0),
                    {0: ("z2_neg_valid",), 1: ("z2_neg_valid",), 2: ("z2_neg_valid",)},
                    "tz below every depth: z2 = -7.5 .. -4, every pixel mirrored about (cx, cy), inside, and 1 / z2 < 0 -> 0", tags=()))
    c.append(_dense("tz_-1_plus_ulp", "48x36", "B", "blocks", pose(IDENT, 0, 0, -1.0 + 2.0 ** -24),
                    {0: ("z2_neg_valid",), 2: ("z2_neg_valid",)},
                    "z = 1 gives z2 = 2^-24: quotients of 2^24 (col - 23) and 2^24 (row - 17.5), all far outside; z = 0.5 gives -0.5 + 2^-24", tags=()))
    c.append(_dense("tz_-2_plus_ulp", "48x36", "A", "blocks", pose(IDENT, 0, 0, -2.0 + 2.0 ** -23),
                    {0: ("tiny_z2", "z2_neg_valid")},
                    "z = 2 gives z2 = 2^-23; pixel (24, 18) = (cx, cy) lies in such a block: X = Y = 0, u = cx, v = cy, valid with 1 / z2 = 2^23 "
                    "and a Jacobian row of gradient x 2^28", tags=()))
    # ---- flips ------------------------------------------------------------------------------------------------------------------------
    c.append(_dense("flip_x", "48x36", "A", "blocks", pose(FLIP_X),
                    {0: ("z2_neg_valid", "sentinel"), 2: ("z2_neg_valid",)},
                    "R = diag(1, -1, -1): z2 = -z, u = 2 cx - col, v = row: behind the camera and inside"))
    c.append(_dense("flip_x_back", "48x36", "A", "blocks", pose(FLIP_X, 0, 0, 8.0),
                    {0: ("sentinel",), 2: ("sentinel",)},
                    "the same brought back in front: z2 = 8 - z", tags=()))
    c.append(_dense("flip_y", "46x35", "B", "blocks", pose(FLIP_Y),
                    {0: ("z2_neg_valid", "sentinel"), 2: ("z2_neg_valid",)},
                    "R = diag(-1, 1, -1): z2 = -z, u = col, v = 2 cy - row"))
    c.append(_dense("flip_y_back", "46x35", "B", "blocks", pose(FLIP_Y, 0, 0, 8.0),
                    {0: ("sentinel",)}, "z2 = 8 - z", tags=()))
    c.append(_dense("flip_z", "48x36", "B", "blocks", pose(FLIP_Z),
                    {0: ("sentinel", "u_eq_0", "v_eq_0"), 2: ("sentinel",)},
                    "R = diag(-1, -1, 1): z2 = z, u = 2 cx - col = 46 - col, v = 35 - row.  A sentinel row (w = 0) warps to (2 cx, 2 cy) = "
                    "(46, 35), inside the image, BEFORE u *= w makes it 0"))
    c.append(_dense("flip_z_shift", "46x35", "A", None, shift("A", 2, 2, FLIP_Z),
                    {0: ("tie_x", "tie_y", "clamp_x", "clamp_y"), 2: ("beyond_grid", "last_cell_x")},
                    "u = 48.5 - col, v = 36.5 - row on level 0 (ties; column 3 -> 45.5 rounds to 46 = iw and is clamped); on level 2 "
                    "u = 11.375 - col: column 0 lands in image column 11, beyond the 11-wide grid, in the bilinear sampler's last cell"))
    # ---- the principal point on pixel (0, 0) ------------------------------------------------------------------------------------------
    below = float(f32(0.5) - f32(2.0 ** -25))
    c.append(_dense("below_half", "48x36", "C", None, pose(IDENT, below / 32.0, below / 32.0, 0),
                    {0: ("below_half", "lt_half_x", "lt_half_y")},
                    "cx = cy = 0, tx = (0.5 - 2^-25) / 32: column 0 has u = 0.49999997, which rounds to 0 but u + 0.5 rounds to 1.0 in float32",
                    tags=()))
    # ---- a single-row level -----------------------------------------------------------------------------------------------------------
    c.append(_dense("single_row", "48x4", "R", None, shift("R", 2, 2),
                    {0: ("tie_x", "tie_y", "clamp_y"), 2: ("lt_half_x", "lt_half_y")},
                    "48 x 4: level 2 is 12 x 1 with cy = 0: v = 0.125 on its only row"))
    # ---- range cases: operands or quotients at and beyond the ends of the dense warp's domain (include/uwt.h "the dense warp's division") ----
    # z = 1: z2 = 1 + tz = tz, every u = cx exactly; 1 / z2 is 2^-125 (normal), 2^-126 (the smallest normal) or subnormal.  Inside
    # |tz| <= TRANSLATION_MAX the device must agree bit for bit; beyond it a seed is refused
    up = float(np.nextafter(f32(TRANSLATION_MAX), f32(np.inf)))
    for tag, tz in (("tz_2p125", 2.0 ** 125), ("tz_m2p125", -2.0 ** 125), ("tz_2p125_next", up), ("tz_2p126", 2.0 ** 126), ("tz_1p5e38", 1.5e38),
                    ("tz_m1p5e38", -1.5e38)):
        c.append(_dense("range_" + tag, "48x36", "A", None, pose(IDENT, 0, 0, tz), {0: ("z2_neg_valid",) if tz < 0 else ()},
                        "z2 = tz: every pixel valid at u = cx, v = cy", tags=("range",), range_tag=tag))
    # identity pose, z2 = z = code * depth_scale / 2^lvl; column 23 (cx) has the zero numerator.  Inside the two depth bounds the device
    # must agree; outside uwt_create refuses the context
    lo, hi = 2.0 ** -98, f32(DEPTH_MAX / 32767.0)
    while float(hi) * 32767.0 > DEPTH_MAX:              # the largest float32 whose level-0 depth is inside, tested in double as uwt_create does
        hi = np.nextafter(hi, f32(0))
    hi = float(hi)
    assert hi * 32767.0 <= DEPTH_MAX < float(np.nextafter(f32(hi), f32(np.inf))) * 32767.0 and lo / 4 == DEPTH_MIN
    for tag, ds in (("ds_lo_in", lo), ("ds_lo_out", float(np.nextafter(f32(lo), f32(0)))), ("ds_2p-137", 2.0 ** -137), ("ds_2p-140", 2.0 ** -140),
                    ("ds_hi_in", hi), ("ds_hi_out", float(np.nextafter(f32(hi), f32(np.inf))))):
        c.append(_dense("range_" + tag, "48x36", "B", "blocks", pose(IDENT), {0: ("sentinel", "u_eq_0")},
                        "depth_scale = %r: depths of %.3g .. %.3g over the three levels (2^-137: 2^-126 on level 0, subnormal below; 2^-140: "
                        "every depth subnormal)" % (ds, 2048 * ds / 4, 16384 * ds), tags=("range",), range_tag=tag, depth_scale=ds))
    # the zero numerator on its own: intrinsics A put the principal point on pixel (24, 18) of level 0, in a block of code 8192; 0 / z2 is an
    # exact zero for every z2 that is not zero, a subnormal one included — where the hardware reciprocal of a subnormal is infinite
    for tag, ds in (("zero_num_lo_in", lo), ("zero_num_2p-137", 2.0 ** -137), ("zero_num_2p-140", 2.0 ** -140)):
        c.append(_dense("range_" + tag, "48x36", "A", "blocks", pose(IDENT), {0: ("zero_numerators", "sentinel")},
                        "depth_scale = %r: pixel (24, 18) has z2 = %.3g and X = Y = 0" % (ds, 8192 * ds), tags=("range",), range_tag=tag, depth_scale=ds))
    return c


def _table_cases():
    """explicit rows on level 0 of 48 x 36, intrinsics A"""
    c = []
    rows = [(x + fx_, y + fy_, z, 1.0) for x in (3, 17, 40) for y in (2, 20, 33) for fx_, fy_ in ((0.75, 0.5), (0.5, 0.75), (0.25, 0.25))
            for z in (0.5, 2.0)]
    c.append(Case("table_fraction", "48x36", "A", None, DEPTH_SCALE, shift("A", 1, 1), ("exact", "table"), None, {0: ("x1_fraction",)},
                  "reference positions with fractions: Mat::at truncates (3.75 -> 3), rounding would read the next pixel", np.array(rows, f32)))
    big = -3.0e38
    rows = [(x, y, big, 1.0) for y in range(2, 34) for x in range(2, 46)]
    c.append(Case("table_minus_inf", "48x36", "A", None, DEPTH_SCALE, pose(IDENT, 0, 0, big), ("table", "range", "cpu_only"), "z2_inf",
                  {0: ("z2_inf",)},
                  "z2 = -3e38 - 3e38 = -inf: u = cx exactly, 1 / z2 = -0, which `< 0` keeps and `<= 0` replaces by +0 — the sign of a zero in "
                  "J (legacy set: fma(g1, 0, g0 * -0))", np.array(rows, f32)))
    return c


CASES = _cases() + _table_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DENSE = [c for c in CASES if c.table is None]
DEVICE = [c for c in CASES if "cpu_only" not in c.tags]
NORMAL = [c for c in DEVICE if "range" not in c.tags]           # inside the normal range: the device must agree bit for bit
RANGE = [c for c in DEVICE if "range" in c.tags]


def refusal(case):
    """where the library refuses a case (include/uwt.h "the dense warp's division"): "create" — uwt_create, for its depth_scale; "seed" — the
    pair of a seeded call, for its translation; None — inside the domain"""
    ds = abs(float(f32(case.depth_scale)))
    if case.depth is not None and ds != 0 and (ds * 32767.0 > DEPTH_MAX or ds / 2 ** (N_LEVELS - 1) < DEPTH_MIN):
        return "create"
    if (np.abs(case.pose[4:]) > f32(TRANSLATION_MAX)).any():
        return "seed"
    return None


def levels_of(case):
    return (0,) if case.table is not None else tuple(range(N_LEVELS))


def params_over(case, **more):
    """parameter fields of a case (for oracle.default_params and capi.default_params alike)"""
    d = dict(n_levels=N_LEVELS, first_level=N_LEVELS - 1, last_level=0, max_iters=1, early_exit=0, has_depth=int(case.depth is not None),
             depth_scale=case.depth_scale)
    d.update(more)
    return d


def frames_of(case):
    """(reference frame, target frame, depth plane or None) of a case's size and depth kind"""
    w, h = SIZES[case.size]
    return image(w, h, 0), image(w, h, 1), depth_plane(case.depth, w, h)


def classify(wp, ev, L, pts):
    """{class: count} of one level's warp `wp`, evaluation `ev` (tests/validity_ref.py) and table `pts`"""
    iw, ih, gw = int(L.iw), int(L.ih), int(L.w)
    u, v, z2, w = (wp[:, k] for k in range(4))
    ok = ev["valid"]
    with np.errstate(all="ignore"):
        fu, fv = u - np.floor(u), v - np.floor(v)
        out = dict(
            u_eq_0=(u == 0) & (w != 0), u_eq_iw=u == iw, v_eq_0=(v == 0) & (w != 0), v_eq_ih=v == ih,
            clamp_x=ok & (u >= iw - 0.5), clamp_y=ok & (v >= ih - 0.5),
            tie_x=ok & (fu == 0.5), tie_y=ok & (fv == 0.5),
            lt_half_x=ok & (u < 0.5), lt_half_y=ok & (v < 0.5),
            below_half=ok & (u == f32(0.5) - f32(2.0 ** -25)),
            beyond_grid=ok & (ev["ix2"] >= gw),
            last_cell_x=ok & (u >= iw - 1), first_cell_x=ok & (u < 1),
            z2_neg_valid=ok & (z2 < 0),
            z2_zero_inf=(z2 == 0) & (np.isinf(u) | np.isinf(v)), z2_zero_nan=(z2 == 0) & (np.isnan(u) | np.isnan(v)) & (w != 0),
            tiny_z2=ok & (z2 > 0) & (z2 <= 2.0 ** -20),
            sentinel=w == 0,
            x1_fraction=ok & ((pts[:, 0] - np.floor(pts[:, 0]) >= 0.5) | (pts[:, 1] - np.floor(pts[:, 1]) >= 0.5)),
            z2_inf=ok & np.isinf(z2),
            zero_numerators=ok & (pts[:, 0] == f32(L.cx)) & (pts[:, 1] == f32(L.cy)) & (u == f32(L.cx)) & (v == f32(L.cy)))
    out = {k: int(np.count_nonzero(m)) for k, m in out.items()}
    out["none_valid"] = int(not ok.any())
    cols = np.unique(np.nonzero(ok)[0] % gw) if pts.shape[0] == gw * int(L.h) else np.zeros(0)
    out["one_column_valid"] = int(ok.any() and cols.size == 1)
    return out


_inputs = {}


def oracle_params(O, case, **more):
    w, h = SIZES[case.size]
    return O.default_params(w, h, *INTRINSICS[case.intr], **params_over(case, **more))


def level_inputs(O, case, lvl):
    """(L, reference image, target image, gx, gy, table) of a case on one level, by the oracle's pyramid, gradient and point stages;
    made once (none of it depends on the arithmetic set)"""
    key = (case.name, lvl)
    if key not in _inputs:
        p = oracle_params(O, case)
        ref, tgt, dep = frames_of(case)
        a, b = O.pyramid(ref, N_LEVELS)[lvl], O.pyramid(tgt, N_LEVELS)[lvl]
        L = O.level_intrinsics(p, lvl)
        gx, gy = O.scharr3(a)
        if case.table is not None:
            pts = case.table
        else:
            pts = O.dense_points(O.pyramid(dep, N_LEVELS)[lvl] if dep is not None else None, L.w, L.h, lvl, p.depth_scale)
        _inputs[key] = (L, a, b, gx, gy, pts)
    return _inputs[key]
