"""The designed inputs of the sparse point producers: images, depth planes, thresholds, key points and point tables built so that every
decision the producers make is taken CLOSE — a magnitude equal to the threshold, a depth byte that is zero while its pixel is not, a
patch over every border, a coordinate on a rounding tie.  A helper of the tests, not a test.

The producers see an image only through Scharr, so the cases design images: a flat plane of 100 with isolated bumps of +-1..+-3, a block
of +120 (one gradient saturated beside a zero one along its sides, both saturated at its corners), a "ladder" — a step whose height
changes from row to row, which gives |g| = 252, 255 and 258 — short ramps, and a patch in the bottom right corner that puts magnitudes
into the image columns beyond the point grid of an odd-sized level.

Every case declares the classes it reaches (`reach`); tests/test_points_cpu.py verifies each declaration on the restatement
(tests/points_ref.py) and that every mistake of points_ref.MUTANTS is noticed by a named case.  tests/test_gpu_points.py gives the same
cases to the device."""
import math
from collections import namedtuple

import numpy as np

import points_ref as PR

F32 = np.float32

# name: (w, h, n_levels, slots, has_depth).  What each shape is the smallest for stands in the class list below.
GEOMS = {
    "g64x48": (64, 48, 4, 10, True),      # coarsest level 8 x 6: one row band; 1, 3 and 8 frames per call out of ten slots
    "g128x64": (128, 64, 2, 2, False),    # 8192 pixels, a power of two: a dyadic mean; gw * bands = 1024 exactly
    "g160x96": (160, 96, 2, 2, False),    # gw * bands = 1920: ragged over the scan's 1024 threads
    "g40x90": (40, 90, 1, 1, False),      # 11 bands of 9 rows: the last band is empty
    "g272x24": (272, 24, 2, 2, False),    # two column blocks
    "g163x99": (163, 99, 4, 3, True),     # levels 1 and 2: image 82 x 50 / 41 x 25 over grids 81 x 49 / 40 x 24; pitch 164, 84, 44
    "g46x35": (46, 35, 3, 2, False),      # 1610 pixels: the mean is no dyadic number; level 2: image 12 x 9 over a grid 11 x 8
}


def intr(w, h):
    return (0.82 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)


def plane(w, h, seed):
    """one designed image; `seed` moves the ladder and draws the bumps, so that no two slots hold the same frame"""
    rng = np.random.default_rng(1000 + seed)
    a = np.full((h, w), 100, np.int64)
    a[h // 8:h // 8 + max(4, h // 5), w // 8:w // 8 + max(5, w // 5)] += 120          # the block
    heights = [0, 5, 7, 0, 8, 6, 0, 2, 8, 0, 4, 7, 1, 3, 7, 1]                        # 3a + 10b + 3c = 84, 85, 86 among its triples
    x0 = w // 2 + 1 + seed % 3
    for k, hh in enumerate(heights):
        y = h // 3 + k
        if y < h - 2:
            a[y, x0:x0 + max(3, w // 6)] += hh                                        # the ladder
    y0 = h - h // 4
    a[y0:h - 1, 2:w // 2] += np.arange(w // 2 - 2)[None, :] % 7                       # short ramps
    a[h - 3:, w - 3:] += 60                                                           # beyond the grid of an odd-sized level
    for y in range(3, h - 3, 5):
        for x in range(3 + y % 3, w - 3, 6):
            near = a[y - 2:y + 3, x - 2:x + 3]
            if near.min() == 100 and near.max() == 100 and rng.random() < 0.6:
                a[y, x] += rng.choice([-3, -2, -1, 1, 2, 3])                          # isolated bumps
    return a.astype(np.uint8)


_frames = {}


def frames_of(geom):
    """the frames of a geometry's slots"""
    if geom not in _frames:
        w, h, _, slots, _ = GEOMS[geom]
        _frames[geom] = [plane(w, h, s) for s in range(slots)]
    return _frames[geom]


# depths a key point is put on: zero, the smallest, the largest positive short, the smallest and the largest negative short
KP_DEPTHS = (0, 1, 0x7FFF, 0x8000, 0xFFFF)
KP_DEPTH_AT = [(10 + 3 * k, 20) for k in range(len(KP_DEPTHS))]      # (x, y) of the pixel holding KP_DEPTHS[k] in slot 0's plane


def depth_plane(geom, slot):
    """Slot s of a geometry with depth.  at<uchar>(y, x) reads byte x of row y: pixel x / 2's low byte for even x, its high byte for odd x.
    slot % 4 == 0: 0x0100 + (pixel index % 200): low bytes mostly non-zero, high byte 1 — and the pixels of KP_DEPTHS in slot 0;
    slot % 4 == 1: 0x0100 everywhere: low byte 0, high byte 1 (even byte columns read zero);
    slot % 4 == 2: 0x0007 everywhere: low byte 7, high byte 0 (odd byte columns read zero);
    slot % 4 == 3: bytes drawn from {0, 0, 3, 250}: zero bytes under selected cells, scattered."""
    w, h, _, _, _ = GEOMS[geom]
    kind = slot % 4
    if kind == 0:
        d = (0x0100 + (np.arange(w * h).reshape(h, w) % 200)).astype(np.uint16)
        if slot == 0:
            for (x, y), v in zip(KP_DEPTH_AT, KP_DEPTHS):
                d[y, x] = v
        return d
    if kind == 1:
        return np.full((h, w), 0x0100, np.uint16)
    if kind == 2:
        return np.full((h, w), 0x0007, np.uint16)
    rng = np.random.default_rng(2000 + slot)
    b = rng.choice(np.array([0, 0, 3, 250], np.uint8), (h, 2 * w))
    return np.ascontiguousarray(b).view("<u2").reshape(h, w).astype(np.uint16)


_depths = {}


def depths_of(geom):
    if geom not in _depths:
        _, _, _, slots, has = GEOMS[geom]
        _depths[geom] = [depth_plane(geom, s) for s in range(slots)] if has else None
    return _depths[geom]


def oracle_params(O, geom, **over):
    w, h, nl, _, has = GEOMS[geom]
    p = O.default_params(w, h, *intr(w, h), **dict(dict(n_levels=nl, first_level=nl - 1, last_level=0), **over))
    p.has_depth = int(has)
    return p


_levels = {}


def level_planes(O, geom, slot):
    """[(gradient_, depth plane or None, (gw, gh))] of one slot on every level: the pyramid the context builds (cv::resize halves)"""
    key = (geom, slot)
    if key not in _levels:
        w, h, nl, _, has = GEOMS[geom]
        p = oracle_params(O, geom)
        imgs = O.pyramid(frames_of(geom)[slot], nl)
        deps = O.pyramid(depths_of(geom)[slot], nl) if has else [None] * nl
        out = []
        for l in range(nl):
            L = O.level_intrinsics(p, l)
            gx, gy = O.scharr3(imgs[l])
            out.append((PR.gradient_magnitude(gx, gy), deps[l], (L.w, L.h)))
        _levels[key] = out
    return _levels[key]


def magnitude_classes(gx, gy):
    """how often a gradient pair reaches each class of the magnitude step"""
    ax, ay = np.abs(gx.astype(np.int64)), np.abs(gy.astype(np.int64))
    s = np.minimum(ax, 255) + np.minimum(ay, 255)
    m = s >> 1
    # an odd sum needs one side clipped: unclipped, gx / 3 + gy / 3 = 2 (I[y+1, x+1] - I[y-1, x-1]) mod 2 is even
    other = np.where(ax >= 255, ay, ax)
    c = dict(mag_zero=s == 0, odd_rounds_down=(s & 1 == 1) & (m & 1 == 0), odd_rounds_up=(s & 1 == 1) & (m & 1 == 1) & (other != 0),
             one_saturated_other_zero=((ax > 255) & (ay == 0)) | ((ay > 255) & (ax == 0)), both_saturated=(ax > 255) & (ay > 255),
             g_just_below_255=(ax == 252) | (ay == 252), g_equal_255=(ax == 255) | (ay == 255), g_just_above_255=(ax == 258) | (ay == 258))
    return {k: int(v.sum()) for k, v in c.items()}


MAGNITUDE_CLASSES = ("mag_zero", "odd_rounds_down", "odd_rounds_up", "one_saturated_other_zero", "both_saturated", "g_just_below_255",
                     "g_equal_255", "g_just_above_255")


# ---- thresholds ------------------------------------------------------------------------------------------------------------------------------
def threshold_for(mean, target):
    """a double t with fl(mean + t) == target: fl(mean + t) is monotone in t, so a bisection over the doubles finds one unless the sum
    skips the target (then None; the tests assert it does not)"""
    lo, hi = target - mean - 1.0, target - mean + 1.0
    for _ in range(200):
        t = lo + (hi - lo) / 2
        s = mean + t
        if s == target:
            return t
        if t in (lo, hi):
            return None
        lo, hi = (t, hi) if s < target else (lo, t)
    return None


def equality_triple(mean, m):
    """(t_eq, t_below, t_above): fl(mean + t) is m, the double below m, the double above m"""
    m = float(m)
    return threshold_for(mean, m), threshold_for(mean, math.nextafter(m, -math.inf)), threshold_for(mean, math.nextafter(m, math.inf))


def pivot_magnitude(mag, grid):
    """the magnitude the equality thresholds are built on: of the distinct values the grid's cells hold above the mean, the one nearest
    the middle for which all three thresholds exist (where mean + t falls on ties only, fl() skips every other double)"""
    gw, gh = grid
    mean = PR.candidate_mean(mag)
    vals = np.unique(mag[:gh, :gw])
    vals = [int(v) for v in vals[vals > mean]]
    for v in sorted(vals, key=lambda v: abs(vals.index(v) - len(vals) // 2)):
        if None not in equality_triple(mean, v):
            return v
    raise AssertionError("no magnitude with all three thresholds")


FIXED_THRESHOLDS = {"frac": 0.37, "all": -300.0, "none": 300.0, "minus_1e300": -1e300, "plus_1e300": 1e300}

Cand = namedtuple("Cand", "name geom lvl first n pivot kind reach")


def threshold_of(O, case):
    """the case's threshold: an equality threshold of the pivot slot's level, or a fixed one"""
    if case.kind in FIXED_THRESHOLDS:
        return FIXED_THRESHOLDS[case.kind]
    mag, _, grid = level_planes(O, case.geom, case.pivot)[case.lvl]
    t = equality_triple(PR.candidate_mean(mag), pivot_magnitude(mag, grid))
    return t[("eq", "below", "above").index(case.kind)]


def _cand(geom, lvl, kind, reach=(), first=0, n=1, pivot=None, tag=""):
    pivot = first if pivot is None else pivot
    every = ("all_pass_threshold",) + (() if GEOMS[geom][4] else ("all_cells",))   # with a depth plane the zero bytes still drop cells
    reach = tuple(reach) + {"eq": ("thres_eq_m",), "below": ("thres_below_m",), "above": ("thres_above_m",), "all": every,
                            "none": ("no_cell",), "plus_1e300": ("no_cell",), "minus_1e300": every}.get(kind, ())
    return Cand("%s_l%d_%s%s" % (geom, lvl, kind, tag), geom, lvl, first, n, pivot, kind, reach)


def _build_candidates():
    out = []
    triple = ("eq", "below", "above")
    # 64 x 48, with depth: every level, and the frame count of the call (the band split depends on it), slots not starting at 0
    for lvl, r in ((0, ("m_lt_1024",)), (1, ()), (2, ()), (3, ("bands_1",))):
        for kind in triple:
            out.append(_cand("g64x48", lvl, kind, r + ("depth_lo_ne_hi",)))
    for kind in triple + ("all",):
        out.append(_cand("g64x48", 0, kind, ("slots_from_1",), first=1, n=3, pivot=2, tag="_n3"))
        out.append(_cand("g64x48", 0, kind, ("slots_from_2", "eight_frames"), first=2, n=8, pivot=5, tag="_n8"))
    out.append(_cand("g64x48", 1, "eq", ("slots_from_2", "eight_frames"), first=2, n=8, pivot=4, tag="_n8"))
    out.append(_cand("g64x48", 0, "eq", ("depth_all_selected_on_zero",), first=1, n=1, tag="_slot1"))   # see all_zero_depth below
    out.append(_cand("g64x48", 0, "all", ("depth_lo_zero_hi_not",), first=1, n=1, tag="_slot1"))
    out.append(_cand("g64x48", 0, "all", ("depth_hi_zero_lo_not",), first=2, n=1, tag="_slot2"))
    out.append(_cand("g64x48", 0, "eq", ("depth_zero_byte_on_selected",), first=3, n=1, tag="_slot3"))
    out.append(_cand("g64x48", 2, "frac", (), first=3, n=1, tag="_slot3"))
    # the power-of-two pixel count, gw * bands == 1024
    for kind in triple + tuple(FIXED_THRESHOLDS):
        out.append(_cand("g128x64", 0, kind, ("m_eq_1024", "dyadic_mean")))
    out.append(_cand("g128x64", 1, "eq", ("m_lt_1024", "dyadic_mean")))
    for kind in triple + ("all",):
        out.append(_cand("g160x96", 0, kind, ("m_gt_1024_ragged",)))
        out.append(_cand("g40x90", 0, kind, ("empty_last_band",)))
        out.append(_cand("g272x24", 0, kind, ("two_column_blocks",)))
    out.append(_cand("g272x24", 1, "eq"))
    for lvl, r in ((0, ("pitch_gt_iw",)), (1, ("pitch_gt_iw", "grid_lt_image", "beyond_grid_moves_mean")),
                   (2, ("pitch_gt_iw", "grid_lt_image", "beyond_grid_moves_mean")), (3, ())):
        for kind in triple + (("all",) if lvl in (1, 2) else ()):
            out.append(_cand("g163x99", lvl, kind, r + ("depth_lo_ne_hi",), first=0, n=3, pivot=1, tag="_n3"))
    for lvl, r in ((0, ("pitch_gt_iw", "mean_not_dyadic")), (1, ("pitch_gt_iw", "grid_lt_image", "beyond_grid_moves_mean")),
                   (2, ("grid_lt_image", "beyond_grid_moves_mean"))):
        for kind in triple + ("all", "frac"):
            out.append(_cand("g46x35", lvl, kind, r))
    return out


CANDIDATES = _build_candidates()
CAND_BY_NAME = {c.name: c for c in CANDIDATES}
assert len(CAND_BY_NAME) == len(CANDIDATES)


def all_zero_depth(O, case):
    """for the depth_all_selected_on_zero case: slot 1's plane (0x0100) with the high byte cleared under every ODD byte column the case
    selects — every selected cell then reads a zero byte, while the plane is far from empty"""
    mag, dep, (gw, gh) = level_planes(O, case.geom, case.first)[case.lvl]
    rows, _ = PR.candidate_points(mag, None, threshold_of(O, case), (gw, gh))
    b = np.ascontiguousarray(dep).view(np.uint8).reshape(dep.shape[0], 2 * dep.shape[1]).copy()
    b[rows[:, 1].astype(int), rows[:, 0].astype(int)] = 0
    return np.ascontiguousarray(b).view("<u2").reshape(dep.shape).astype(np.uint16)


def candidate_inputs(O, case):
    """[(gradient_, depth or None, (gw, gh))] for the frames first .. first + n - 1 of a case, and its threshold"""
    frames = [level_planes(O, case.geom, s)[case.lvl] for s in range(case.first, case.first + case.n)]
    if "depth_all_selected_on_zero" in case.reach:
        frames = [(m, all_zero_depth(O, case), g) for m, _, g in frames]
    return frames, threshold_of(O, case)


def level0_depths(O, case):
    """the level-0 depth planes to upload for a case's slots (None: the geometry's own)"""
    if "depth_all_selected_on_zero" in case.reach:
        assert case.lvl == 0
        return {case.first: all_zero_depth(O, case)}
    return {}


def candidate_classes(O, case):
    """the classes a candidate case reaches, from its inputs and the restatement's rows: {class: count or flag}"""
    frames, t = candidate_inputs(O, case)
    w, h, nl, slots, has = GEOMS[case.geom]
    mag, dep, (gw, gh) = level_planes(O, case.geom, case.pivot)[case.lvl]
    if "depth_all_selected_on_zero" in case.reach:
        dep = frames[0][1]
    ih, iw = mag.shape
    mean = PR.candidate_mean(mag)
    m = pivot_magnitude(mag, (gw, gh))
    thres = mean + t
    bands, rows = PR.bands_of(gw, gh, case.n)
    cells = gw * bands
    sel, n_sel = PR.candidate_points(mag, None, t, (gw, gh))
    got = dict(thres_eq_m=thres == float(m), thres_below_m=thres == math.nextafter(float(m), -math.inf),
               thres_above_m=thres == math.nextafter(float(m), math.inf), all_pass_threshold=n_sel == gw * gh,
               all_cells=PR.candidate_points(mag, dep, t, (gw, gh))[1] == gw * gh, no_cell=n_sel == 0, bands_1=bands == 1 and gh < 8,
               empty_last_band=(bands - 1) * rows >= gh, m_lt_1024=cells < 1024, m_eq_1024=cells == 1024,
               m_gt_1024_ragged=cells > 1024 and cells % 1024 != 0, two_column_blocks=gw > PR.K_BLOCK,
               grid_lt_image=gw < iw or gh < ih, pitch_gt_iw=PR.pitch_of(iw) > iw,
               beyond_grid_moves_mean=PR.candidate_mean(mag, (gw, gh), "mean_over_grid") != mean,
               dyadic_mean=(iw * ih) & (iw * ih - 1) == 0, mean_not_dyadic=mean * 2.0 ** 40 != math.floor(mean * 2.0 ** 40),
               slots_from_1=case.first == 1, slots_from_2=case.first == 2, eight_frames=case.n == 8)
    if dep is not None:
        by = PR.depth_bytes(dep)[:gh, :gw]
        lo = (np.asarray(dep, np.uint16)[:gh, :gw] & 0xFF)
        sx, sy = sel[:, 0].astype(int), sel[:, 1].astype(int)
        got.update(depth_zero_byte_on_selected=bool(n_sel and (by[sy, sx] == 0).any() and (by[sy, sx] != 0).any()),
                   depth_all_selected_on_zero=bool(n_sel and (by[sy, sx] == 0).all() and (by != 0).any()),
                   depth_lo_ne_hi=bool(n_sel and (by[sy, sx] != lo[sy, sx]).any()),
                   depth_lo_zero_hi_not=bool(((dep & 0xFF) == 0).all() and ((dep >> 8) != 0).all()),
                   depth_hi_zero_lo_not=bool(((dep & 0xFF) != 0).all() and ((dep >> 8) == 0).all()))
    return got, m


# ---- key points ------------------------------------------------------------------------------------------------------------------------------
def edge_values(n):
    """the coordinates at which a patch of half-width 5 changes what it covers, in an image n wide"""
    return [0.0, 0.5, 4.5, 5.0, 5.5, n - 6.0, n - 5.5, n - 1.0, n - 0.5]


Patch = namedtuple("Patch", "name kp reach")


def _interior(rng, w, h, n):
    return rng.uniform([6, 6], [w - 7, h - 7], (n, 2)).astype(F32)


def patch_sets(w, h):
    """the key-point sets of a w x h level 0, in a fixed order; every coordinate is inside the documented domain 0 <= x < w, 0 <= y < h"""
    rng = np.random.default_rng(31)
    ex, ey = edge_values(w), edge_values(h)
    grid = np.array([[x, y] for x in ex for y in ey], F32)
    many = np.concatenate([grid, _interior(rng, w, h, 256 - len(grid))])
    many[200] = [w / 2 + 0.25, h / 2 + 0.75]        # key point 201: interior, 121 cells it must not add
    on_depths = np.array([[x + 0.75, y + 0.5] for x, y in KP_DEPTH_AT], F32)     # fractions: read at ((int)y, (int)x)
    sets = [
        Patch("edges", grid, ("border_low", "border_high", "fraction_half", "i_eq_0_cell", "upper_bound_on_integer")),
        Patch("minus_zero", np.array([[-0.0, -0.0], [-0.0, 7.5], [9.0, -0.0]], F32), ("minus_zero", "border_low")),
        Patch("on_depths", on_depths, ("depth_0", "depth_1", "depth_7fff", "depth_8000", "depth_ffff")),
        Patch("none", np.zeros((0, 2), F32), ("count_0",)),
        Patch("one", many[:1], ("count_1",)),
        Patch("n199", many[:199], ("count_199",)),
        Patch("n200", many[:200], ("count_200",)),
        Patch("n201", many[:201], ("count_201", "cut_at_200")),
        Patch("n256", many, ("count_256", "cut_at_200")),
        Patch("duplicates", np.tile(np.array([[20.25, 11.75]], F32), (30, 1)), ("duplicates",)),
        Patch("asymmetric", np.array([[30.5, 8.0], [12.0, 20.5], [3.0, 30.25]], F32), ("order_shows", "fraction_half")),
    ]
    return sets


REFUSED_KEYPOINTS = {"x_eq_w": lambda w, h: [[float(w), 3.0]], "y_eq_h": lambda w, h: [[3.0, float(h)]],
                     "nan": lambda w, h: [[float("nan"), 3.0]], "negative": lambda w, h: [[-0.25, 3.0]],
                     "second_bad": lambda w, h: [[3.0, 3.0], [5.0, -1.0]]}


def patch_classes(kp, depth0, w, h):
    kp = np.asarray(kp, F32).reshape(-1, 2)
    x, y = kp[:, 0], kp[:, 1]
    got = dict(border_low=bool(((x < 5) | (y < 5)).any()), border_high=bool(((x > w - 6) | (y > h - 6)).any()),
               fraction_half=bool(((x % 1 == 0.5) | (y % 1 == 0.5)).any()), minus_zero=bool((np.signbit(kp) & (kp == 0)).any()),
               i_eq_0_cell=bool(((x - 5 <= 0) & (x + 5 >= 0)).any()), upper_bound_on_integer=bool(((x + 5) % 1 == 0).any()),
               duplicates=len(kp) > 1 and len(np.unique(kp, axis=0)) < len(kp), cut_at_200=len(kp) > 200,
               order_shows=bool(len(kp) and not PR.same_bits(PR.patch_points(kp, None, w, h)[0], PR.patch_points(kp, None, w, h, mut="patch_y_outer")[0])))
    for n in (0, 1, 199, 200, 201, 256):
        got["count_%d" % n] = len(kp) == n
    if depth0 is not None and len(kp):
        d = np.asarray(depth0, np.uint16)[y.astype(int), x.astype(int)]
        for v, k in zip(KP_DEPTHS, ("depth_0", "depth_1", "depth_7fff", "depth_8000", "depth_ffff")):
            got[k] = bool((d == v).any())
    return got


# ---- add_patch_points tables -----------------------------------------------------------------------------------------------------------------
Table = namedtuple("Table", "name pts patch_sizes reach")


def table_sets(w, h):
    """point tables of a w x h level: (x, y, z, w) rows; z distinct per row so that a cell shows which point it came from"""
    rng = np.random.default_rng(41)

    def rows(xy):
        xy = np.asarray(xy, F32).reshape(-1, 2)
        z = (0.5 + 0.001 * np.arange(len(xy))).astype(F32)
        return np.column_stack([xy, z, np.ones(len(xy), F32)]).astype(F32)

    ties = [[k + 0.5, j + 0.5] for k, j in ((0, 0), (1, 2), (2, 1), (3, 4), (6, 7), (w - 2, h - 2))] + [[-0.5, 3.0], [3.0, -0.5], [-0.5, -0.5],
                                                                                                       [2.5, 3.0], [4.0, 3.5]]
    borders = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w // 2, 0], [0, h // 2], [w - 1, h // 2], [w // 2, h - 1], [1, 1], [w - 2, h - 2]]
    frac = [[3.4, 2.6], [7.25, 5.75], [w - 1.4, h - 1.6]]
    rand = lambda n: np.column_stack([rng.uniform(-0.5, w - 0.5, n), rng.uniform(-0.5, h - 0.5, n)])
    return [Table("ties", rows(ties), (1, 3, 5, 11), ("tie_half", "tie_minus_half")),
            Table("borders", rows(borders), (1, 3, 5, 11), ("on_border",)),
            Table("fractions", rows(frac), (3, 5), ("fraction",)),
            Table("n0", rows(np.zeros((0, 2))), (5,), ("count_0",)),
            Table("n1", rows(rand(1)), (1, 5), ("count_1",)),
            Table("n256", rows(rand(256)), (5,), ("count_256",)),
            Table("n257", rows(rand(257)), (3, 5), ("count_257",)),
            Table("n600", rows(rand(600)), (5,), ("count_600",))]


def table_classes(pts, w, h):
    x, y = pts[:, 0], pts[:, 1]
    fr = lambda v: v - np.floor(v)
    got = dict(tie_half=bool(((fr(x) == 0.5) & (x > 0)).any() and ((fr(y) == 0.5) & (y > 0)).any()), tie_minus_half=bool(((x == -0.5) | (y == -0.5)).any()),
               on_border=bool(((x == 0) | (x == w - 1)).any() and ((y == 0) | (y == h - 1)).any()),
               fraction=bool(((fr(x) != 0) & (fr(x) != 0.5)).any()))
    for n in (0, 1, 256, 257, 600):
        got["count_%d" % n] = len(pts) == n
    return got
