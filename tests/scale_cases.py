"""Designed residual histograms for the robust scale stage (tests/test_scale_cpu.py shows that every case reaches its target
and that the set is discriminating; tests/test_gpu_scale.py runs the same table through every device form).

The lever: without depth, or with any non-zero depth, the identity pose maps every grid pixel to itself, so the residual of pixel p
is I2[p] - I1[p] and the test chooses it.  A map that is constant on 2x2 blocks survives the halving of the pyramid, so levels 0 and
1 see the same map.  Row 0 and column 0 of a level fail x2 > 0 / y2 > 0 and never count; a pixel of depth 0 does not count either.

Two placements:
  spread   a shuffled map drawn from (value, share) pairs over the whole grid; every threshold of the case has a margin of several
           per cent of n, so the same (med, dmed) holds on both levels whatever the uncounted border holds;
  exact    explicit (value, count) pairs.  With depth: one level-0 pixel of depth per chosen cell, so that levels 0 and 1 count
           exactly the same multiset (the halved depth of such a block is non-zero).  Without depth: the counts fill the interior
           cells (level 1 exact) and the border cells hold `edge`.

What the restatement (tests/scale_ref.py) says can be realised, found while writing the cases and asserted in test_scale_cpu.py:
  * Tukey: dmed 0..255 (the u8 clamp); 255 only as the fallback (more than half of the deviations >= 255).
  * Huber: dmed 0..510, NOT 255: with n even, n/2 values at a and n/2 at b > a, the count at a equals n/2 and does not exceed
    it, so med = b, and the deviations are n/2 zeros and n/2 times b - a: dmed = b - a, up to 510 (a = -255, b = 255), which is the
    fallback of the 510 clamp.  Every dmed above 255 needs such an exact half, hence n even: those cases carry depth.
  * med + dmed > 255 (only the low side exists) also needs an exact half: the values above med all deviate by less than dmed, so
    they and med's own count must not exceed n/2, while the values below must not either.
  * med - dmed < -255 cannot happen: the values <= med number more than n/2 by the median's own rule and would all deviate by less
    than dmed.  The nearest case is med - dmed == -255 (the low side's last bin).
  * more than half of the mass negative under Tukey with a positive median cannot happen (bin 0 would cross); nearest: exactly half.
"""
import numpy as np

import scale_ref as R

TUKEY, HUBER = R.TUKEY, R.HUBER
KIND_NAME = {TUKEY: "tukey", HUBER: "huber"}

# name -> (width, height, intrinsics, n_levels)
SIZES = {"main": (128, 96, (96.0, 96.0, 63.5, 47.5), 2),
         "twin": (126, 94, (96.0, 96.0, 62.5, 46.5), 2),     # 126 / 63 wide, 94 / 47 high: every level's rows end inside a group of four
         "sweep": (64, 48, (48.0, 48.0, 31.5, 23.5), 1)}
CONST_DEPTH = 5000      # 1 m at the default depth scale


def design(q_small, base_seed, depth=None, rep=2):
    """(I1, I2, depth) of a pair whose residual at the identity pose is q_small replicated rep x rep: I1 a texture clipped so that
    I2 = I1 + q stays a u8.  depth: None, a constant, or a level-0 u16 image."""
    q = np.repeat(np.repeat(np.asarray(q_small, np.int32), rep, 0), rep, 1)
    assert np.abs(q).max() <= 255
    tex = np.random.default_rng(base_seed).integers(0, 256, q.shape).astype(np.int32)
    i1 = np.clip(tex, np.maximum(0, -q), np.minimum(255, 255 - q))
    i2 = i1 + q
    assert i1.min() >= 0 and i2.min() >= 0 and i1.max() <= 255 and i2.max() <= 255
    if depth is not None and np.ndim(depth) == 0:
        depth = np.full(q.shape, depth, np.uint16)
    return i1.astype(np.uint8), i2.astype(np.uint8), None if depth is None else np.ascontiguousarray(depth, np.uint16)


class Case:
    def __init__(self, name, family, kind, target, q_small, doc, size="main", depth=None, n=None):
        self.name, self.family, self.kind, self.target, self.q_small, self.doc = name, family, kind, target, q_small, doc
        self.size, self.depth, self.n = size, depth, n      # n: the exact count of valid pixels on every level, where the case fixes it
        self.id = "%s-%s-%s" % (family, KIND_NAME[kind], name)

    @property
    def has_depth(self):
        return self.depth is not None

    @property
    def rep(self):
        return 1 if self.size == "sweep" else 2

    def frames(self):
        return design(self.q_small, 1000 + (hash_name(self.id) % 1000), self.depth, self.rep)

    def __repr__(self):
        return self.id


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def small_shape(size):
    w, h, _, _ = SIZES[size]
    return (h, w) if size == "sweep" else (h // 2, w // 2)


def spread(shares, seed, size="main"):
    """A shuffled map over the whole small grid from (value, share) pairs; what rounding leaves over goes to the first value."""
    hs, ws = small_shape(size)
    n = hs * ws
    vals = []
    for v, s in shares:
        vals += [v] * int(s * n)
    vals += [shares[0][0]] * (n - len(vals))
    vals = np.array(vals, np.int32)
    np.random.default_rng(seed).shuffle(vals)
    return vals.reshape(hs, ws)


def exact_depth(counts, seed, fill=0):
    """(q_small, depth, n): every (value, count) on cells of the interior, one level-0 pixel of depth per cell; the rest `fill`, no depth"""
    hs, ws = small_shape("main")
    cells = [(y, x) for y in range(1, hs) for x in range(1, ws)]
    rng = np.random.default_rng(seed)
    rng.shuffle(cells)
    q = np.full((hs, ws), fill, np.int32)
    depth = np.zeros((2 * hs, 2 * ws), np.uint16)
    i = 0
    for v, c in counts:
        for _ in range(c):
            y, x = cells[i]
            q[y, x] = v
            depth[2 * y + int(rng.integers(0, 2)), 2 * x + int(rng.integers(0, 2))] = 4000 + 8 * int(rng.integers(0, 500))
            i += 1
    return q, depth, i


def exact_edge(counts, edge, seed):
    """q_small without depth: the counts fill the interior cells (they must number all of them), the border cells hold `edge`"""
    hs, ws = small_shape("main")
    vals = np.array([v for v, c in counts for _ in range(c)], np.int32)
    assert vals.size == (hs - 1) * (ws - 1)
    np.random.default_rng(seed).shuffle(vals)
    q = np.full((hs, ws), edge, np.int32)
    q[1:, 1:] = vals.reshape(hs - 1, ws - 1)
    return q


def lane_boundaries(lo, hi, offset=0):
    """v and v + 1 for every v in [lo, hi) whose bin v + offset is the last of a lane (8 bins per lane)"""
    out = []
    for v in range(lo, hi):
        if (v + offset) % 8 == 7:
            out += [v, v + 1]
    return out


TUKEY_DMED_LIMIT = 255
HUBER_DMED_LIMIT = 510


def build_cases():
    cases = []

    def add(*a, **kw):
        cases.append(Case(*a, **kw))

    # ---- lane walk: the deviation crossing in the last bin of a lane (k == 7) and in the first bin of the next; 40 % of the mass
    # sits at deviation 0, so the crossing lane gets its count through the carry of the 64-lane scan, and every lane behind the
    # crossing crosses too (the min reduction picks the first)
    for kind in (TUKEY, HUBER):
        for i, d in enumerate(lane_boundaries(0, 255)):      # 7, 8, ..., 247, 248; 255 is the saturation family's
            side = 1 if (i // 2) % 2 == 0 else -1       # the deviation bin fed from the high side, or from the low side
            add("dmed%d" % d, "lane_dmed", kind, (0, d), spread([(0, 0.4), (side * d, 0.3), (-side * 255, 0.3)], 100 + d),
                "deviation crossing at bin %d = lane %d, k = %d; scan carry from lane 0; every lane behind it crosses too (min reduction); "
                "fed from the %s side" % (d, d // 8, d % 8, "high" if side > 0 else "low"))
    # Huber above 255: exact halves (see the head of the file), n even, through depth
    for d in [255, 256] + [d for d in lane_boundaries(256, 509)] + [509, 510]:
        q, dep, n = exact_depth([(-255, 600), (d - 255, 600)], 300 + d)
        add("dmed%d" % d, "lane_dmed", HUBER, (d - 255, d), q, "Huber deviation %d by an exact half: lane %d, k = %d%s"
            % (d, d // 8, d % 8, "; 510 = the clamp's fallback (no bin crosses)" if d == 510 else ""), depth=dep, n=n)
    # the median crossing likewise: Tukey over the saturated values (30 % of the mass negative, all in the saturation bin 0 while
    # the median is positive), Huber over the signed ones (30 % at -255: lane 0 carries into the crossing lane)
    for m in lane_boundaries(0, 255):
        add("med%d" % m, "lane_med", TUKEY, (m, 1), spread([(m, 0.4), (-3, 0.3), (m + 1, 0.3)], 500 + m),
            "Tukey median at bin %d = lane %d, k = %d; the negative saturation bin holds 30 %%" % (m, m // 8, m % 8))
    add("med255", "lane_med", TUKEY, (255, 0), spread([(255, 0.6), (254, 0.4)], 755), "Tukey median in the last bin, 255")
    for m in lane_boundaries(-254, 255, offset=255):
        add("med%d" % m, "lane_med", HUBER, (m, 1), spread([(m, 0.4), (-255, 0.3), (m + 1, 0.3)], 700 + m),
            "Huber median at bin %d = lane %d, k = %d" % (m + 255, (m + 255) // 8, (m + 255) % 8))
    add("med-255", "lane_med", HUBER, (-255, 0), spread([(-255, 0.6), (-254, 0.4)], 1001), "Huber median in the first bin, -255")
    add("med255", "lane_med", HUBER, (255, 0), spread([(255, 0.6), (254, 0.4)], 1002), "Huber median in the last bin, 255 (lane 63, k = 6)")

    # ---- one-sided deviations
    for kind in (TUKEY, HUBER):
        q, dep, n = exact_depth([(100, 300), (80, 200), (200, 400), (255, 100)], 1100 + kind)
        add("med200_dmed100", "one_sided", kind, (200, 100), q, "med + d > 255: only the low side contributes; an exact half "
            "below the median and an exact half of deviations below 100", depth=dep, n=n)
    q, dep, n = exact_depth([(-255, 500), (-200, 400), (-145, 100)], 1103)
    add("med-200_dmed55", "one_sided", HUBER, (-200, 55), q, "the mirror: med - d == -255, the low side's last bin (med - d < -255 "
        "cannot be a crossing, see the head of the file)", depth=dep, n=n)
    add("med-200_dmed55_spread", "one_sided", HUBER, (-200, 55), spread([(-200, 0.4), (-255, 0.3), (0, 0.3)], 1104),
        "med - d == -255 without depth")

    # ---- saturation and degeneracy
    add("fallback", "saturation", TUKEY, (0, 255), spread([(0, 0.4), (-255, 0.3), (255, 0.3)], 1200),
        "Tukey: 60 % of the deviations at 255: no bin below the clamp crosses, the fallback gives 255")
    add("two_sided_255", "saturation", TUKEY, (0, 255), spread([(-255, 0.55), (255, 0.45)], 1201),
        "Tukey: every deviation saturates; the fallback with an empty deviation histogram")
    add("dmed255", "saturation", HUBER, (0, 255), spread([(0, 0.4), (-255, 0.3), (255, 0.3)], 1202), "Huber: deviation 255 is an ordinary bin")
    for kind in (TUKEY, HUBER):
        add("all0", "saturation", kind, (0, 0), spread([(0, 1.0)], 1210), "dmed == 0 (MAD 0 -> 1), all residuals 0")
        add("all200", "saturation", kind, (200, 0), spread([(200, 1.0)], 1211),
            "dmed == 0, all residuals 200" + ("; every Tukey weight is 0 (A = 0 into the solve)" if kind == TUKEY else "; Huber quotient at ax = 200"))
    add("all-200", "saturation", TUKEY, (0, 200), spread([(-200, 1.0)], 1212), "all residuals -200: Tukey's saturated median is 0, the deviation 200")
    add("all-200", "saturation", HUBER, (-200, 0), spread([(-200, 1.0)], 1212), "dmed == 0, all residuals -200")
    q, dep, n = exact_depth([(-50, 500), (100, 500)], 1220)
    add("half_negative", "saturation", TUKEY, (100, 150), q, "Tukey: exactly half of the mass in the negative saturation bin, the "
        "median positive (more than half cannot be)", depth=dep, n=n)

    q, dep, n = exact_depth([(-200, 500), (100, 500)], 1221)
    add("half_beyond_clamp", "saturation", TUKEY, (100, 255), q, "Tukey: half of the deviations are 300, which the u8 clamp turns "
        "into 255 (the only way a deviation above 255 decides: more than half cannot be that negative)", depth=dep, n=n)

    # ---- ties at the threshold
    for kind in (TUKEY, HUBER):
        q, dep, n = exact_depth([(3, 500), (12, 300), (14, 200)], 1300 + kind)
        add("n1000", "ties", kind, (12, 9), q, "n even: the count through 3 equals n / 2 and the count of deviations <= 2 too; the "
            "crossing is the next occupied bin both times", depth=dep, n=n)
        q, dep, n = exact_depth([(3, 500), (12, 300), (14, 200), (40, 1)], 1310 + kind)
        add("n1001", "ties", kind, (12, 9), q, "n odd against (float)(n / 2): both counts equal 500", depth=dep, n=n)
        add("n2961_no_depth", "ties", kind, (12, 9), exact_edge([(3, 1480), (12, 880), (14, 600), (40, 1)], 40, 1320 + kind),
            "n odd without depth: both counts equal n / 2 = 1480 on level 1; level 0 has the same answer with margins")
        for k, vals in enumerate([[], [37], [37, -5], [37, -5, 120]]):
            q, dep, n = exact_depth([(v, 1) for v in vals], 1330 + k, fill=77)
            tgt = {0: (None, None), 1: (37, 0), 2: (37, 42), 3: (37, 42)}[k]
            add("n%d" % k, "ties", kind, tgt, q, "n == %d through zero depth%s" % (k, "" if k else ": no valid pixel, MAD 1"), depth=dep, n=n)

    # ---- one constant-depth twin of each family, one odd-sized twin of each family
    for fam, kind, name, tgt, shares in [("lane_dmed", TUKEY, "dmed127", (0, 127), [(0, 0.4), (127, 0.3), (-255, 0.3)]),
                                         ("lane_dmed", HUBER, "dmed128", (0, 128), [(0, 0.4), (-128, 0.3), (255, 0.3)]),
                                         ("lane_med", TUKEY, "med63", (63, 1), [(63, 0.4), (-3, 0.3), (64, 0.3)]),
                                         ("lane_med", HUBER, "med-8", (-8, 1), [(-8, 0.4), (-255, 0.3), (-7, 0.3)]),
                                         ("one_sided", HUBER, "med-200_dmed55", (-200, 55), [(-200, 0.4), (-255, 0.3), (0, 0.3)]),
                                         ("saturation", TUKEY, "fallback", (0, 255), [(0, 0.4), (-255, 0.3), (255, 0.3)]),
                                         ("saturation", TUKEY, "all200", (200, 0), [(200, 1.0)]),
                                         ("ties", HUBER, "margins", (12, 9), [(12, 0.3), (3, 0.4), (14, 0.15), (40, 0.15)])]:
        add(name + "_const_depth", fam, kind, tgt, spread(shares, 1400), "constant depth: the same mapping", depth=CONST_DEPTH)
        add(name + "_126x94", fam, kind, tgt, spread(shares, 1401, "twin"), "126x94: the ragged instantiations", size="twin")
    return cases


def sweep_map(d, seed=0):
    """64x48 map, median 0, deviation d, every integer of [-255, 255] at least once among the 63 x 47 counted pixels: the 511
    values once, then 900 at 0, 850 at +d and 700 at -d (2450 left over; checked by test_scale_cpu.py for every d)."""
    hs, ws = small_shape("sweep")
    vals = np.array(list(range(-255, 256)) + [0] * 900 + [d] * 850 + [-d] * 700, np.int32)
    assert vals.size == (hs - 1) * (ws - 1)
    np.random.default_rng(2000 + d + seed).shuffle(vals)
    q = np.zeros((hs, ws), np.int32)
    q[1:, 1:] = vals.reshape(hs - 1, ws - 1)
    return q


def sweep_cases(kind, ds=range(256)):
    """One frame per deviation 0..255 at median 0: together every pair (residual value, scale) an integer-residual evaluation can meet
    under that median — the Huber quotient k / ax for ax up to 255 (d == 0: MAD 1), the Tukey polynomial and its cut-off."""
    return [Case("d%d" % d, "sweep", kind, (0, d), sweep_map(d), "weight sweep, deviation %d%s" % (d, ": MAD 0 -> 1, the Huber "
                 "quotient k / ax for ax up to 255" if d == 0 else ""), size="sweep") for d in ds]


CASES = build_cases()
FAMILIES = ["lane_dmed", "lane_med", "one_sided", "saturation", "ties"]


# ---------------------------------------------------------------- the oracle's view of a case (shared by the CPU and the GPU tests)

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


def oracle_params(O, case, **over):
    w, h, intr, nl = SIZES[case.size]
    kw = dict(n_levels=nl, first_level=nl - 1, last_level=0, has_depth=int(case.has_depth), weights=case.kind)
    kw.update(over)
    return O.default_params(w, h, *intr, **kw)


def level_map(case, lvl):
    """the designed residual of every grid pixel of a level"""
    q = np.asarray(case.q_small, np.int32)
    if case.rep == 2 and lvl == 0:
        q = np.repeat(np.repeat(q, 2, 0), 2, 1)
    return q


def evaluate(O, case, lvl, sampler=0, frames=None):
    """(J, r, idx, n_grid) of the oracle's residual evaluation of a case's level at the identity pose, under the active arithmetic set"""
    i1, i2, dep = case.frames() if frames is None else frames
    nl = SIZES[case.size][3]
    p = oracle_params(O, case, sampler=sampler)
    L = O.level_intrinsics(p, lvl)
    a, b = O.pyramid(i1, nl)[lvl], O.pyramid(i2, nl)[lvl]
    d = O.pyramid(dep, nl)[lvl] if dep is not None else None
    gx, gy = O.scharr3(a)
    pts = O.dense_points(d, L.w, L.h, lvl)
    J, r, idx = O.residual_jacobian_ex(a, b, gx, gy, pts, O.warp(pts, IDENTITY, L), L, sampler=sampler)
    return J, r, idx, L.w * L.h
