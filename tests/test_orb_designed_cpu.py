"""The ORB restatement (tests/orb_ref.py) held to the designed catalogue of tests/orb_designed_cases.py — no device.  Three things:
orb_ref gives the hand-written expectation on every case; each case reaches the classes it declares and every class occurs; each
deliberate mistake orb_ref can be asked to make (`mut`) is noticed by the case named for it, or is argued equivalent.  The mutant
table is printed under `pytest -s`.  Every comparison is exact."""
import time

import numpy as np
import pytest

import orb_cases as K
import orb_designed_cases as D
import orb_ref as O

ARITH_INDEPENDENT = True   # ORB has no arithmetic set
F32 = np.float32
CASES = D.all_cases()
BY = {c["name"]: c for c in CASES}
assert len(BY) == len(CASES)
GROUPS = {"rings_t20": [c for c in CASES if c["family"] == "rings" and c["params"]["fast_threshold"] == D.T],
          "rings_t0": [c for c in CASES if c["family"] == "rings" and c["params"]["fast_threshold"] == 0],
          "rings_t255": [c for c in CASES if c["family"] == "rings" and c["params"]["fast_threshold"] == 255],
          "dots": [c for c in CASES if c["family"] == "dots"], "lattice": [c for c in CASES if c["family"] == "lattice"],
          "steer": [c for c in CASES if c["family"] == "steer"]}
T0 = time.time()

_ref = {}


def ref_of(c):
    """orb_ref's (key points, descriptors) of a case, computed once.  A lattice case runs orb_ref's detection under its own quota
    and capacity; the direction and descriptor of a key point depend on its position alone, so they are orb_ref's description of
    the frame's whole list, computed once per frame, at the positions the case's detection kept."""
    if c["name"] not in _ref:
        if c["family"] == "steer":
            _ref[c["name"]] = O.describe(c["img"], c["kp"], c["params"], c["pattern"])
        elif c["family"] == "lattice":
            key = ("whole", c["kind"])
            if key not in _ref:
                k, d = O.detect_describe(c["img"], D.params(n_features=65536), 4096)
                _ref[key] = ({(float(r["x"]), float(r["y"])): i for i, r in enumerate(k)}, k, d)
            at, wk, wd = _ref[key]
            k = O.detect(c["img"], c["params"], c["cap"])[0]
            rows = [at[(float(r["x"]), float(r["y"]))] for r in k]
            k["dir_x"], k["dir_y"] = wk["dir_x"][rows], wk["dir_y"][rows]
            _ref[c["name"]] = (k, wd[rows])
        else:
            _ref[c["name"]] = O.detect_describe(c["img"], c["params"], c["cap"], c["pattern"])
    return _ref[c["name"]]


def literal_map(c):
    S = np.zeros(c["img"].shape, np.int32)
    for (x, y), v in c["scores"].items():
        S[y, x] = v
    return S


@pytest.mark.parametrize("group", list(GROUPS))
def test_restatement_equals_hand_expectation(group):
    for c in GROUPS[group]:
        p, name = c["params"], c["name"]
        wk, wd = ref_of(c)
        ek, ed, full = D.expectation(c)
        if not full:      # the direction is orb_ref's own there (the case says so); everything else is not
            assert c["from_ref"] == "direction and descriptor"
            ek = ek.copy()
            assert len(ek) == len(wk), name
            ek["dir_x"], ek["dir_y"] = wk["dir_x"], wk["dir_y"]
        assert K.same_keypoints(wk, ek) is None, (name, K.same_keypoints(wk, ek))
        if ed is not None:
            assert D.same_descriptors(wd, ed) is None, (name, D.same_descriptors(wd, ed))
        if c["family"] in ("rings", "dots"):
            S = O.fast_scores(c["img"], p["edge_threshold"], p["fast_threshold"])
            hand = D.hand_score_map(c["img"], p["edge_threshold"], p["fast_threshold"])
            assert np.array_equal(S, hand), name
            if "scores" in c:
                assert np.array_equal(S, literal_map(c)), name
                assert [(int(x), int(y)) for y, x in zip(*O.suppress(S))] == c["kept"] == D.hand_kept(hand), name
            else:
                assert S[D.RING_C[1], D.RING_C[0]] == c["centre_score"], name
        if c["family"] == "rings":
            assert D.hand_score(c["img"], *D.RING_C) == c["centre_raw"], name


def test_literals_and_arithmetic_of_the_case_file():
    """what the case file writes twice agrees with itself: the dot rule with the literal lists, an isolated dot's H with
    3024 v^4, the plain lattice's H with 21504 * 255^4 and with the pixel loop, the steered moments and their f32 facts"""
    for c in GROUPS["dots"]:
        assert c["kept"] == c["kept_literal"], c["name"]
        assert len(c["kept"]) == {"dots_96x80": 20, "dots_128x96": 16}[c["name"]]
    d96 = BY["dots_96x80"]["img"]
    assert D.hand_harris(d96, 16, 28) == 3024 * 201 ** 4          # 21 (12 v^2)^2
    lat = D.lattice_frame("plain")
    assert D.H_PLAIN == 90924301440000 == D.hand_harris(lat, 18, 18) == D.hand_harris(lat, 238, 222)
    cand = D.lattice_candidates("graded")
    assert len(cand) == D.LATTICE_N and len({r[2] for r in cand}) == 200
    g = D.lattice_frame("graded")
    for y, x, H in cand[::97]:
        assert D.hand_harris(g, x, y) == H
    assert D.hand_moments(lat, 18, 18) == (0, 0) and D.hand_moments(lat, 238, 222) == (0, 0)
    # the steered half
    for name, (variant, moments, direction) in D.STEER_VARIANTS.items():
        img = BY[name]["img"]
        assert D.hand_moments(img, *D.STEER_C) == moments, name
        got = D.hand_direction(img, *D.STEER_C)
        assert (got[0].tobytes(), got[1].tobytes()) == (F32(direction[0]).tobytes(), F32(direction[1]).tobytes()), (name, got)
    fx, fy = F32(2911), F32(5042)
    n = np.sqrt(F32(F32(fx * fx) + F32(fy * fy)))
    assert n.dtype == np.float32 and n == 5822 and F32(fx / n) == 0.5 and F32(fy / n) == F32(0.86602545)
    assert O.pattern_ok(D.steer_pattern())
    assert D.hand_moments(BY["steer_mirror"]["img"], *D.STEER_C)[0] == 0
    k, _, _ = D.expectation(BY["steer_mirror"])
    assert k["dir_x"][0] == 0 and abs(k["dir_y"][0]) == 1
    assert not D.expectation(BY["steer_flat"])[1].any()


def test_the_tie_is_reached_and_every_rounding_mutant_flips_a_bit():
    """the f64 value of the f32 expression x0 * c - y0 * s has fraction exactly 0.5 at the entries built for it, with rnd(1.5) = 2
    and rnd(-1.5) = -1 among them, and each of the three wrong roundings changes the steered descriptor"""
    pat = D.steer_pattern()
    co = D.hand_coordinates(D.C_HALF, D.S_HALF, pat).astype(np.float64)
    for k, x0 in enumerate(D.TIE_X0):
        assert co[k, 0] == x0 / 2.0 and co[k, 0] - np.floor(co[k, 0]) == 0.5, k
        assert co[14 + k, 1] == x0 / 2.0, k          # (0, y0): the y coordinate y0 * c
    assert int(O.rnd(F32(1.5))) == 2 and int(O.rnd(F32(-1.5))) == -1 and int(O.rnd(F32(0.5))) == 1 and int(O.rnd(F32(-0.5))) == 0
    c = BY["steer_pp"]
    want = ref_of(c)[1]
    for mut in ("rnd_rint", "rnd_away", "rnd_trunc"):
        got = O.describe(c["img"], c["kp"], c["params"], c["pattern"], mut=mut)[1]
        flipped = int(np.unpackbits(got ^ want).sum())
        print(mut, "flips", flipped, "bits of steer_pp")
        assert flipped >= 1, mut


def test_the_clamp_acts_only_under_weight_zero():
    """x1 = min(x0 + 1, w - 1) differs from x0 + 1 only where x0 = w - 1.  For every width 1..2100 and layer 1..7 either the layer
    is narrower than the frame and its last destination column has x0 <= w - 2, or it is as wide as the frame (w <= 3 at layer 1,
    w = 1 at layers 2 and 3) and N = 2 x w leaves fx = 0 throughout.  So the clamp never acts under a non-zero weight: the class is unreachable
    and the mutant `x1_unclamped` equivalent.  The same holds along y."""
    same = []
    for l in range(1, 8):
        w = np.arange(1, 2101, dtype=np.int64)
        lw = (w * 5 ** l + 6 ** l // 2) // 6 ** l
        ok = lw >= 1
        x0_last = ((2 * (lw - 1) + 1) * w - lw) // (2 * np.maximum(lw, 1))
        assert (((lw < w) & (x0_last <= w - 2)) | (lw == w))[ok].all(), l
        same += [(l, int(v)) for v in w[ok & (lw == w)]]
    assert same == [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1)], same   # (a frame one pixel wide has no layer 4)
    for l, w in same:
        assert all(((2 * x + 1) * w - w) % (2 * w) == 0 for x in range(w))


def test_layers_by_hand():
    """exact halves of the 22-bit sum round up; level 0 is the plane; the hand-picked pixels of layer 1; how many pixels of each
    frame's layers the missing 2^21 of the mutant changes"""
    for name, img, hand in D.layer_frames():
        h, w = img.shape
        assert O.layer(img, 0) is not None and np.array_equal(O.layer(img, 0), img)
        L1 = O.layer(img, 1)
        assert L1.shape == O.layer_size(w, h, 1)[::-1]
        for (x, y), want in hand.items():
            assert L1[y, x] == want, (name, x, y, L1[y, x], want)
        differ = sum(int((O.layer(img, l, mut="layer_no_round") != O.layer(img, l)).sum()) for l in range(1, 8))
        print(name, "layer 1", L1.shape, "pixels of layers 1..7 that the missing 2^21 changes:", differ)
        assert differ > 0
    assert sum(sum(cell) % 4 == 2 for _, cell, _ in D.LAYER_CELLS) >= 3                                        # cell sums 2, 1018 and 2: (s + 2) >> 2 rounds the half up
    assert O.layer_size(97, 91, 1) == (81, 76)


# ---- reach ---------------------------------------------------------------------------------------------------------------------
DIRS = {"n": (0, -1), "ne": (1, -1), "e": (1, 0), "se": (1, 1), "s": (0, 1), "sw": (-1, 1), "w": (-1, 0), "nw": (-1, -1)}
_per_image = {}


def stage_of(c):
    """(score map, (ys, xs, H) per layer) of a detecting case, shared by the cases of one frame and one (edge, threshold)"""
    p = c["params"]
    key = (id(c["img"]), p["edge_threshold"], p["fast_threshold"], p["n_levels"])
    if key not in _per_image:
        per = []
        for l in range(p["n_levels"]):
            L = O.layer(c["img"], l)
            per.append((O.fast_scores(L, p["edge_threshold"], p["fast_threshold"]),) + tuple(O.layer_candidates(L, p)))
        _per_image[key] = per
    return _per_image[key]


def raw_above(img, x, y, t):
    win = img[y - 3:y + 4, x - 3:x + 4]
    return win.min() != win.max() and D.hand_score(img, x, y) > t


def reach(c):
    r = set()
    p, img = c["params"], c["img"]
    e, t = p["edge_threshold"], p["fast_threshold"]
    h, w = img.shape
    if c["family"] == "rings":
        cx, cy = D.RING_C
        d = [int(img[cy + dy, cx + dx]) - int(img[cy, cx]) for dx, dy in O.RING]
        r.add("bright" if max(d) > -min(d) else "dark")
        on = [abs(v) > t for v in d]
        if any(on) and not all(on):
            start = next(i for i in range(16) if on[i] and not on[i - 1])
            run = next(j for j in range(1, 17) if not on[(start + j) % 16])
            if sum(on) == run:      # one arc
                r |= {"arc9": {"arc9"}, "arc8": {"arc8"}}.get("arc%d" % run, set())
                if run == 9 and start >= 8:
                    r.add("wrap_%d" % start)
        raw = D.hand_score(img, cx, cy)
        r |= ({"score_t1"} if raw == t + 1 else set()) | ({"score_t"} if raw == t else set())
        r |= {"thr%d" % t} if t in (0, 255) else set()
    if c["family"] in ("rings", "dots", "lattice", "lattice8"):
        per = stage_of(c)
        S = per[0][0]
        ys, xs = np.nonzero(S)
        if c["family"] in ("rings", "dots"):
            for name, (dx, dy) in DIRS.items():
                if (S[ys + dy, xs + dx] == S[ys, xs]).any():
                    r.add("eq_" + name)
            for y, x in zip(ys, xs):
                lx, ly = (x - e) % 32, (y - e) % 32
                side = [sx for sx in (-1, 1) if (lx == 0 and sx < 0 or lx == 31 and sx > 0) and e <= x + sx < w - e]
                vert = [sy for sy in (-1, 1) if (ly == 0 and sy < 0 or ly == 31 and sy > 0) and e <= y + sy < h - e]
                if any(S[y + dy, x + sx] >= S[y, x] for sx in side for dy in (-1, 0, 1)):
                    r.add("tile_lr")
                if any(S[y + sy, x + dx] >= S[y, x] for sy in vert for dx in (-1, 0, 1)):
                    r.add("tile_tb")
                if any(S[y + sy, x + sx] >= S[y, x] for sx in side for sy in vert):
                    r.add("tile_corner")
            kys, kxs = per[0][1], per[0][2]
            for y, x in zip(kys, kxs):
                r |= ({"band_first_col"} if x == e else set()) | ({"band_last_col"} if x == w - e - 1 else set())
                r |= ({"band_first_row"} if y == e else set()) | ({"band_last_row"} if y == h - e - 1 else set())
                off = [(x + dx, y + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                       if not (e <= x + dx < w - e and e <= y + dy < h - e)]
                if any(raw_above(img, qx, qy, t) for qx, qy in off):
                    r.add("off_band_neighbour")
            for y in range(e, h - e):
                r |= ({"outside_first_col"} if raw_above(img, e - 1, y, t) else set()) | ({"outside_last_col"} if raw_above(img, w - e, y, t) else set())
            for x in range(e, w - e):
                r |= ({"outside_first_row"} if raw_above(img, x, e - 1, t) else set()) | ({"outside_last_row"} if raw_above(img, x, h - e, t) else set())
        quota = O.level_quota(p["n_features"], p["n_levels"])
        kept = 0
        for l, (_, lys, lxs, H) in enumerate(per):
            n, q = len(lys), quota[l]
            kept += min(n, q)
            r |= ({"raw_le_1024"} if 0 < n <= 1024 else set()) | ({"raw_1025_2048"} if 1024 < n <= 2048 else set())
            r |= ({"raw_gt_2048"} if n > 2048 else set()) | ({"raw_not_multiple"} if n > 1024 and n % 1024 else set())
            r |= ({"quota_list_minus1"} if q == n - 1 else set()) | ({"quota_eq_list"} if q == n > 0 else set())
            r |= {"quota_list_plus1"} if q == n + 1 and n > 0 else set()
            Hs = np.sort(H)[::-1]
            if 0 < q < n and Hs[q - 1] == Hs[q]:
                r.add("quota_cuts_tie")
        r |= ({"kept_gt_1024"} if kept > 1024 else set()) | ({"cap_lt_kept_gt_1024"} if c["cap"] < kept and kept > 1024 else set())
        r |= {"cap_eq_kept"} if c["cap"] == kept else set()
    if c["family"] != "lattice8":
        k, _ = ref_of(c)
        pat = O.default_pattern() if c["pattern"] is None else c["pattern"]
        for i in list(range(len(k)))[:3]:
            gx, gy = int(k[i]["x"]), int(k[i]["y"])
            if not p["upright"] and D.hand_moments(img, gx, gy) == (0, 0):
                r.add("n0")
            r |= ({"c_half"} if abs(k[i]["dir_x"]) == 0.5 else set()) | ({"c_zero"} if k[i]["dir_x"] == 0 and abs(k[i]["dir_y"]) == 1 else set())
            co = D.hand_coordinates(k[i]["dir_x"], k[i]["dir_y"], pat).astype(np.float64)
            fl = np.floor(co)
            tie = co - fl == 0.5
            r |= ({"tie_pos"} if (tie & (fl >= 0)).any() else set()) | ({"tie_neg"} if (tie & (fl < 0)).any() else set())
            q = np.floor((co.astype(np.float32) + F32(0.5)).astype(np.float64)).astype(np.int64)
            if (img[gy + q[:, 1], gx + q[:, 0]] == img[gy + q[:, 3], gx + q[:, 2]]).any():
                r.add("equal_intensities")
    return r


def test_every_case_reaches_what_it_declares_and_every_class_occurs():
    seen = {}
    for c in CASES:
        got = reach(c)
        assert c["classes"] <= got, (c["name"], sorted(c["classes"] - got))
        assert c["classes"] <= set(D.CLASSES), c["name"]
        for cls in c["classes"]:
            seen.setdefault(cls, []).append(c["name"])
    # the layer class is reached by the layer frame (test_layers_by_hand asserts the pixels)
    assert any(sum(cell) % 4 == 2 for _, cell, _ in D.LAYER_CELLS)
    seen["layer_half"] = ["layers_96x96"]
    missing = [cls for cls in D.CLASSES if cls not in seen]
    assert not missing, missing
    print()
    for cls in D.CLASSES:
        print("%-22s %4d  %s" % (cls, len(seen[cls]), seen[cls][0]))


def test_the_eight_layer_lattice_is_worth_running():
    c = BY["lat_8layers"]
    per = stage_of(c)
    quota = O.level_quota(c["params"]["n_features"], 8)
    counts = [len(s[1]) for s in per]
    print("raw per layer", counts, "quota", quota)
    assert counts[0] == D.LATTICE_N > quota[0]
    k, _ = O.detect_describe(c["img"], c["params"], c["cap"])
    _ref[c["name"]] = (k, _)
    assert np.count_nonzero(np.bincount(k["octave"], minlength=8)[1:]) >= 1
    assert {"raw_gt_2048", "raw_1025_2048", "raw_le_1024"} <= reach(c)


def test_the_noise_pair_is_worth_chaining():
    """4718 raw candidates against a quota and a capacity of 4096, and more than 1024 symmetric matches under the ratio test"""
    import match_ref as M
    ref, tgt = D.noise_pair()
    p = D.params(n_features=D.NOISE_FEATURES)
    assert len(O.layer_candidates(ref, p)[0]) == 4718
    (k0, d0), (k1, d1) = O.detect_describe(ref, p, 4096), O.detect_describe(tgt, p, 4096)
    assert len(k0) == len(k1) == 4096
    m, _, _ = M.match(d0, d1, 0.65)
    assert len(m) == 4027
    # and the lattice is not: one descriptor for every dot
    assert len({bytes(r) for r in ref_of(BY["lat_nf65536"])[1]}) == 1


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
def names(*groups, extra=()):
    return [c["name"] for g in groups for c in GROUPS[g]] + list(extra)


LATTICE_FEW = ["lat_nf1", "lat_nf1023", "lat_cap1025", "grad_nf1039_inside", "grad_cap1039_inside", "grad_cap1037_between", "grad_nf14_between"]
FAST_SET = names("rings_t20", "rings_t0", "dots")
SELECT_SET = names("dots", extra=LATTICE_FEW)
DESCRIBE_SET = names("steer", "dots", extra=["ring_b9_s3_t20", "ring_d9_s12_t20", "lat_nf1", "grad_nf14_between"])
# mutant: (the case named for it, the cases it is tried on, what is compared)
MUTANT_TABLE = {
    "fast_ge": ("ring_b9t_s0_t20", FAST_SET, "detect"), "arc8": ("ring_b8_s5_t20", FAST_SET, "detect"),
    "arc10": ("ring_b9_s0_t20", FAST_SET, "detect"), "no_wrap": ("ring_b9_s8_t20", FAST_SET, "detect"),
    "no_dark": ("ring_d9_s0_t20", FAST_SET, "detect"), "no_bright": ("ring_b9_s0_t20", FAST_SET, "detect"),
    "sup_ge": ("dots_96x80", FAST_SET, "detect"), "sup_4": ("dots_96x80", FAST_SET, "detect"),
    "offband_kept": ("dots_96x80", FAST_SET, "detect"), "band_le": ("dots_96x80", FAST_SET, "detect"),
    "harris5": ("dots_96x80", SELECT_SET, "detect"), "harris_c_swapped": (None, FAST_SET + LATTICE_FEW, "detect"),
    "order_xy": ("dots_96x80", SELECT_SET, "detect"), "H_asc": ("grad_nf1039_inside", SELECT_SET, "detect"),
    "quota_after_merge": ("lat_8layers", ["lat_8layers"], "detect"), "cap_first": ("grad_cap1037_between", SELECT_SET, "detect"),
    "response_f32": ("dots_96x80", SELECT_SET, "detect"), "layer_no_round": ("layers_96x96", ["layers_96x96", "layers_97x91"], "layer"),
    "x1_unclamped": (None, ["layers_96x96", "layers_97x91"], "layer"), "layer_pos_trunc": ("lat_8layers", ["lat_8layers"], "describe"),
    "n0_zero": ("steer_flat", DESCRIBE_SET, "describe"), "square_patch": ("dots_96x80", DESCRIBE_SET, "describe"),
    "rnd_rint": ("steer_pp", DESCRIBE_SET, "describe"), "rnd_away": ("steer_pp", DESCRIBE_SET, "describe"),
    "rnd_trunc": ("steer_pp", DESCRIBE_SET, "describe"), "bit_le": ("steer_flat", DESCRIBE_SET, "describe"),
    "msb_first": ("steer_pp", DESCRIBE_SET, "describe")}
EQUIVALENT = {
    "harris_c_swapped": "c = sum Ix Iy is symmetric in its two factors and H = 25 (a b - c c) - (a + b)^2 is symmetric in (a, b): "
                        "exchanging Ix and Iy, in c alone or throughout, changes no H",
    "x1_unclamped": "the clamp acts only where the weight of x1 is 0 (test_the_clamp_acts_only_under_weight_zero)"}
LAYER_FRAMES = {name: img for name, img, _ in D.layer_frames()}


_plain = {}


def plain_detect(c):
    if c["name"] not in _plain:
        _plain[c["name"]] = O.detect(c["img"], c["params"], c["cap"])[0]
    return _plain[c["name"]]


def noticed(name, mut, what):
    if what == "layer":
        img = LAYER_FRAMES[name]
        return any(not np.array_equal(O.layer(img, l, mut), O.layer(img, l)) for l in range(1, 8))
    c = BY[name]
    if what == "detect":
        return K.same_keypoints(O.detect(c["img"], c["params"], c["cap"], mut=mut)[0], plain_detect(c)) is not None
    kp = c["kp"] if c["family"] == "steer" else ref_of(c)[0]
    pick = slice(None) if len(kp) <= 40 or name == "lat_8layers" else slice(0, 8)
    a = O.describe(c["img"], kp[pick], c["params"], c["pattern"], mut=mut)
    b = O.describe(c["img"], kp[pick], c["params"], c["pattern"])
    return K.same_keypoints(a[0], b[0]) is not None or D.same_descriptors(a[1], b[1]) is not None


def test_every_mutant_is_noticed_by_its_named_case_or_is_equivalent():
    assert set(MUTANT_TABLE) == set(O.MUTANTS)
    t = time.time()
    lines = []
    for mut in O.MUTANTS:
        named, tried, what = MUTANT_TABLE[mut]
        hits = [n for n in tried if noticed(n, mut, what)]
        if named is None:
            assert not hits and mut in EQUIVALENT, (mut, hits[:3])
            lines.append("%-18s %-24s equivalent (0 of %d): %s" % (mut, "-", len(tried), EQUIVALENT[mut]))
        else:
            assert named in tried and named in hits, (mut, named, hits[:5])
            lines.append("%-18s %-24s noticed by %d of %d cases" % (mut, named, len(hits), len(tried)))
    print()
    print("\n".join(lines))
    print("mutant table: %.1f s; the file so far: %.1f s" % (time.time() - t, time.time() - T0))
