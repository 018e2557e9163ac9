"""The designed ORB catalogue (tests/test_orb_designed_cpu.py, tests/test_gpu_orb_designed.py): a helper module, not a test.

Every case is a u8 frame, the ORB parameters, a capacity and a sampling pattern, the classes of decisions it is built to reach,
and an expectation that does NOT come from tests/orb_ref.py.  Three kinds of expectation, named in each case's `source`:

  literal     score maps, key-point positions and bits written down (rings, dots, the plain lattice, the flat patch)
  arithmetic  a few lines over the dot positions: which dot survives (dot_rule), the Harris measure of a lattice dot from its own
              and its 8 neighbours' amplitudes (lattice_H), the order by a lexsort over (-H, y, x), the plain lattice's descriptor
  hand_*      the contract of include/uwt.h read once more, pixel by pixel in scalar loops (hand_score, hand_harris,
              hand_direction, hand_descriptor): slow, used on the small frames only, and itself held to the literals above

What is taken from orb_ref on purpose (`from_ref` names it; the CPU test compares nothing there, the device is compared with
orb_ref): the whole 8-layer lattice, the direction and descriptor of the graded and the half lattice's key points (their positions, order
and responses are arithmetic), the noise pair, the layer pixels beyond the hand-picked ones.  orb_ref is imported for its constants and for
default_pattern(), which is data of the contract (the library's copy is compared with it elsewhere)."""
import math

import numpy as np

import orb_ref as O

F32 = np.float32
E, T = 16, 20                      # edge and FAST threshold of the whole-call cases
LATTICE_W, LATTICE_H = 256, 240
LATTICE_N = 2912                   # 56 x 52 dots inside the band of edge 16
H_PLAIN = 21504 * 255 ** 4         # 21 (32 v^2)^2: lattice_H with nine equal amplitudes = 90 924 301 440 000

CLASSES = (
    ["arc9", "arc8", "bright", "dark", "score_t1", "score_t", "thr0", "thr255"] + ["wrap_%d" % i for i in range(8, 16)]
    + ["eq_%s" % d for d in ("n", "ne", "e", "se", "s", "sw", "w", "nw")] + ["tile_lr", "tile_tb", "tile_corner", "off_band_neighbour"]
    + ["band_first_col", "band_last_col", "band_first_row", "band_last_row", "outside_first_col", "outside_last_col",
       "outside_first_row", "outside_last_row"]
    + ["raw_le_1024", "raw_1025_2048", "raw_gt_2048", "raw_not_multiple", "quota_list_minus1", "quota_eq_list", "quota_list_plus1",
       "quota_cuts_tie", "kept_gt_1024", "cap_lt_kept_gt_1024", "cap_eq_kept"]
    + ["n0", "c_half", "c_zero", "tie_pos", "tie_neg", "equal_intensities", "layer_half"])
# Not in the list: "clamped last column / row".  x1 = min(x0 + 1, w - 1) acts only where x0 = w - 1, and for a layer narrower than
# the frame x0 <= w - 2 everywhere (test_the_clamp_acts_only_under_weight_zero); where w_l = w the weight of x1 is 0.
UNREACHABLE = ["layer_clamp"]


def params(**over):
    p = dict(n_features=500, n_levels=1, edge_threshold=E, fast_threshold=T, upright=0)
    p.update(over)
    return p


# ---- the contract once more, in scalar loops ------------------------------------------------------------------------------------
def hand_score(img, x, y):
    """the raw FAST score of a pixel (before the threshold): max over the 16 arcs of 9 of the arc's smallest step up or down"""
    p = int(img[y, x])
    d = [int(img[y + dy, x + dx]) - p for dx, dy in O.RING]
    best = -256
    for i in range(16):
        arc = [d[(i + j) % 16] for j in range(9)]
        best = max(best, min(arc), min(-v for v in arc))
    return best


def hand_score_map(img, e, t):
    h, w = img.shape
    S = np.zeros((h, w), np.int32)
    for y in range(e, h - e):
        for x in range(e, w - e):
            win = img[y - 3:y + 4, x - 3:x + 4]
            if win.min() == win.max():      # a flat neighbourhood scores 0
                continue
            s = hand_score(img, x, y)
            if s > t:
                S[y, x] = s
    return S


def hand_kept(S):
    """(x, y) of the scores strictly above all 8 neighbours, row by row"""
    h, w = S.shape
    out = []
    for y, x in zip(*np.nonzero(S)):
        nb = [S[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and 0 <= y + dy < h and 0 <= x + dx < w]
        if all(S[y, x] > v for v in nb):
            out.append((int(x), int(y)))
    return out


def hand_harris(img, x, y):
    a = b = c = 0
    I = lambda yy, xx: int(img[yy, xx])
    for v in range(y - 3, y + 4):
        for u in range(x - 3, x + 4):
            ix = 2 * (I(v, u + 1) - I(v, u - 1)) + (I(v - 1, u + 1) - I(v - 1, u - 1)) + (I(v + 1, u + 1) - I(v + 1, u - 1))
            iy = 2 * (I(v + 1, u) - I(v - 1, u)) + (I(v + 1, u - 1) - I(v - 1, u - 1)) + (I(v + 1, u + 1) - I(v - 1, u + 1))
            a, b, c = a + ix * ix, b + iy * iy, c + ix * iy
    return 25 * (a * b - c * c) - (a + b) * (a + b)


def hand_moments(img, gx, gy):
    m10 = m01 = 0
    for v in range(-15, 16):
        for u in range(-O.UMAX[abs(v)], O.UMAX[abs(v)] + 1):
            m10 += u * int(img[gy + v, gx + u])
            m01 += v * int(img[gy + v, gx + u])
    return m10, m01


def hand_direction(img, gx, gy):
    m10, m01 = hand_moments(img, gx, gy)
    fx, fy = F32(m10), F32(m01)
    n = F32(np.sqrt(F32(F32(fx * fx) + F32(fy * fy))))
    return (F32(1.0), F32(0.0)) if n == 0 else (F32(fx / n), F32(fy / n))


def hand_coordinates(c, s, pattern):
    """the f32 values that are rounded, [256, 4]: x0 c - y0 s, x0 s + y0 c, x1 c - y1 s, x1 s + y1 c"""
    out = np.zeros((256, 4), np.float32)
    for k in range(256):
        x0, y0, x1, y1 = (F32(int(v)) for v in pattern[k])
        out[k] = (F32(F32(x0 * c) - F32(y0 * s)), F32(F32(x0 * s) + F32(y0 * c)), F32(F32(x1 * c) - F32(y1 * s)), F32(F32(x1 * s) + F32(y1 * c)))
    return out


def hand_descriptor(img, gx, gy, c, s, pattern):
    co = hand_coordinates(c, s, pattern)
    out = [0] * 32
    for k in range(256):
        px0, py0, px1, py1 = (int(math.floor(float(F32(v + F32(0.5))))) for v in co[k])
        if int(img[gy + py0, gx + px0]) < int(img[gy + py1, gx + px1]):
            out[k // 8] |= 1 << (k % 8)
    return np.array(out, np.uint8)


def hand_records(rows):
    """(level, gy, gx, H) -> KEYPOINT records with direction (1, 0)"""
    k = np.zeros(len(rows), O.KEYPOINT)
    for i, (l, gy, gx, H) in enumerate(rows):
        k[i] = (F32(gx * 6 ** l / 5 ** l), F32(gy * 6 ** l / 5 ** l), F32(31 * 6 ** l / 5 ** l), F32(H / (25.0 * 7140.0 ** 4)), 1.0, 0.0, l, 0)
    return k


def hand_select(cands, quota, cap):
    """one layer: cands (gy, gx, H) -> the quota best by (H descending, y, x), in (y, x) order, then the capacity cut"""
    best = sorted(cands, key=lambda r: (-r[2], r[0], r[1]))[:quota]
    rows = sorted(best, key=lambda r: (r[0], r[1]))
    if len(rows) > cap:
        keep = sorted(rows, key=lambda r: (-r[2], r[0], r[1]))[:cap]
        rows = sorted(keep, key=lambda r: (r[0], r[1]))
    return [(0, gy, gx, H) for gy, gx, H in rows]


def hand_whole(img, p, cap, pattern, kept_xy=None):
    """the whole call on a small one-layer frame by the hand_* loops; kept_xy: the suppressed corners where a literal gives them"""
    assert p["n_levels"] == 1
    if kept_xy is None:
        kept_xy = hand_kept(hand_score_map(img, p["edge_threshold"], p["fast_threshold"]))
    rows = hand_select([(y, x, hand_harris(img, x, y)) for x, y in kept_xy], p["n_features"], cap)
    k = hand_records(rows)
    return hand_describe(img, k, p, pattern)


def hand_describe(img, k, p, pattern):
    k = k.copy()
    pat = O.default_pattern() if pattern is None else pattern
    d = np.zeros((len(k), 32), np.uint8)
    for i in range(len(k)):
        gx, gy = int(k[i]["x"]), int(k[i]["y"])                  # (layer 0: the position is the coordinate)
        c, s = (F32(1.0), F32(0.0)) if p["upright"] else hand_direction(img, gx, gy)
        k[i]["dir_x"], k[i]["dir_y"] = c, s
        d[i] = hand_descriptor(img, gx, gy, c, s, pat)
    return k, d


# ---- rings ---------------------------------------------------------------------------------------------------------------------
RING_C = (32, 32)
RING_KINDS = ("9", "8", "9t")      # an arc of exactly 9 at centre +- (T + 1); of exactly 8; of 9 with its middle pixel at centre +- T
RING_RAW = {"9": T + 1, "8": 1, "9t": T}   # the raw score at the centre, written out: what is left of the ring steps by 1 only


def ring_frame(start, bright, kind, w=64, h=64):
    """Background 100 and a centre one below it (bright) or above it (dark), so that no pixel but the centre sees a step above T:
    the painted arc is T + 1 from the centre and T from the background."""
    sign = 1 if bright else -1
    img = np.full((h, w), 100, np.uint8)
    cx, cy = RING_C
    centre = 100 - sign
    img[cy, cx] = centre
    n = 8 if kind == "8" else 9
    for j in range(n):
        dx, dy = O.RING[(start + j) % 16]
        img[cy + dy, cx + dx] = centre + sign * (T if kind == "9t" and j == 4 else T + 1)
    return img


def ring_cases():
    out = []
    for thr in (T, 0, 255):
        for bright in (True, False):
            for kind in RING_KINDS:
                for start in range(16):
                    img = ring_frame(start, bright, kind)
                    raw = RING_RAW[kind]
                    cls = {"bright" if bright else "dark"}
                    if thr != T:
                        cls.add("thr%d" % thr)
                    elif kind == "9":
                        cls |= {"arc9", "score_t1"} | ({"wrap_%d" % start} if start >= 8 else set())
                    else:
                        cls.add("arc8" if kind == "8" else "score_t")
                    c = dict(name="ring_%s%s_s%d_t%d" % ("b" if bright else "d", kind, start, thr), family="rings", img=img,
                             params=params(fast_threshold=thr), cap=64, pattern=None, classes=cls, centre_raw=raw)
                    if thr == T:       # literal: the centre alone scores, and only under an arc of exactly 9
                        c["source"] = "literal"
                        c["scores"] = {RING_C: raw} if raw > thr else {}
                        c["kept"] = [RING_C] if raw > thr else []
                    elif thr == 255:   # literal: no score exceeds 255
                        c["source"] = "literal"
                        c["scores"], c["kept"] = {}, []
                    else:              # under 0 every step scores: the map by hand_score, the centre's entry a literal
                        c["source"] = "hand"
                        c["centre_score"] = raw
                    out.append(c)
    return out


# ---- dots and pairs ------------------------------------------------------------------------------------------------------------
# (x, y, value) on background 0.  A single pixel of value v scores v (its ring is 0: the dark arcs) and no other pixel scores
# (a pixel of value 0 never has 9 contiguous ring pixels on dots): the score map is the dots themselves, inside the band.
DOTS_96 = [
    # single dots one step outside / on the band's first and last column and row, and on its four corners
    (15, 20, 200), (16, 28, 201), (79, 20, 202), (80, 28, 203), (24, 15, 204), (32, 16, 205), (24, 63, 206), (32, 64, 207),
    (16, 16, 210), (79, 16, 211), (16, 63, 212), (79, 63, 213),
    # equal pairs inside tile (0, 0): horizontal, vertical, both diagonals — all suppressed
    (24, 36, 100), (25, 36, 100), (31, 36, 100), (31, 37, 100), (37, 36, 100), (38, 37, 100), (43, 37, 100), (44, 36, 100),
    # v against v - 1 inside the tile: the stronger is kept
    (24, 42, 100), (25, 42, 99), (31, 42, 100), (31, 43, 99), (37, 42, 100), (38, 43, 99), (43, 43, 100), (44, 42, 99),
    # across x = 47 | 48
    (47, 20, 100), (48, 20, 100), (47, 24, 100), (48, 24, 99), (47, 28, 99), (48, 28, 100), (47, 32, 100), (48, 33, 100),
    # across y = 47 | 48
    (54, 47, 100), (54, 48, 100), (58, 47, 100), (58, 48, 99), (62, 47, 99), (62, 48, 100), (66, 47, 100), (67, 48, 100),
    # the meeting point of four tiles: one pixel in each
    (47, 47, 100), (48, 48, 100), (48, 47, 99), (47, 48, 98),
    # equal pairs straddling the band's edges: the pixel inside survives, the score off the band is 0
    (15, 40, 150), (16, 40, 150), (72, 15, 150), (72, 16, 150), (79, 40, 150), (80, 40, 150), (72, 63, 150), (72, 64, 150)]
# 128 x 96 at edge 31: the band is 66 x 34, tiles of 32 leave a partial last tile of 2 columns (x = 95, 96) and of 2 rows (y = 63, 64)
DOTS_128 = [
    (30, 36, 200), (31, 44, 201), (96, 36, 202), (97, 44, 203), (40, 30, 204), (48, 31, 205), (36, 64, 206), (44, 65, 207),
    (31, 31, 210), (96, 31, 211), (31, 64, 212), (96, 64, 213),
    (62, 36, 100), (63, 36, 100), (62, 40, 100), (63, 40, 99), (62, 44, 99), (63, 44, 100), (62, 48, 100), (63, 49, 100),
    (94, 40, 100), (95, 40, 100), (94, 44, 100), (95, 44, 99), (94, 48, 99), (95, 48, 100), (94, 52, 100), (95, 53, 100),
    (52, 62, 100), (52, 63, 100), (56, 62, 100), (56, 63, 99), (70, 62, 99), (70, 63, 100), (74, 62, 100), (75, 63, 100),
    (62, 62, 100), (63, 63, 100), (63, 62, 99), (62, 63, 98),
    (30, 52, 150), (31, 52, 150), (84, 30, 150), (84, 31, 150)]


def dot_frame(dots, w, h):
    img = np.zeros((h, w), np.uint8)
    for x, y, v in dots:
        img[y, x] = v
    return img


def dot_rule(dots, w, h, e, t):
    """(scores {(x, y): v}, kept [(x, y)] row by row): a dot scores its value inside the band; it is kept iff that exceeds T and
    every dot beside it INSIDE THE BAND is weaker"""
    inside = {(x, y): v for x, y, v in dots if e <= x < w - e and e <= y < h - e and v > t}
    kept = [(x, y) for (x, y), v in inside.items()
            if all(inside.get((x + dx, y + dy), 0) < v for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)]
    return inside, sorted(kept, key=lambda q: (q[1], q[0]))


# what the rule gives, written out once more as literals (kept dots, row by row)
KEPT_96 = [(32, 16), (16, 16), (72, 16), (79, 16), (79, 20), (47, 24), (16, 28), (48, 28), (16, 40), (79, 40), (24, 42), (31, 42),
           (37, 42), (43, 43), (58, 47), (62, 48), (16, 63), (24, 63), (72, 63), (79, 63)]
KEPT_128 = [(31, 31), (48, 31), (84, 31), (96, 31), (96, 36), (62, 40), (31, 44), (63, 44), (94, 44), (95, 48), (31, 52), (56, 62),
            (70, 63), (31, 64), (36, 64), (96, 64)]


def dot_cases():
    out = []
    eq = {"eq_%s" % d for d in ("n", "ne", "e", "se", "s", "sw", "w", "nw")}
    band = {"band_first_col", "band_last_col", "band_first_row", "band_last_row", "outside_first_col", "outside_last_col",
            "outside_first_row", "outside_last_row", "off_band_neighbour"}
    for name, dots, w, h, e, literal in (("dots_96x80", DOTS_96, 96, 80, E, KEPT_96), ("dots_128x96", DOTS_128, 128, 96, 31, KEPT_128)):
        scores, kept = dot_rule(dots, w, h, e, T)
        out.append(dict(name=name, family="dots", img=dot_frame(dots, w, h), params=params(edge_threshold=e), cap=64, pattern=None,
                        classes=(eq if name == "dots_96x80" else eq - {"eq_ne", "eq_sw"}) | band | {"tile_lr", "tile_tb", "tile_corner", "raw_le_1024", "equal_intensities"},
                        source="literal", scores=scores, kept=kept, kept_literal=sorted(literal, key=lambda q: (q[1], q[0])), dots=dots))
    return out


# ---- the lattice ---------------------------------------------------------------------------------------------------------------
def lattice_amplitudes(kind):
    """amplitude of dot (row, col) of img[2::4, 2::4], 60 x 64 dots: "plain" 255, "graded" 40 + (64 row + col) mod 200, "half" 255 on
    the first 32 rows of dots and nothing below (1568 dots inside the band)"""
    r, c = np.mgrid[0:LATTICE_H // 4, 0:LATTICE_W // 4]
    return {"plain": np.full(r.shape, 255), "graded": 40 + (64 * r + c) % 200, "half": np.where(r < 32, 255, 0)}[kind].astype(np.int64)


def lattice_frame(kind="plain"):
    img = np.zeros((LATTICE_H, LATTICE_W), np.uint8)
    img[2::4, 2::4] = lattice_amplitudes(kind)
    return img


def lattice_H(A):
    """H of every dot that has its 8 neighbours, from the amplitudes alone.  The Sobel support of a dot is its 3 x 3; dots are 4
    apart, so the supports are disjoint and the 7 x 7 block around a dot holds its own support (sum Ix^2 = sum Iy^2 = 12 A^2, sum
    Ix Iy = 0), one column of each horizontal neighbour's (Ix^2: 6, Iy^2: 2, Ix Iy: 0), one row of each vertical neighbour's
    (2, 6, 0) and one pixel of each diagonal neighbour's (1, 1, +1 on the main diagonal, -1 on the other)."""
    q = A.astype(np.int64) ** 2
    c, l, r, u, d = q[1:-1, 1:-1], q[1:-1, :-2], q[1:-1, 2:], q[:-2, 1:-1], q[2:, 1:-1]
    ul, ur, dl, dr = q[:-2, :-2], q[:-2, 2:], q[2:, :-2], q[2:, 2:]
    diag = ul + ur + dl + dr
    a = 12 * c + 6 * (l + r) + 2 * (u + d) + diag
    b = 12 * c + 2 * (l + r) + 6 * (u + d) + diag
    cc = ul + dr - ur - dl
    H = np.zeros(A.shape, np.int64)
    H[1:-1, 1:-1] = 25 * (a * b - cc * cc) - (a + b) * (a + b)
    return H


def lattice_candidates(kind):
    """(gy, gx, H) of the dots inside the band, row by row: every one a corner of score A > T whose neighbours score 0"""
    A = lattice_amplitudes(kind)
    H = lattice_H(A)
    out = []
    for r in range(H.shape[0]):
        for c in range(H.shape[1]):
            x, y = 4 * c + 2, 4 * r + 2
            if A[r, c] > T and E <= x < LATTICE_W - E and E <= y < LATTICE_H - E:
                out.append((y, x, int(H[r, c])))
    return out


def lattice_bits(pattern):
    """the plain lattice's descriptor: the direction is (1, 0) (the patch is symmetric about every dot: both moments are 0), the
    sampled offsets are the pattern's own, and an offset holds 255 iff both coordinates are multiples of 4"""
    dot = lambda x, y: x % 4 == 0 and y % 4 == 0
    out = [0] * 32
    for k, (x0, y0, x1, y1) in enumerate(np.asarray(pattern, np.int64)):
        if not dot(x0, y0) and dot(x1, y1):
            out[k // 8] |= 1 << (k % 8)
    return np.array(out, np.uint8)


_lat = {}


def lattice_expect(kind, n_features, cap):
    """(records with direction (1, 0), rows): arithmetic only"""
    if kind not in _lat:
        _lat[kind] = lattice_candidates(kind)
    cand = _lat[kind]
    if kind == "plain":      # every H equal: the order is the row-major one and no sort is needed — written so on purpose
        assert all(r[2] == H_PLAIN for r in cand) and len(cand) == LATTICE_N
        rows = [(0, y, x, H) for y, x, H in cand[:min(n_features, cap, LATTICE_N)]]
    else:
        ys, xs, Hs = (np.array(v, np.int64) for v in zip(*cand))
        best = np.sort(np.lexsort((xs, ys, -Hs))[:n_features])          # (cand is row-major: an index is a place)
        if len(best) > cap:
            best = np.sort(best[np.lexsort((xs[best], ys[best], -Hs[best]))[:cap]])
        rows = [(0, int(ys[i]), int(xs[i]), int(Hs[i])) for i in best]
    return hand_records(rows), rows


def graded_cuts():
    """quotas and caps of the graded lattice: just past 1024, (between two blocks of equal H, inside the next block), and past 2048"""
    H = np.sort(np.array([r[2] for r in lattice_candidates("graded")], np.int64))[::-1]
    edge = [i for i in range(1, len(H)) if H[i] != H[i - 1]]                      # a block of equal H ends before each
    b1 = next(i for i in edge if i > 1024)
    b2 = next(i for i in edge if i > 2048)
    inside = lambda b: b + 2
    assert H[b1 - 1] != H[b1] and H[inside(b1) - 1] == H[inside(b1)] and H[inside(b2) - 1] == H[inside(b2)]
    return [("between", b1), ("inside", inside(b1)), ("inside", inside(b2)), ("between", edge[0])]


def lattice_cases():
    out = []
    plain, graded = lattice_frame("plain"), lattice_frame("graded")

    def size_classes(nf, cap, n=LATTICE_N):
        kept = min(nf, n)
        cls = {"raw_gt_2048", "raw_not_multiple"}
        cls |= {"quota_list_minus1"} if nf == n - 1 else {"quota_eq_list"} if nf == n else {"quota_list_plus1"} if nf == n + 1 else set()
        if kept > 1024:
            cls.add("kept_gt_1024")
            if cap < kept:
                cls.add("cap_lt_kept_gt_1024")
        if cap == kept:
            cls.add("cap_eq_kept")
        return cls

    for nf in (1, 1023, 1024, 1025, 2911, 2912, 2913, 65536):
        out.append(dict(name="lat_nf%d" % nf, family="lattice", img=plain, params=params(n_features=nf), cap=4096, pattern=None,
                        classes=size_classes(nf, 4096) | {"n0", "equal_intensities"} | ({"quota_cuts_tie"} if nf < LATTICE_N else set()),
                        source="arithmetic", kind="plain"))
    for cap in (1, 1024, 1025, 2911, 2912):
        out.append(dict(name="lat_cap%d" % cap, family="lattice", img=plain, params=params(n_features=65536), cap=cap, pattern=None,
                        classes=size_classes(65536, cap) | {"n0"}, source="arithmetic", kind="plain"))
    for kind, q in graded_cuts():
        out.append(dict(name="grad_nf%d_%s" % (q, kind), family="lattice", img=graded, params=params(n_features=q), cap=4096, pattern=None,
                        classes=size_classes(q, 4096) | ({"quota_cuts_tie"} if kind == "inside" else set()), source="arithmetic",
                        kind="graded", from_ref="direction and descriptor"))
        out.append(dict(name="grad_cap%d_%s" % (q, kind), family="lattice", img=graded, params=params(n_features=65536), cap=q, pattern=None,
                        classes=size_classes(65536, q), source="arithmetic", kind="graded", from_ref="direction and descriptor"))
    out.append(dict(name="lat_half", family="lattice", img=lattice_frame("half"), params=params(n_features=65536), cap=4096, pattern=None,
                    classes={"raw_1025_2048", "raw_not_multiple", "kept_gt_1024"},
                    source="arithmetic", kind="half", from_ref="direction and descriptor"))
    out.append(dict(name="lat_8layers", family="lattice8", img=plain, params=params(n_levels=8), cap=4096, pattern=None,
                    classes={"raw_gt_2048", "raw_1025_2048", "raw_le_1024", "raw_not_multiple"}, source="orb_ref", from_ref="everything"))
    return out


def ring_frame_256(start=11):
    return ring_frame(start, True, "9", LATTICE_W, LATTICE_H)


def batch_frames():
    """{flat, lattice, ring, lattice} of one size, and their expectations under n_features 65536, cap 4096: (name, frame, kept (x, y))"""
    return [("flat", np.full((LATTICE_H, LATTICE_W), 77, np.uint8), []), ("lattice", lattice_frame("plain"), None),
            ("ring", ring_frame_256(), [RING_C]), ("lattice", lattice_frame("plain"), None)]


# ---- the steered half ----------------------------------------------------------------------------------------------------------
STEER_C = (32, 32)
STEER_PIXELS = [(11, 0, 255), (1, 0, 106), (0, 14, 255), (0, 8, 184)]     # (u, v, I): m10 = 2911, m01 = 5042
C_HALF, S_HALF = F32(0.5), F32(0.86602545)                                 # sqrtf(2911^2 + 5042^2) = 5822 = 2 * 2911 in f32
TIE_X0 = (1, -1, 3, -3, 5, -5, 7, -7, 9, -9, 11, -11, 13, -13)


def steer_pattern():
    """valid; entries 0..13 are (x0, 0, ..) with x0 odd of both signs — x0 * 0.5f is k + 0.5 — entries 14..27 are (0, y0, ..)
    likewise for the variant whose sine is the half; the second points and the other entries are the default's"""
    p = O.default_pattern().copy()
    for k, v in enumerate(TIE_X0):
        p[k, 0], p[k, 1] = v, 0
        p[14 + k, 0], p[14 + k, 1] = 0, v
    assert all((p[k, 0], p[k, 1]) != (p[k, 2], p[k, 3]) for k in range(256))
    return p


def symmetric_texture(seed, kind):
    """64 x 64, values 0..100; "point": T(u, v) = T(-u, -v) about (32, 32) over u, v in -31..31; "mirror": T(u, v) = T(-u, v)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 101, (63, 63))
    if kind == "point":
        f = a.reshape(-1)
        f[63 * 63 // 2 + 1:] = f[:63 * 63 // 2][::-1]
    else:
        a[:, 32:] = a[:, :31][:, ::-1]
    img = np.zeros((64, 64), np.uint8)
    img[1:, 1:] = a
    return img


def steer_frame(variant):
    """the four pixels over a point-symmetric texture (which adds nothing to either moment); variant: (sign of u, sign of v, swap)"""
    su, sv, swap = variant
    img = symmetric_texture(7, "point")
    cx, cy = STEER_C
    px = [((v, u, i) if swap else (su * u, sv * v, i)) for u, v, i in STEER_PIXELS]
    for u, v, i in px:
        assert abs(u) <= O.UMAX[abs(v)]
        img[cy + v, cx + u] = img[cy - v, cx - u] = 0
    for u, v, i in px:
        img[cy + v, cx + u] = i
    return img


STEER_VARIANTS = {"steer_pp": ((1, 1, False), (2911, 5042), (C_HALF, S_HALF)), "steer_np": ((-1, 1, False), (-2911, 5042), (-C_HALF, S_HALF)),
                  "steer_pn": ((1, -1, False), (2911, -5042), (C_HALF, -S_HALF)), "steer_swap": ((1, 1, True), (5042, 2911), (S_HALF, C_HALF))}


def steer_cases():
    """describe-only cases: a provided key point at (32, 32)"""
    kp = np.zeros(1, O.KEYPOINT)
    kp[0] = (32.0, 32.0, 31.0, 0.25, -3.0, 9.0, 0, 7)   # direction in: nonsense; response and laplacian pass through
    pat = steer_pattern()
    out = []
    for name, (variant, moments, direction) in STEER_VARIANTS.items():
        out.append(dict(name=name, family="steer", img=steer_frame(variant), params=params(), cap=4, pattern=pat, kp=kp, moments=moments,
                        direction=direction, classes={"c_half", "tie_pos", "tie_neg"} if name != "steer_swap" else {"tie_pos", "tie_neg"},
                        source="literal direction, hand_descriptor"))
    out.append(dict(name="steer_upright", family="steer", img=steer_frame((1, 1, False)), params=params(upright=1), cap=4, pattern=pat, kp=kp,
                    moments=None, direction=(F32(1.0), F32(0.0)), classes=set(), source="literal direction, hand_descriptor"))
    out.append(dict(name="steer_flat", family="steer", img=np.full((64, 64), 93, np.uint8), params=params(), cap=4, pattern=pat, kp=kp,
                    moments=(0, 0), direction=(F32(1.0), F32(0.0)), bits=np.zeros(32, np.uint8), classes={"n0", "equal_intensities"},
                    source="literal"))
    mirror = symmetric_texture(9, "mirror")
    out.append(dict(name="steer_mirror", family="steer", img=mirror, params=params(), cap=4, pattern=pat, kp=kp, moments=None,
                    direction=None, classes={"c_zero"}, source="c = 0 literal, hand_direction, hand_descriptor"))
    return out


# ---- layers --------------------------------------------------------------------------------------------------------------------
# 96 -> 80: destination x has N = 192 x + 16 over 160, so x = 2 (mod 5) has fx = 1024 exactly, from source column 2 + 6 (x - 2) / 5;
# the same along y.  There the value is (a + b + c + d + 2) >> 2 of the 2 x 2 source cell: a cell sum of 2 (mod 4) is the exact half.
LAYER_CELLS = [((2, 2), (1, 0, 0, 0), 0), ((7, 2), (1, 1, 0, 0), 1), ((12, 2), (1, 1, 1, 0), 1), ((2, 7), (255, 255, 255, 254), 255),
               ((7, 7), (9, 10, 10, 9), 10), ((77, 77), (200, 201, 200, 201), 201), ((12, 7), (0, 0, 0, 2), 1)]


def layer_frames():
    """(name, frame, hand values {(x, y) of layer 1: value})"""
    rng = np.random.RandomState(3)
    a = rng.randint(0, 256, (96, 96)).astype(np.uint8)
    hand = {}
    for (x, y), cell, want in LAYER_CELLS:
        sx, sy = 2 + 6 * (x - 2) // 5, 2 + 6 * (y - 2) // 5
        a[sy, sx], a[sy, sx + 1], a[sy + 1, sx], a[sy + 1, sx + 1] = cell
        hand[(x, y)] = want
    b = rng.randint(0, 256, (91, 97)).astype(np.uint8)      # 97 -> 81: the remaining pixels against orb_ref
    return [("layers_96x96", a, hand), ("layers_97x91", b, {})]


# ---- a pair for the chained call ---------------------------------------------------------------------------------------------
# Every dot of the plain lattice has the same descriptor and the graded lattice repeats each of its 200 about 14 times: the nearest
# and the second nearest neighbour are equally far, the ratio test of the matcher refuses every match, and uwt_tracking_orb_batch
# ends at its minimum of matches.  What does pass the chain with more than 1024 key points is white noise against itself moved by
# three columns: 4718 raw candidates on layer 0 (five tiles of 1024, the last partly filled), a quota of 4096 cutting between
# distinct H, and 4027 symmetric matches (tests/test_orb_designed_cpu.py asserts the counts).  Against orb_ref only.
NOISE_FEATURES = 4096


def noise_pair():
    big = np.random.RandomState(33).randint(0, 256, (LATTICE_H, LATTICE_W + 4)).astype(np.uint8)
    return np.ascontiguousarray(big[:, :LATTICE_W]), np.ascontiguousarray(big[:, 3:LATTICE_W + 3])


def all_cases():
    return ring_cases() + dot_cases() + lattice_cases() + steer_cases()


def intrinsics(w, h):
    return (float(w), float(w), (w - 1) / 2.0, (h - 1) / 2.0)


# ---- the expectation of a case ---------------------------------------------------------------------------------------------------
_expect = {}


def expectation(c):
    """(key points, descriptors or None, full).  full: every field is derived here.  Not full: x, y, size, response, octave and
    laplacian are; dir_x, dir_y hold (1, 0) and the descriptors are None — the caller takes those from orb_ref (`from_ref`).
    None for the case that is compared with orb_ref alone."""
    if c["name"] in _expect:
        return _expect[c["name"]]
    fam = c["family"]
    if fam in ("rings", "dots"):
        out = hand_whole(c["img"], c["params"], c["cap"], c["pattern"], c.get("kept")) + (True,)
    elif fam == "lattice":
        k, _ = lattice_expect(c["kind"], c["params"]["n_features"], c["cap"])
        if c["kind"] == "plain":
            out = (k, np.tile(lattice_bits(O.default_pattern()), (len(k), 1)), True)
        else:
            out = (k, None, False)
    elif fam == "steer":
        k = c["kp"].copy()
        cx, cy = STEER_C
        cs = c["direction"] if c["direction"] is not None else hand_direction(c["img"], cx, cy)
        k["dir_x"], k["dir_y"] = cs
        bits = c["bits"] if "bits" in c else hand_descriptor(c["img"], cx, cy, cs[0], cs[1], c["pattern"])
        out = (k, bits[None, :], True)
    else:
        out = None
    _expect[c["name"]] = out
    return out


def same_descriptors(got, want):
    """descriptors compared as bytes (an empty list equals an empty list); a description of the first difference or None"""
    got, want = np.ascontiguousarray(got, np.uint8).reshape(-1, 32), np.ascontiguousarray(want, np.uint8).reshape(-1, 32)
    if got.shape != want.shape:
        return "shape: %r against %r" % (got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        return "descriptor %d of %d: %d bits differ (%d rows differ)" % (bad[0], len(got), int(np.unpackbits(got[bad[0]] ^ want[bad[0]]).sum()), bad.size)
    return None
