"""The ORB contract of include/uwt.h (uwt_orb_*) restated in numpy: a helper module, not a test.  Integers are exact (int64), every
f32 / f64 step is the one IEEE operation the contract names; tests compare the device with this as integers and bytes.

`mut` names ONE deliberate mistake (MUTANTS); tests/test_orb_designed_cpu.py shows that each is noticed by a named case of
tests/orb_designed_cases.py, or argues why none can.  With mut=None nothing here changes."""
import numpy as np

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("dir_x", "<f4"), ("dir_y", "<f4"),
                     ("octave", "<i4"), ("laplacian", "<i4")])
MAX_LEVELS = 8
PATCH = 31
MIN_EDGE, MAX_EDGE = 16, 1024
# the Bresenham ring of 16 at radius 3 (dx, dy), clockwise from the top
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
        (-2, -2), (-1, -3)]
# UWT_ORB_UMAX: the half-width of row |v| of the circular patch of radius 15
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
HARRIS_DEN = float(25 * 7140 ** 4)
PATTERN_SEED = 0x6F726221
F32 = np.float32
MUTANTS = ("fast_ge", "arc8", "arc10", "no_wrap", "no_dark", "no_bright", "sup_ge", "sup_4", "offband_kept", "band_le", "harris5",
           "harris_c_swapped", "order_xy", "H_asc", "quota_after_merge", "cap_first", "response_f32", "layer_no_round", "x1_unclamped",
           "layer_pos_trunc", "n0_zero", "square_patch", "rnd_rint", "rnd_away", "rnd_trunc", "bit_le", "msb_first")


def default_params():
    return dict(n_features=500, n_levels=8, edge_threshold=31, fast_threshold=20, upright=0)


def layer_dim(n, level):
    p6, p5 = 6 ** level, 5 ** level
    return (n * p5 + p6 // 2) // p6


def layer_size(w, h, level):
    return layer_dim(w, level), layer_dim(h, level)


def level_quota(n_features, n_levels):
    """uwt_orb_level_quota: doubles, + - * / and rint only"""
    factor = np.float64(1.0) / np.float64(1.2)
    fp = np.float64(1.0)
    for _ in range(n_levels):
        fp = fp * factor
    want = np.float64(n_features) * (np.float64(1.0) - factor) / (np.float64(1.0) - fp)
    out, total = [], 0
    for _ in range(n_levels - 1):
        n = int(np.rint(want))
        out.append(n)
        total += n
        want = want * factor
    out.append(max(n_features - total, 0))
    return out


def mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def default_pattern():
    """uwt_orb_default_pattern: 256 x (x0, y0, x1, y1) int8"""
    out = np.zeros((256, 4), np.int8)
    n = 0
    for k in range(256):
        while True:
            e = [((mix(PATTERN_SEED ^ mix(n + j)) * 21) >> 32) - 10 for j in range(4)]
            n += 4
            if (e[0], e[1]) != (e[2], e[3]):
                break
        out[k] = e
    return out


def pattern_ok(p):
    p = np.asarray(p, np.int64).reshape(256, 4)
    return bool(((p[:, 0] ** 2 + p[:, 1] ** 2 <= 225) & (p[:, 2] ** 2 + p[:, 3] ** 2 <= 225)).all())


def layer(img, level, mut=None):
    """layer `level` of the scale pyramid, from level 0 alone"""
    img = np.ascontiguousarray(img, np.uint8)
    if level == 0:
        return img
    h, w = img.shape
    lw, lh = layer_size(w, h, level)

    def axis(n, ln):
        d = np.arange(ln, dtype=np.int64)
        N = (2 * d + 1) * n - ln
        i0 = N // (2 * ln)
        f = ((N % (2 * ln)) * 2048) // (2 * ln)
        return i0, np.minimum(i0 + 1, n - 1), f

    x0, x1, fx = axis(w, lw)
    y0, y1, fy = axis(h, lh)
    I = img.astype(np.int64)
    wx0, wx1, wy0, wy1 = (2048 - fx)[None, :], fx[None, :], (2048 - fy)[:, None], fy[:, None]
    a01, a11 = I[y0][:, x1], I[y1][:, x1]
    if mut == "x1_unclamped":   # x0 + 1 read past the row's end: the first pixel of the next row (the last row: its own last pixel)
        flat, over = I.reshape(-1), (x0 + 1 > w - 1)[None, :]
        a01 = np.where(over, flat[np.minimum(y0[:, None] * w + x0[None, :] + 1, w * h - 1)], a01)
        a11 = np.where(over, flat[np.minimum(y1[:, None] * w + x0[None, :] + 1, w * h - 1)], a11)
    half = 0 if mut == "layer_no_round" else 1 << 21
    s = (I[y0][:, x0] * wx0 * wy0 + a01 * wx1 * wy0 + I[y1][:, x0] * wx0 * wy1 + a11 * wx1 * wy1 + half) >> 22
    return s.astype(np.uint8)


def fast_scores(L, edge, thr, mut=None):
    """the dense score map of a layer: 0 off the candidate band and for a non-corner"""
    h, w = L.shape
    S = np.zeros((h, w), np.int32)
    if w < 2 * edge + 1 or h < 2 * edge + 1:
        return S
    I = L.astype(np.int32)
    lo = 3 if mut == "offband_kept" else edge                      # (the mutant scores every pixel that has a ring)
    hy, hx = (h - lo, w - lo) if mut != "band_le" else (h - lo + 1, w - lo + 1)
    ys, xs = slice(lo, hy), slice(lo, hx)
    p = I[ys, xs]
    d = np.stack([I[lo + dy:hy + dy, lo + dx:hx + dx] - p for dx, dy in RING])
    bright = np.full(p.shape, -(1 << 20), np.int32)
    dark = bright.copy()
    length = {"arc8": 8, "arc10": 10}.get(mut, 9)
    for i in range(16):
        if mut == "no_wrap" and i + length > 16:
            continue
        arc = d[[(i + j) % 16 for j in range(length)]]
        bright = np.maximum(bright, arc.min(axis=0))
        dark = np.maximum(dark, (-arc).min(axis=0))
    sc = bright if mut == "no_dark" else dark if mut == "no_bright" else np.maximum(bright, dark)
    S[ys, xs] = np.where(sc >= thr if mut == "fast_ge" else sc > thr, sc, 0)
    return S


def suppress(S, mut=None):
    """(ys, xs) of the scores strictly greater than their 8 neighbours, row-major"""
    P = np.pad(S, 1)
    h, w = S.shape
    top = S > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy or dx) and not (mut == "sup_4" and dy and dx):
                n = P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                top &= (S >= n) if mut == "sup_ge" else (S > n)
    return np.nonzero(top)


def harris(L, ys, xs, mut=None):
    """H at the given pixels (each at least 4 from every border): int64"""
    I = L.astype(np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    a = np.zeros(len(ys), np.int64)
    b, c = a.copy(), a.copy()
    r = 2 if mut == "harris5" else 3
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y, x = ys + dy, xs + dx
            ix = 2 * (I[y, x + 1] - I[y, x - 1]) + (I[y - 1, x + 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y + 1, x - 1])
            iy = 2 * (I[y + 1, x] - I[y - 1, x]) + (I[y + 1, x - 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y - 1, x + 1])
            a += ix * ix
            b += iy * iy
            c += iy * ix if mut == "harris_c_swapped" else ix * iy
    return 25 * (a * b - c * c) - (a + b) * (a + b)


def layer_candidates(L, p, mut=None):
    """(ys, xs, H) of a layer's suppressed corners, row-major"""
    e = p["edge_threshold"]
    ys, xs = suppress(fast_scores(L, e, p["fast_threshold"], mut), mut)
    if mut == "offband_kept":   # (its candidates are still those of the band: only the scores around it differ)
        h, w = L.shape
        on = (ys >= e) & (ys < h - e) & (xs >= e) & (xs < w - e)
        ys, xs = ys[on], xs[on]
    return ys, xs, harris(L, ys, xs, mut)


def detect(img, p=None, cap=4096, layers=None, mut=None):
    """the key points of a frame, directions (1, 0): KEYPOINT records in contract order, and (level, gy, gx, H) int64 rows"""
    p = p or default_params()
    h, w = img.shape
    quota = level_quota(p["n_features"], p["n_levels"])
    rows = []
    for l in range(p["n_levels"]):
        L = layers[l] if layers is not None else layer(img, l, mut)
        ys, xs, H = layer_candidates(L, p, mut)
        Hs = H if mut == "H_asc" else -H
        order = np.lexsort((ys, xs, Hs) if mut == "order_xy" else (xs, ys, Hs))
        if mut != "quota_after_merge":
            order = order[:quota[l]]
        rows += [(l, int(ys[i]), int(xs[i]), int(H[i])) for i in order]
    place = (lambda r: (r[0], r[2], r[1])) if mut == "order_xy" else (lambda r: r[:3])
    if mut == "quota_after_merge":
        rows = sorted(rows, key=lambda r: (-r[3], place(r)))[:sum(quota)]
    rows.sort(key=place)
    if len(rows) > cap:
        if mut == "cap_first":
            keep = range(cap)
        else:
            keep = sorted(range(len(rows)), key=lambda i: (rows[i][3] if mut == "H_asc" else -rows[i][3], place(rows[i])))[:cap]
        rows = [rows[i] for i in sorted(keep)]
    k = np.zeros(len(rows), KEYPOINT)
    for i, (l, gy, gx, H) in enumerate(rows):
        p6, p5 = np.float64(6 ** l), np.float64(5 ** l)
        k[i]["x"] = F32(np.float64(gx * 6 ** l) / p5)
        k[i]["y"] = F32(np.float64(gy * 6 ** l) / p5)
        k[i]["size"] = F32(np.float64(PATCH * 6 ** l) / p5)
        k[i]["response"] = F32(H) / F32(HARRIS_DEN) if mut == "response_f32" else F32(np.float64(H) / np.float64(HARRIS_DEN))
        k[i]["dir_x"], k[i]["dir_y"], k[i]["octave"], k[i]["laplacian"] = 1.0, 0.0, l, 0
    return k, np.array(rows, np.int64).reshape(-1, 4)


def layer_pos(v, level, mut=None):
    """the layer position of a level-0 coordinate: rnd of the inverse scaling, in double"""
    if mut == "layer_pos_trunc":
        return int(np.float64(v) * np.float64(5 ** level) / np.float64(6 ** level))
    return int(np.floor(np.float64(v) * np.float64(5 ** level) / np.float64(6 ** level) + np.float64(0.5)))


def keypoint_ok(k, w, h, p):
    if not (np.isfinite(k["x"]) and np.isfinite(k["y"])) or abs(k["x"]) > 1e6 or abs(k["y"]) > 1e6:
        return False
    l = int(k["octave"])
    if l < 0 or l >= p["n_levels"]:
        return False
    lw, lh = layer_size(w, h, l)
    e = p["edge_threshold"]
    gx, gy = layer_pos(k["x"], l), layer_pos(k["y"], l)
    return e <= gx < lw - e and e <= gy < lh - e


def rnd(v, mut=None):
    if mut == "rnd_rint":
        return np.rint(v).astype(np.int64)
    if mut == "rnd_away":
        return (np.sign(v) * np.floor(np.abs(v) + F32(0.5))).astype(np.int64)
    if mut == "rnd_trunc":
        return np.trunc(v + F32(0.5)).astype(np.int64)
    return np.floor(v + F32(0.5)).astype(np.int64)


def describe(img, kp, p=None, pattern=None, layers=None, mut=None):
    """direction and descriptor at the records' layer positions: (records with directions, uint8 [n, 32])"""
    p = p or default_params()
    pat = (default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)).astype(np.float32)
    out = np.array(kp, KEYPOINT).reshape(-1)
    desc = np.zeros((len(out), 32), np.uint8)
    cache = {}
    for i in range(len(out)):
        l = int(out[i]["octave"])
        if l not in cache:
            cache[l] = (layers[l] if layers is not None else layer(img, l, mut)).astype(np.int64)
        I = cache[l]
        gx, gy = layer_pos(out[i]["x"], l, mut), layer_pos(out[i]["y"], l, mut)
        c, s = F32(1.0), F32(0.0)
        if not p["upright"]:
            m10 = m01 = 0
            for v in range(-15, 16):
                half = 15 if mut == "square_patch" else UMAX[abs(v)]
                u = np.arange(-half, half + 1)
                row = I[gy + v, gx + u]
                m10 += int((u * row).sum())
                m01 += int(v * row.sum())
            fx, fy = F32(m10), F32(m01)
            n = np.sqrt(F32(fx * fx) + F32(fy * fy), dtype=np.float32)
            if n != 0:
                c, s = F32(fx / n), F32(fy / n)
            elif mut == "n0_zero":
                c, s = F32(0.0), F32(0.0)
        out[i]["dir_x"], out[i]["dir_y"] = c, s
        px0 = rnd(F32(pat[:, 0] * c) - F32(pat[:, 1] * s), mut)
        py0 = rnd(F32(pat[:, 0] * s) + F32(pat[:, 1] * c), mut)
        px1 = rnd(F32(pat[:, 2] * c) - F32(pat[:, 3] * s), mut)
        py1 = rnd(F32(pat[:, 2] * s) + F32(pat[:, 3] * c), mut)
        a, b = I[gy + py0, gx + px0], I[gy + py1, gx + px1]
        bits = (a <= b) if mut == "bit_le" else (a < b)
        desc[i] = np.packbits(bits, bitorder="big" if mut == "msb_first" else "little")
    return out, desc


def detect_describe(img, p=None, cap=4096, pattern=None, mut=None):
    p = p or default_params()
    layers = [layer(img, l, mut) for l in range(p["n_levels"])]
    k, _ = detect(img, p, cap, layers, mut)
    return describe(img, k, p, pattern, layers, mut)
