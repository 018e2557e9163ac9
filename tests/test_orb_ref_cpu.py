"""The numpy restatement of the ORB contract (tests/orb_ref.py) against ground it cannot share a bug with: hand-made frames whose
corners are known, a score worked out by hand, the symmetry of the whole chain under a quarter turn, the closed forms of the layer
sizes and the quota, and the stated properties of the default pattern.  No device, no library."""
from fractions import Fraction

import numpy as np

import orb_cases as K
import orb_ref as O
import ransac_ref as R

ARITH_INDEPENDENT = True


def test_squares_give_corners_at_their_corners_only():
    img, boxes = K.squares()
    p = O.default_params()
    S = O.fast_scores(img, p["edge_threshold"], p["fast_threshold"])
    corners = [(x, y) for x0, y0, x1, y1 in boxes for x in (x0, x1) for y in (y0, y1)]
    for x, y in corners:
        assert S[y, x] > p["fast_threshold"], (x, y)
    ys, xs = np.nonzero(S)
    assert len(ys) >= len(corners)
    for y, x in zip(ys, xs):   # nothing on flat ground or along a straight edge: every corner pixel is within 2 of a square's corner
        assert min(max(abs(x - cx), abs(y - cy)) for cx, cy in corners) <= 2, (x, y)
    for x0, y0, x1, y1 in boxes:
        xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
        assert S[y0 - 1:y0 + 2, xm - 3:xm + 4].max() == 0 and S[ym - 3:ym + 4, x0 - 1:x0 + 2].max() == 0   # mid-edge
        assert S[ym, xm] == 0                                                                              # inside
    assert S[5, 5] == 0 and (O.fast_scores(K.flat(160, 96), 31, 20) == 0).all()


def test_score_of_a_hand_made_ring():
    d = [30, 40, 50, 35, 45, 60, 33, 31, 32, -5, -5, -5, -5, -5, -5, -5]
    img = np.full((7, 7), 100, np.uint8)
    for (dx, dy), v in zip(O.RING, d):
        img[3 + dy, 3 + dx] = 100 + v
    # one arc of nine brighter pixels, the weakest of them 30 above the centre; every dark arc holds a brighter pixel
    assert O.fast_scores(img, 3, 20)[3, 3] == 30
    assert O.fast_scores(img, 3, 29)[3, 3] == 30 and O.fast_scores(img, 3, 30)[3, 3] == 0   # a corner iff the score is ABOVE the threshold
    assert O.fast_scores((200 - img.astype(np.int64)).astype(np.uint8), 3, 20)[3, 3] == 30   # the same ring, dark
    assert np.count_nonzero(O.fast_scores(img, 3, 20)) == 1                                  # the band is the centre alone
    # eight in a row are not enough
    d8 = [30] * 8 + [-5] * 8
    img8 = np.full((7, 7), 100, np.uint8)
    for (dx, dy), v in zip(O.RING, d8):
        img8[3 + dy, 3 + dx] = 100 + v
    assert O.fast_scores(img8, 3, 20)[3, 3] == 0
    assert len(set(O.RING)) == 16 and all(dx * dx + dy * dy in (9, 10, 8) for dx, dy in O.RING)


def test_harris_of_a_hand_made_block():
    # a vertical step: Ix = 4 * 100 on the two columns beside the step, Iy = 0: a = 14 * 400^2, b = c = 0
    img = np.zeros((11, 11), np.uint8)
    img[:, 6:] = 100
    H = O.harris(img, [5], [5])[0]
    a = 14 * 400 * 400
    assert H == -a * a
    # a quarter-plane corner has both gradients: H is that of its transpose
    img2 = np.zeros((11, 11), np.uint8)
    img2[5:, 5:] = 100
    assert O.harris(img2, [5], [5])[0] == O.harris(np.ascontiguousarray(img2.T), [5], [5])[0] > 0
    assert 25 * 7140 ** 4 == O.HARRIS_DEN and int(O.HARRIS_DEN) % 256 == 0


def test_quarter_turn_moves_key_points_directions_and_bits_with_it():
    w, h = 120, 96
    img = K.texture(w, h, 7)
    rot = np.ascontiguousarray(np.rot90(img))    # rot[i, j] = img[j, w - 1 - i]: (x, y) -> (y, w - 1 - x), a vector (u, v) -> (v, -u)
    p = O.default_params()
    p.update(n_levels=1, n_features=5000)
    k0, rows0 = O.detect(img, p)
    k1, rows1 = O.detect(rot, p)
    assert len(k0) >= 10
    moved = sorted((0, w - 1 - gx, gy, H) for _, gy, gx, H in rows0.tolist())
    assert moved == sorted(tuple(r) for r in rows1.tolist())
    a, _ = O.describe(img, k0, p)
    b, _ = O.describe(rot, k1, p)
    at = {(int(k["x"]), int(k["y"])): k for k in b}
    for k in a:
        t = at[(int(k["y"]), w - 1 - int(k["x"]))]
        assert t["dir_x"] == k["dir_y"] and t["dir_y"] == -k["dir_x"]          # exactly a quarter turn
        assert abs(float(k["dir_x"]) ** 2 + float(k["dir_y"]) ** 2 - 1.0) < 1e-6
    # upright descriptors under the pattern turned the same way hold the same bits
    p["upright"] = 1
    pat = O.default_pattern().astype(np.int64)
    turned = np.stack([pat[:, 1], -pat[:, 0], pat[:, 3], -pat[:, 2]], 1).astype(np.int8)
    _, d0 = O.describe(img, k0, p, pat)
    _, d1 = O.describe(rot, k1, p, turned)
    row = {(int(k["x"]), int(k["y"])): i for i, k in enumerate(k1)}
    for i, k in enumerate(k0):
        assert d0[i].tobytes() == d1[row[(int(k["y"]), w - 1 - int(k["x"]))]].tobytes()
    assert len({d.tobytes() for d in d0}) > len(d0) // 2    # and they are not all alike


def test_layer_sizes_and_layers():
    for n in (1, 61, 62, 63, 91, 96, 97, 160, 240, 256, 479, 480, 640, 735, 16384):
        for l in range(8):
            assert O.layer_dim(n, l) == int(n * Fraction(5, 6) ** l + Fraction(1, 2))   # n / 1.2^l to the nearest, halves up
    assert [O.layer_size(160, 96, l)[1] for l in range(4)] == [96, 80, 67, 56]
    assert [O.layer_size(97, 91, l) for l in range(4)] == [(97, 91), (81, 76), (67, 63), (56, 53)]
    img = K.texture(97, 91, 11)
    assert O.layer(img, 0) is not None and np.array_equal(O.layer(img, 0), img)
    for l in range(1, 8):
        L = O.layer(img, l)
        assert L.shape == O.layer_size(97, 91, l)[::-1] and L.dtype == np.uint8
        # against bilinear interpolation in double at the pixel centres: the 11-bit weights and the rounding move a value by 1 at most
        h, w = img.shape
        ys = (np.arange(L.shape[0]) + 0.5) * h / L.shape[0] - 0.5
        xs = (np.arange(L.shape[1]) + 0.5) * w / L.shape[1] - 0.5
        y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
        fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        I = img.astype(np.float64)
        want = I[y0][:, x0] * (1 - fx) * (1 - fy) + I[y0][:, x1] * fx * (1 - fy) + I[y1][:, x0] * (1 - fx) * fy + I[y1][:, x1] * fx * fy
        assert np.abs(L.astype(np.float64) - want).max() <= 1.0, l
        assert (O.layer(K.flat(97, 91, 201), l) == 201).all()


def test_quota_is_the_geometric_split():
    assert O.level_quota(500, 8) == [109, 90, 75, 63, 52, 44, 36, 31]
    for nl in range(1, 9):
        for nf in list(range(8, 700)) + [1000, 2048, 4096, 65536]:
            q = O.level_quota(nf, nl)
            assert len(q) == nl and sum(q) == nf and min(q) >= 0, (nf, nl, q)
            for l in range(nl - 2):
                assert abs(q[l + 1] - q[l] / 1.2) <= 1.0, (nf, nl, q)
    # below 8 features the rounding of the first layers can overshoot by one: the only case
    over = [(nf, nl) for nf in range(1, 8) for nl in range(1, 9) if sum(O.level_quota(nf, nl)) != nf]
    assert over == [(7, 8)] and O.level_quota(7, 8) == [2, 1, 1, 1, 1, 1, 1, 0]


def test_default_pattern_and_patch_table():
    pat = O.default_pattern()
    assert pat.shape == (256, 4) and pat.dtype == np.int8
    assert O.pattern_ok(pat) and np.abs(pat).max() <= 10
    assert not ((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3])).any()          # no test compares a pixel with itself
    assert len({tuple(r) for r in pat.tolist()}) > 250                               # and the tests are not copies of each other
    assert all(O.mix(x) == R.mix(x) for x in (0, 1, 0x6F726221, 0xFFFFFFFF, 123456789))
    bad = pat.copy()
    bad[17] = (15, 1, 0, 0)
    assert not O.pattern_ok(bad)
    bad[17] = (9, 12, -12, -9)
    assert O.pattern_ok(bad)
    # the circular patch: symmetric under a quarter turn, inside radius 15.5, and its moments fit f32 exactly
    U = O.UMAX
    cells = {(u, v) for v in range(-15, 16) for u in range(-U[abs(v)], U[abs(v)] + 1)}
    assert {(v, -u) for u, v in cells} == cells
    assert all(u * u + v * v < 15.5 ** 2 + 1 for u, v in cells) and {(15, 0), (0, 15), (11, 10)} <= cells
    assert 255 * sum(abs(u) for u, _ in cells) < 1 << 24
