"""The numpy restatement of ObtainImageTransformed (tests/warp_image_ref.py) against itself: the literal loop and the winner form
agree, the stated deviations and the landing rule hold, and the integer blend is addWeighted's.  Nothing of the library runs here."""
import numpy as np

import warp_image_ref as WR

ARITH_INDEPENDENT = True   # no arithmetic set is involved


def random_table(rng, rows, cols, n, targets):
    """n rows whose warped positions fall on `targets` distinct pixels (heavy collisions), some outside the image"""
    tx = rng.integers(-2, cols + 2, targets).astype(np.float32)
    ty = rng.integers(-2, rows + 2, targets).astype(np.float32)
    pick = rng.integers(0, targets, n)
    pts = np.zeros((n, 4), np.float32)
    pts[:, 0] = rng.uniform(0, cols - 0.01, n)
    pts[:, 1] = rng.uniform(0, rows - 0.01, n)
    pts[:, 2:] = 1
    wp = np.zeros((n, 4), np.float32)
    wp[:, 0] = tx[pick] + rng.uniform(-0.49, 0.49, n).astype(np.float32)
    wp[:, 1] = ty[pick] + rng.uniform(-0.49, 0.49, n).astype(np.float32)
    return pts, wp


def both(original, pts, wp, fill):
    a, b = np.full(original.shape, fill, np.uint8), np.full(original.shape, fill, np.uint8)
    va = WR.obtain_image_transformed(original, pts, wp, a)
    vb, n_landed = WR.winner_form(original, pts, wp, b)
    return a, va, b, vb, n_landed


def test_loop_equals_winner_form_under_heavy_collisions():
    rng = np.random.default_rng(3)
    for rows, cols, n, targets in ((37, 53, 3000, 40), (12, 9, 500, 300), (61, 97, 6000, 700)):
        original = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        pts, wp = random_table(rng, rows, cols, n, targets)
        a, va, b, vb, n_landed = both(original, pts, wp, 7)
        assert np.array_equal(a, b) and np.array_equal(va, vb)
        assert n_landed > int(vb.sum()) > 0   # rows did lose to later rows
        assert not va[0].any() and not va[:, 0].any()   # row 0 and column 0 are never written
        assert (a[va == 0] == 7).all()   # pixels no row lands on keep what the output held


def test_the_last_row_in_table_order_wins():
    original = np.arange(30, dtype=np.uint8).reshape(5, 6)
    pts = np.array([[1, 1, 1, 1], [2, 2, 1, 1], [3, 3, 1, 1]], np.float32)
    wp = np.array([[4, 2, 1, 1], [4, 2, 1, 1], [4.4, 1.6, 1, 1]], np.float32)
    a, va, b, vb, n_landed = both(original, pts, wp, 0)
    assert a[2, 4] == original[3, 3] == b[2, 4] and n_landed == 3 and va.sum() == 1


def test_deviations_are_skipped():
    original = np.arange(30, dtype=np.uint8).reshape(5, 6) + 100
    good = [2.0, 2.0, 1, 1]
    pts = np.array([[6.0, 1, 1, 1], [1, 5.0, 1, 1], [-1.0, 1, 1, 1], [np.nan, 1, 1, 1], good, good, good, good, good, [-0.5, -0.9, 1, 1]],
                   np.float32)
    wp = np.array([[1, 1, 1, 1], [1, 2, 1, 1], [1, 3, 1, 1], [1, 4, 1, 1], [np.nan, 2, 1, 1], [2, np.inf, 1, 1], [3e9, 2, 1, 1],
                   [2, -2147483520.0, 1, 1], [2147483392.0, 1, 1, 1], [5, 4, 1, 1]], np.float32)
    a, va, b, vb, n_landed = both(original, pts, wp, 0)
    assert np.array_equal(a, b) and np.array_equal(va, vb)
    # only the last row lands: (int)-0.5 = (int)-0.9 = 0 reads original[0, 0]; 2147483392 = 2^31 - 256 converts and misses the image
    assert n_landed == 1 and va.sum() == 1 and a[4, 5] == original[0, 0]


def test_halves_round_away_from_zero():
    assert WR.c_round(2.5) == 3 and WR.c_round(0.5) == 1 and WR.c_round(0.49) == 0 and WR.c_round(-0.5) == -1 and WR.c_round(1.5) == 2
    original = np.full((6, 6), 9, np.uint8)
    pts = np.tile(np.array([[1, 1, 1, 1]], np.float32), (3, 1))
    wp = np.array([[2.5, 1.5, 1, 1], [0.5, 0.5, 1, 1], [0.49, 3, 1, 1]], np.float32)
    a, va, b, vb, n_landed = both(original, pts, wp, 0)
    assert np.array_equal(va, vb) and n_landed == 2
    assert va[2, 3] == 1 and va[1, 1] == 1 and not va[3].any()   # 2.5 -> 3, 0.5 -> 1 land; 0.49 -> 0 does not


def test_blend_is_add_weighted_for_every_pair_of_bytes():
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = np.clip(np.rint(0.5 * a + 0.5 * b + 1.0), 0, 255).astype(np.uint8)   # np.rint rounds halves to even, as cvRound does
    assert np.array_equal(WR.blend(a, b), want)


def test_quality_and_mosaic_shapes():
    rng = np.random.default_rng(5)
    i1, i2, w = (rng.integers(0, 256, (7, 9), dtype=np.uint8) for _ in range(3))
    valid = (rng.random((7, 9)) < 0.5).astype(np.uint8)
    q, d = WR.quality(i1, i2, w, valid, 63, 40)
    cov = valid.astype(bool)
    assert q["n_covered"] == cov.sum() and q["sum_abs"] == int(d.astype(np.int64).sum()) and not d[~cov].any()
    assert q["sum_sq"] == sum(int(x) ** 2 for x in d[cov]) and tuple(q) == WR.QUALITY_FIELDS
    m = WR.mosaic(i1, i2, w)
    assert m.shape == (14, 18) and np.array_equal(m[:7, :9], i1) and np.array_equal(m[:7, 9:], i2)
    assert np.array_equal(m[7:, 9:], WR.blend(i1, i2))
