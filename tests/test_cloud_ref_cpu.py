"""tests/cloud_ref.py pinned on cases small enough to compute by hand: a 3 x 2 frame with power-of-two intrinsics (fx = fy = 2, cx = 1,
cy = 0.5: every operation is exact, so both arithmetic sets must give the hand values), identity pose, a pure translation, a stride
beyond the table, an all-zero depth frame, and the bookkeeping of a batch."""
from types import SimpleNamespace

import numpy as np

import cloud_ref as CR

L32 = SimpleNamespace(w=3, h=2, fx=2.0, fy=2.0, cx=1.0, cy=0.5, invfx=0.5, invfy=0.5, iw=3, ih=2)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
SHIFT = np.array([0, 0, 0, 1, 1, 2, 3], np.float32)
DEPTH = np.array([[2, 4, 8], [0, 2, 4]], np.uint16)   # x depth_scale 0.5: z = 1 2 4 / invalid 1 2
IMAGE = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
# ObtainAllPoints' table by hand: rows i = y * 3 + x, a zero depth gives [0 0 1 0]
TABLE = np.array([[0, 0, 1, 1], [1, 0, 2, 1], [2, 0, 4, 1], [0, 0, 1, 0], [1, 1, 1, 1], [2, 1, 2, 1]], np.float32)
# X = (x - 1) / 2 * z, Y = (y - 0.5) / 2 * z
X = np.array([-0.5, 0.0, 2.0, -0.5, 0.0, 1.0], np.float32)
Y = np.array([-0.25, -0.5, -1.0, -0.25, 0.25, 0.5], np.float32)
Z = np.array([1, 2, 4, 1, 1, 2], np.float32)
W = TABLE[:, 3]
INTENSITY = np.array([10, 20, 30, 10, 50, 60], np.uint32)   # image[(int)y][(int)x]; the invalid row reads pixel (0, 0)


def xyz(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1)


def test_dense_table_is_the_hand_table(O):
    assert np.array_equal(O.dense_points(DEPTH, 3, 2, 0, 0.5), TABLE)


def test_unprojection_by_hand_in_both_sets():
    for name in ("opencv", "legacy"):
        x, y, z = CR.unproject(TABLE, L32, name)
        assert np.array_equal(x, X) and np.array_equal(y, Y) and np.array_equal(z, Z), name


def test_identity_pose_mode0_is_minus_x_minus_z_minus_y(O, arith):
    rec, n_sel = CR.visualizer_loop(O, TABLE, IDENTITY, L32, arith, mode=0, stride=1, image=IMAGE, frame_index=3)
    assert n_sel == 6 and rec.size == 6
    assert np.array_equal(xyz(rec), np.stack([-X, -Z, -Y], axis=1))
    assert np.array_equal(rec["tag"], INTENSITY | np.uint32(3 << 8))


def test_identity_pose_mode1_is_the_camera_point(O, arith):
    rec, _ = CR.visualizer_loop(O, TABLE, IDENTITY, L32, arith, mode=1, stride=1)
    assert np.array_equal(xyz(rec), np.stack([X, Y, Z], axis=1))
    assert not rec["tag"].any()   # no image: intensity 0, frame 0


def test_pure_translation(O, arith):
    rec0, _ = CR.visualizer_loop(O, TABLE, SHIFT, L32, arith, mode=0, stride=1)
    assert np.array_equal(xyz(rec0), np.stack([-X - 1, -Z - 3, -Y - 2], axis=1))   # t unpermuted: (x, z, y) pairs with (tx, tz, ty)
    rec1, _ = CR.visualizer_loop(O, TABLE, SHIFT, L32, arith, mode=1, stride=1)
    assert np.array_equal(xyz(rec1), np.stack([X + 1 * W, Y + 2 * W, Z + 3 * W], axis=1))   # the w = 0 row takes no translation


def test_selection_and_stride_beyond_the_table(O, arith):
    rec, n_sel = CR.visualizer_loop(O, TABLE, IDENTITY, L32, arith, stride=2)
    assert n_sel == 3 and np.array_equal(xyz(rec), np.stack([-X, -Z, -Y], axis=1)[[0, 2, 4]])
    rec, n_sel = CR.visualizer_loop(O, TABLE, IDENTITY, L32, arith, stride=100)
    assert n_sel == 1 and np.array_equal(xyz(rec), [[0.5, -1.0, 0.25]])   # row 0 only
    rec, n_sel = CR.visualizer_loop(O, TABLE, IDENTITY, L32, arith, stride=3, skip_invalid=1)   # rows 0 and 3; row 3 has w = 0
    assert n_sel == 2 and rec.size == 1 and np.array_equal(xyz(rec), [[0.5, -1.0, 0.25]])
    rec, n_sel = CR.visualizer_loop(O, np.zeros((0, 4), np.float32), IDENTITY, L32, arith)
    assert n_sel == 0 and rec.size == 0


def test_all_zero_depth_frame(O, arith):
    tab = O.dense_points(np.zeros((2, 3), np.uint16), 3, 2, 0, 0.5)
    assert np.array_equal(tab, np.tile(np.array([0, 0, 1, 0], np.float32), (6, 1)))
    rec, n_sel = CR.visualizer_loop(O, tab, SHIFT, L32, arith, stride=2, skip_invalid=1)
    assert n_sel == 3 and rec.size == 0
    rec, n_sel = CR.visualizer_loop(O, tab, SHIFT, L32, arith, stride=2, skip_invalid=0)   # the reference emits them: N / stride bogus rows
    assert n_sel == 3 and rec.size == 3
    assert np.array_equal(xyz(rec), np.tile(np.array([0.5 - 1, -1.0 - 3, 0.25 - 2], np.float32), (3, 1)))


def test_vectorised_selection_equals_the_loop(O, arith):
    rng = np.random.default_rng(3)
    tab = rng.uniform(-2, 5, (257, 4)).astype(np.float32)
    tab[rng.integers(0, 257, 60), 3] = 0
    tab[5, 0] = np.nan
    pose = np.array([0.01, -0.02, 0.03, 0.999, 0.3, -0.2, 0.1], np.float32)
    img = rng.integers(0, 256, (2, 3), dtype=np.uint8)
    for mode in (0, 1):
        for stride in (1, 7, 300):
            for skip in (0, 1):
                a, na = CR.visualizer_loop(O, tab, pose, L32, arith, mode, stride, skip, img, 2)
                b, nb = CR.frame_cloud(O, tab, pose, L32, arith, mode, stride, skip, img, 2)
                assert na == nb and a.tobytes() == b.tobytes(), (mode, stride, skip)


def test_batch_bookkeeping(O, arith):
    zero = np.tile(np.array([0, 0, 1, 0], np.float32), (6, 1))
    bad = SHIFT.copy()
    bad[5] = np.nan
    frames = [(TABLE, IDENTITY, IMAGE), (zero, SHIFT, IMAGE), (TABLE, bad, IMAGE), (TABLE, SHIFT, None)]
    pts, info, call = CR.batch_cloud(O, frames, L32, arith, stride=1, skip_invalid=1)
    assert info == [(0, 6, 6, 5, 0, 5), (0, 6, 6, 0, 5, 0), (1, 0, 0, 0, 5, 0), (0, 6, 6, 5, 5, 5)]
    assert call == (0, 4, 0, 0, 10, 10) and pts.size == 10
    assert np.array_equal(pts["tag"] >> 8, [0] * 5 + [3] * 5)
    assert np.array_equal(pts["tag"][:5] & 255, INTENSITY[[0, 1, 2, 4, 5]]) and not (pts["tag"][5:] & 255).any()
    pts2, info2, call2 = CR.batch_cloud(O, frames, L32, arith, stride=1, skip_invalid=1, cap=7)
    assert pts2.tobytes() == pts.tobytes()   # the full cloud; the caller compares the first `written` records
    assert [r[5] for r in info2] == [5, 0, 0, 2] and call2 == (CR.CAPACITY, 4, 0, 0, 10, 7)
    pts3, info3, call3 = CR.batch_cloud(O, frames, L32, arith, stride=4, skip_invalid=0)
    assert [r[2:5] for r in info3] == [(2, 2, 0), (2, 2, 2), (0, 0, 4), (2, 2, 4)] and call3[4] == 6
