"""The restatement of the SURF contract (tests/surf_ref.py) on its own: that the contract is SURF — blobs are found where they are,
at their scale and with their sign; the key points move with the image; descriptors survive a rotation; the chain to RANSAC inliers
holds — and that it still computes what the committed vectors record.  The bars of the translation, rotation and chain tests are
set below the values measured over at least five seeds each (profiles/r11/README.md)."""
import os

import numpy as np
import pytest

import match_ref as M
import ransac_ref as R
import surf_cases as K
import surf_ref as S

ARITH_INDEPENDENT = True
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surf_160x96.npz")


@pytest.fixture(scope="module")
def blob_keypoints():
    return S.detect_describe(K.blob_image())


def test_ref_blobs_known_answers(blob_keypoints):
    kp, desc = blob_keypoints
    assert len(kp) == len(K.BLOBS)                       # exactly one key point per blob, nothing else
    taken = set()
    for x, y, sigma, pol in K.BLOBS:
        d = np.hypot(kp["x"] - x, kp["y"] - y)
        near = np.nonzero(d <= 1.0)[0]
        assert near.size == 1, (x, y, sigma, d.min())    # within 1 px of its centre
        k = kp[near[0]]
        taken.add(int(near[0]))
        assert k["laplacian"] == -pol                    # a bright blob has a negative Laplacian
        assert k["octave"] == K.BLOB_OCTAVE[sigma]
        assert 4.5 * sigma <= k["size"] <= 6.5 * sigma   # the filter that fits a Gaussian blob: ~5.5 sigma
        assert k["response"] > 100.0
    assert len(taken) == len(K.BLOBS)
    assert set(kp["octave"].tolist()) == {0, 1, 2, 3}    # every octave produces at least one key point
    assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-6)
    order = list(zip(kp["octave"].tolist(), kp["size"].tolist()))
    assert [o for o, _ in order] == sorted(o for o, _ in order)


def test_ref_flat_small_and_capacity():
    assert len(S.detect(K.flat(160, 96))) == 0
    assert len(S.detect(K.texture(20, 20, 1))) == 0      # too small for octave 0: its largest filter is 27
    assert S.octaves_of(160, 96, S.default_params()) == [0, 1] and S.octaves_of(256, 240, S.default_params()) == [0, 1, 2, 3]
    img = K.texture(160, 96, 3)
    full, few = S.detect(img), S.detect(img, None, 16)
    assert len(full) > 16 and len(few) == 16
    keep = np.sort(np.lexsort((np.arange(len(full)), -full["response"].astype(np.float64)))[:16])
    assert K.same_keypoints(few, full[keep]) is None


@pytest.mark.parametrize("seed", [40, 41, 42, 43, 44])
def test_ref_integer_translation(seed):
    """content away from the border, moved by whole pixels: the same key points, moved.  A shift by a multiple of 8 keeps every
    octave's grid in phase (all octaves compared); an odd shift keeps octave 0's (step 1) alone."""
    w, h, margin = 256, 240, 40
    a = S.detect(K.padded_texture(w, h, seed, margin))
    print("seed", seed, "key points", len(a), np.bincount(a["octave"], minlength=4))
    assert len(a) >= 60                                   # measured 105..143
    for shift, octaves in (((8, -16), (0, 1, 2, 3)), ((3, 5), (0,))):
        b = S.detect(K.padded_texture(w, h, seed, margin, shift))
        a2, b2 = a[np.isin(a["octave"], octaves)], b[np.isin(b["octave"], octaves)]
        assert len(a2) == len(b2)                         # no key point is left out of the comparison
        assert np.abs(b2["x"] - (a2["x"] + shift[0])).max() <= 1e-3 and np.abs(b2["y"] - (a2["y"] + shift[1])).max() <= 1e-3
        assert np.array_equal(a2["size"], b2["size"]) and np.array_equal(a2["response"], b2["response"])
        assert np.array_equal(a2["laplacian"], b2["laplacian"]) and np.array_equal(a2["octave"], b2["octave"])


@pytest.mark.parametrize("seed", [50, 51, 52, 53, 54])
def test_ref_rot90_orientation(seed):
    """np.rot90 of a texture frame: the matches that pass the ratio test land on the rotated positions — the orientation test"""
    n = 160
    img = K.texture(n, n, seed)
    k0, d0 = S.detect_describe(img)
    k1, d1 = S.detect_describe(np.ascontiguousarray(np.rot90(img)))
    m, _, _ = M.match(d0, d1, 0.65)
    x, y = k0["x"][m["query_idx"]], k0["y"][m["query_idx"]]
    err = np.hypot(k1["x"][m["train_idx"]] - y, k1["y"][m["train_idx"]] - (n - 1 - x))   # rot90: (x, y) -> (y, n - 1 - x)
    share = float((err <= 2.0).mean())
    print("seed", seed, "key points", len(k0), len(k1), "matches", len(m), "share within 2 px", share)
    assert len(m) >= 35                                   # measured 52..78
    assert share >= 0.9                                   # measured 1.0 on eight seeds
    # the directions turn with the image: (c, s) -> (s, -c)
    a0 = S.angle_deg(k0["dir_x"][m["query_idx"]], k0["dir_y"][m["query_idx"]])
    a1 = S.angle_deg(k1["dir_x"][m["train_idx"]], k1["dir_y"][m["train_idx"]])
    turn = (a1 - a0 + 540.0) % 360.0 - 180.0
    assert np.median(np.abs(turn + 90.0)) <= 10.0         # one 10-degree window step


@pytest.mark.parametrize("seed", [60, 61, 62, 63, 64])
def test_ref_chain_to_ransac_inliers(synth, seed):
    ref, tgt, _, _, _ = synth.render_pair(256, 240, 210.0, 210.0, 127.5, 119.5, seed=seed)
    (k0, d0), (k1, d1) = S.detect_describe(ref), S.detect_describe(tgt)
    m, _, _ = M.match(d0, d1, 0.65)
    xy0, xy1 = np.stack([k0["x"], k0["y"]], 1), np.stack([k1["x"], k1["y"]], 1)
    _, good, info = R.ransac(m, xy0, xy1)
    print("seed", seed, "key points", len(k0), len(k1), "matches", len(m), "inliers", len(good))
    assert len(m) >= 90                                   # measured 130..183
    assert len(good) >= 8


def test_ref_angle():
    assert S.angle_deg(1, 0) == 0.0 and S.angle_deg(0, 1) == 90.0 and S.angle_deg(-1, 0) == 180.0 and S.angle_deg(0, -1) == 270.0
    a = S.angle_deg(np.float32(0.5), np.float32(-0.8660254))
    assert abs(float(a) - 300.0) <= 1e-5


def test_ref_equals_committed_vectors():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_surf_golden", os.path.join(os.path.dirname(GOLDEN), "make_surf_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    g = np.load(GOLDEN)
    now = maker.vectors()
    assert sorted(g.files) == sorted(now)
    for k in g.files:
        assert g[k].dtype == now[k].dtype and g[k].tobytes() == np.ascontiguousarray(now[k]).tobytes(), k
    assert len(g["keypoints"]) >= 30 and set(g["keypoints"]["octave"].tolist()) == {0, 1}
