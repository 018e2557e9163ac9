"""CPU-side checks of the ORB surface: the library's host functions equal the restatement exactly (tests/orb_ref.py),
include/uwt.h declares the entries and states the contract, the library exports them, the ABI stays 4, and the Python mirror's
RobustMatcher(detector=1) runs the reference's ORB branch.  No device calls here."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import orb_ref as O

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["uwt_default_orb_params", "uwt_orb_level_quota", "uwt_orb_default_pattern", "uwt_orb_layer_size", "uwt_orb_set_pattern",
           "uwt_orb_detect_describe_batch", "uwt_orb_detect_describe_batch_async", "uwt_orb_describe_batch", "uwt_orb_layer",
           "uwt_orb_fast_scores", "uwt_orb_harris"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "uwt.h")).read()


def test_host_functions_equal_the_restatement(capi):
    assert capi.lib().uwt_abi_version() == 4   # additions only: no struct of the existing ABI changed
    p, d = capi.default_orb_params(), O.default_params()
    assert C.sizeof(capi.OrbParams) == 20
    assert [f[0] for f in capi.OrbParams._fields_] == ["n_features", "n_levels", "edge_threshold", "fast_threshold", "upright"] == list(d)
    assert [getattr(p, k) for k in d] == [d[k] for k in d] == [500, 8, 31, 20, 0]
    assert capi.lib().uwt_default_orb_params(None) == capi.ERR_INVALID_ARG
    for nl in range(1, 9):
        for nf in list(range(0, 260)) + [499, 500, 501, 1000, 1999, 4096, 65536]:
            assert capi.orb_level_quota(nf, nl).tolist() == O.level_quota(nf, nl), (nf, nl)
    for bad in ((500, 0), (500, 9), (-1, 8)):
        with pytest.raises(capi.UwtError):
            capi.orb_level_quota(*bad)
    got = capi.orb_default_pattern()
    assert got.dtype == np.int8 and got.shape == (256, 4) and got.tobytes() == O.default_pattern().tobytes()
    for w, h in ((160, 96), (97, 91), (256, 240), (640, 480), (735, 479), (1, 1), (16384, 16384)):
        for l in range(8):
            assert capi.orb_layer_size(w, h, l) == O.layer_size(w, h, l), (w, h, l)
    for bad in ((0, 96, 0), (160, 96, 8), (160, 96, -1)):
        with pytest.raises(capi.UwtError):
            capi.orb_layer_size(*bad)
    assert capi.lib().uwt_orb_set_pattern(None, None) == capi.ERR_INVALID_ARG


def test_header_declares_and_library_exports_the_orb_entries(capi, header):
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    body = re.search(r"typedef struct uwt_orb_params \{(.*?)\} uwt_orb_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == ("int32_t n_features; int32_t n_levels; int32_t edge_threshold; int32_t fast_threshold; "
                                                 "int32_t upright;")
    for phrase in ("src/Tracker.cpp:210-223", "w_l = (w 5^l + 6^l / 2) / 6^l", "N = (2 x + 1) w - w_l", "UWT_ORB_RING", "UWT_ORB_UMAX",
                   "H = 25 (a b - c c) - (a + b)(a + b)", "(H descending, y ascending, x ascending)", "rnd(v) = (int)floorf(v + 0.5f)",
                   "0x6f726221", "x x + y y <= 225", "since round 16", "an ORB branch of uwt_tracking_batch"):
        assert phrase in header, phrase
    assert "NOT built: cuda::ORB" not in header
    # the literal tables of the header are those of the restatement
    at = header.index("UWT_ORB_RING")
    ring = re.findall(r"\((-?\d),(-?\d)\)", header[at:])[:16]
    assert [(int(a), int(b)) for a, b in ring] == O.RING
    at = header.index("UWT_ORB_UMAX")
    umax = re.search(r"U = ((?:\d+, ){15}\d+)", header[at:]).group(1)
    assert [int(v) for v in umax.split(",")] == O.UMAX


def test_wrappers_exist(capi):
    for name in ("orb_set_pattern", "orb_detect_describe_batch", "orb_detect_describe_batch_async", "orb_describe_batch", "orb_layer",
                 "orb_fast_scores", "orb_harris"):
        assert callable(getattr(capi.Context, name)), name


def test_python_mirror_runs_the_orb_branch(capi):
    tracker = importlib.import_module("uw-slam_amd.tracker")
    calls = []
    kp = np.zeros(5, capi.KEYPOINT)
    kp["x"], kp["y"], kp["size"] = 40 + np.arange(5), 50 + np.arange(5), 31.0
    desc = np.eye(5, 32, dtype=np.uint8)

    class Ctx:
        def orb_set_pattern(self, pattern=None):
            calls.append(("pattern", None if pattern is None else np.asarray(pattern).shape))

        def orb_detect_describe_batch(self, slots, params=None, **kw):
            calls.append(("detect", list(slots), params.n_features, params.n_levels, params.edge_threshold, params.fast_threshold, params.upright))
            return [(kp.copy(), desc.copy()) for _ in slots]

        def orb_describe_batch(self, slots, kps, params=None, **kw):
            calls.append(("describe", list(slots), [len(k) for k in kps]))
            return [(np.array(k, capi.KEYPOINT), desc[:len(k)].copy()) for k in kps]

        def match_descriptors_batch(self, pairs, ratio=0.65):
            assert pairs[0][0].dtype == np.uint8 and pairs[0][0].shape[1] == 32    # byte rows: matched under Hamming
            n = min(len(pairs[0][0]), len(pairs[0][1]))
            return [np.array([(i, i, 0.0) for i in range(n)], capi.MATCH)]

        def ransac_inliers_batch(self, pairs, params=None):
            m = pairs[0][0]
            return [(np.ones(len(m), np.uint8), m[:3], np.zeros((), capi.RANSAC_INFO))]

    class FakeTracker:
        _ctx = Ctx()

        def _bind(self, frame):
            frame._slot = 0 if frame is prev else 1
            return frame._slot

    prev, cur = tracker.Frame(np.zeros((4, 4), np.uint8)), tracker.Frame(np.zeros((4, 4), np.uint8))
    assert len(prev.orb_keypoints_) == 0 and prev.orb_keypoints_.dtype == capi.KEYPOINT
    rm = tracker.RobustMatcher(FakeTracker(), detector=1)
    assert rm.detector_ == 1 and tracker.RobustMatcher(FakeTracker()).detector_ == 0
    with pytest.raises(ValueError):
        tracker.RobustMatcher(FakeTracker(), detector=2)
    good = rm.DetectAndTrackFeatures(prev, cur, False)
    assert calls == [("detect", [0, 1], 500, 8, 31, 20, 0)]
    assert len(good) == 3 and prev.n_matches_ == cur.n_matches_ == 3
    assert np.array_equal(prev.keypoints_, np.stack([kp["x"][:3], kp["y"][:3]], 1))
    assert len(prev.orb_keypoints_) == len(cur.orb_keypoints_) == 3 and len(prev.surf_keypoints_) == 0
    del calls[:]
    rm.DetectAndTrackFeatures(prev, cur, True)                    # the kept records are described again, the current frame detected
    assert calls[0] == ("describe", [0], [3]) and calls[1][:2] == ("detect", [1])
    del calls[:]
    prev.orb_keypoints_ = prev.orb_keypoints_[:0]
    rm.n_features_, rm.fast_threshold_, rm.orb_pattern_ = 300, 12, O.default_pattern()
    rm.DetectAndTrackFeatures(prev, cur, usekeypoints=True)       # nothing kept: detection; the pattern goes first, once
    assert calls == [("pattern", (256, 4)), ("detect", [0, 1], 300, 8, 31, 12, 0)]
    del calls[:]
    rm.DetectAndTrackFeatures(prev, cur, False)
    assert calls[0][0] == "detect"
