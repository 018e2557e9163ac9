"""CPU-side checks of the RANSAC surface: include/uwt.h declares the entries and states the contract, the library exports them,
uw-slam_amd.capi wraps them, uwt_ransac_iterations (a host function) equals its formula, the mirrors carry ransacTest, and the
C++ one compiles and links.  No device calls here."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["uwt_default_ransac_params", "uwt_ransac_iterations", "uwt_ransac_inliers_batch", "uwt_ransac_inliers_batch_async"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


def test_header_declares_and_library_exports_the_ransac_entries(capi):
    src = open(os.path.join(ROOT, "include", "uwt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b(int|int32_t) %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert int(re.search(r"#define UWT_RANSAC_MAX_HYPOTHESES (\d+)", code).group(1)) == capi.RANSAC_MAX_HYPOTHESES
    assert capi.lib().uwt_abi_version() == 4   # no struct of the existing ABI changed
    # the contract is stated where the other entries cite the reference
    for phrase in ("src/Tracker.cpp:105-169", "0x7feb352d", "0x846ca68b", "(u * (N - s)) >> 32", "full pivoting", "|v| > best",
                   "lowest unused column", "d1 <= t2 && d2 <= t2", "count_h > max(best, 7)", "hypotheses_run", "since round 10", "refit"):
        assert phrase in src, phrase


def test_record_layouts_match_the_header(capi):
    assert capi.RANSAC_INFO.itemsize == 88
    assert capi.RANSAC_INFO.names == ("status", "n_inliers", "best_hypothesis", "hypotheses_run", "F")
    assert C.sizeof(capi.RansacParams) == 24
    assert [f[0] for f in capi.RansacParams._fields_] == ["distance", "confidence", "max_hypotheses", "seed"]
    p = capi.default_ransac_params()
    assert (p.distance, p.confidence, p.max_hypotheses, p.seed) == (3.0, 0.99, 1000, 0)   # include/Tracker.h:82-83
    assert capi.lib().uwt_default_ransac_params(None) == capi.ERR_INVALID_ARG


def formula(confidence, n, k, H):
    """need(k) as include/uwt.h states it, with Python's math.log (the same libm, the same operation order)"""
    if confidence == 1 or k <= 0 or n <= 0:
        return H
    w = k / n
    w2 = w * w
    w4 = w2 * w2
    w8 = w4 * w4
    num = math.log(1 - confidence)
    den = math.log(1 - w8) if w8 < 1 else -math.inf
    if den >= 0 or -num >= H * (-den):
        return H
    return round(num / den)   # half to even, as rint


def test_ransac_iterations_equals_the_formula(capi):
    checked = 0
    for confidence in (0.5, 0.9, 0.99, 0.999, 0.999999, 1.0, 1e-9):
        for n in (1, 7, 8, 9, 63, 200, 257, 2000, 4096):
            for H in (1, 255, 1000, capi.RANSAC_MAX_HYPOTHESES):
                for k in sorted(set(list(range(0, min(n, 64) + 1)) + list(range(0, n + 1, max(1, n // 97))) + [n - 1, n])):
                    assert capi.ransac_iterations(confidence, n, k, H) == formula(confidence, n, k, H), (confidence, n, k, H)
                    checked += 1
    assert checked > 10000
    assert capi.ransac_iterations(0.99, 200, 200, 1000) == 0 and capi.ransac_iterations(0.99, 200, 0, 1000) == 1000
    assert capi.ransac_iterations(1.0, 200, 150, 1000) == 1000 and capi.ransac_iterations(0.99, 0, 0, 1000) == 1000
    assert capi.ransac_iterations(0.99, 200, 140, 1000) == 78


def test_wrappers_pack_pairs_into_the_fixed_stride_form(capi):
    for name in ("ransac_inliers_batch", "ransac_inliers_batch_async"):
        assert callable(getattr(capi.Context, name))
    m = np.array([(0, 1, 0.5), (2, 0, 0.25)], capi.MATCH)
    a, b = np.arange(6, dtype=np.float32).reshape(3, 2), np.arange(4, dtype=np.float32).reshape(2, 2)
    cap, kp_cap, mt, nm, k0, n0, k1, n1 = capi.Context._ransac_block([(m, a, b), (m[:0], b, a)], None, None)
    assert (cap, kp_cap) == (2, 3) and mt.shape == (2, 2) and k0.shape == k1.shape == (2, 3, 2)
    assert list(nm) == [2, 0] and list(n0) == [3, 2] and list(n1) == [2, 3]
    assert mt[0].tobytes() == m.tobytes() and np.array_equal(k0[0], a) and np.array_equal(k1[1], a) and not k1[0, 2:].any()
    assert capi.Context._ransac_block([(m, a, b)], 9, 11)[:2] == (9, 11)


def test_python_mirror_carries_ransac_test():
    tracker = importlib.import_module("uw-slam_amd.tracker")
    capi = importlib.import_module("uw-slam_amd.capi")
    rm = tracker.RobustMatcher(None)
    assert (rm.distance_, rm.confidence_, rm.refineF_) == (3.0, 0.99, True)   # include/Tracker.h:81-83
    matches = np.array([(0, 2, 1.0), (3, 1, 2.0), (4, 0, 3.0)], capi.MATCH)
    kp0 = np.arange(10, dtype=np.float32).reshape(5, 2)
    kp1 = 100 + np.arange(8, dtype=np.float32).reshape(4, 2)
    seen = {}

    def fake(pairs, params=None):   # (the GPU call: tests/test_gpu_ransac.py)
        seen["params"] = (params.distance, params.confidence, params.max_hypotheses, params.seed)
        m = pairs[0][0]
        return [(np.array([1, 0, 1], np.uint8), m[[0, 2]], np.zeros((), capi.RANSAC_INFO))]

    class Ctx:
        ransac_inliers_batch = staticmethod(fake)
    rm._src = Ctx()
    rm.MatchDescriptors = lambda a, b: matches
    out = []
    good, mask, _ = rm.ransacTest(matches, kp0, kp1, out)
    assert len(good) == len(out) == 2 and list(mask) == [1, 0, 1] and seen["params"] == (3.0, 0.99, 1000, 0)
    prev, cur = tracker.Frame(np.zeros((4, 4), np.uint8)), tracker.Frame(np.zeros((4, 4), np.uint8))
    kept = rm.DetectAndTrackFeatures(prev, cur, None, None, (kp0, kp1))
    assert len(kept) == 2 and prev.n_matches_ == cur.n_matches_ == 2
    assert np.array_equal(prev.keypoints_, kp0[[0, 4]]) and np.array_equal(cur.keypoints_, kp1[[2, 0]])


def test_ransac_mirror_compiles_and_links(capi, tmp_path):
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_ransac")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_ransac.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "uw_tracker.hpp")).read()
    for phrase in ("ransacTest(", "DetectAndTrackFeatures(", "distance_ = 3.0", "confidence_ = 0.99", "refineF_"):
        assert phrase in hpp, phrase
