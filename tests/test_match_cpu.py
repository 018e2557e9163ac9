"""CPU-side checks of the descriptor-matching surface: include/uwt.h declares the entries, the library exports them, uw-slam_amd.capi
wraps them, the two mirrors carry RobustMatcher, and the C++ one compiles and links.  No compute calls here."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ARITH_INDEPENDENT = True   # matching has no arithmetic set
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["uwt_knn_match_batch", "uwt_match_descriptors_batch", "uwt_match_descriptors_batch_async"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


def test_header_declares_and_library_exports_the_matching_entries(capi):
    src = open(os.path.join(ROOT, "include", "uwt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert "UWT_NORM_L2 = 0" in code and "UWT_NORM_HAMMING = 1" in code
    assert int(re.search(r"#define UWT_MATCH_MAX_ROWS (\d+)", code).group(1)) == capi.MATCH_MAX_ROWS
    assert int(re.search(r"#define UWT_MATCH_MAX_ROW_BYTES (\d+)", code).group(1)) == capi.MATCH_MAX_ROW_BYTES >= 128 * 4
    assert capi.lib().uwt_abi_version() == 4   # no struct of the existing ABI changed
    # the contract is stated where the other entries cite the reference
    for phrase in ("src/Tracker.cpp:202-236", "ransacTest", "LOWEST j", "!(d0 / d1 > ratio)"):
        assert phrase in src, phrase


def test_record_layouts_match_the_header(capi):
    assert capi.KNN2.itemsize == 16 and capi.KNN2.names == ("idx0", "idx1", "d0", "d1")
    assert capi.MATCH.itemsize == 12 and capi.MATCH.names == ("query_idx", "train_idx", "distance")


def test_wrappers_pack_pairs_into_the_fixed_stride_form(capi):
    for name in ("knn_match_batch", "match_descriptors_batch", "match_descriptors_batch_async"):
        assert callable(getattr(capi.Context, name))
    A, B = np.arange(12, dtype=np.float32).reshape(3, 4), np.ones((5, 4), np.float32)
    norm, dim, cap, q, nq, t, nt = capi.Context._descriptor_block([(A, B), (B[:0], A)], None, None)
    assert (norm, dim, cap) == (capi.NORM_L2, 4, 5) and q.shape == t.shape == (2, 5, 4)
    assert list(nq) == [3, 0] and list(nt) == [5, 3]
    assert np.array_equal(q[0, :3], A) and not q[0, 3:].any() and np.array_equal(t[1, :3], A)
    norm, dim, cap, *_ = capi.Context._descriptor_block([(A.astype(np.uint8), B.astype(np.uint8))], None, 9)
    assert (norm, dim, cap) == (capi.NORM_HAMMING, 4, 9)
    with pytest.raises(ValueError):
        capi.Context._descriptor_block([(A, B.astype(np.uint8))], None, None)
    with pytest.raises(ValueError):
        capi.Context._descriptor_block([(A.astype(np.float64), B.astype(np.float64))], None, None)


def test_python_mirror_gathers_and_sets_keypoints():
    tracker = importlib.import_module("uw-slam_amd.tracker")
    capi = importlib.import_module("uw-slam_amd.capi")
    rm = tracker.RobustMatcher(None)
    assert rm.ratio_ == float(np.float32(0.65))   # include/Tracker.h:80
    matches = np.array([(0, 2, 1.0), (3, 1, 2.0)], capi.MATCH)
    kp0 = np.arange(10, dtype=np.float32).reshape(5, 2)
    kp1 = 100 + np.arange(8, dtype=np.float32).reshape(4, 2)
    g0, g1 = rm.getGoodKeypoints(matches, (kp0, kp1))
    assert np.array_equal(g0, kp0[[0, 3]]) and np.array_equal(g1, kp1[[2, 1]])
    prev, cur = tracker.Frame(np.zeros((4, 4), np.uint8)), tracker.Frame(np.zeros((4, 4), np.uint8))
    assert prev.n_matches_ == 0   # include/System.h:93
    rm.MatchDescriptors = lambda a, b: matches   # (the GPU call: tests/test_gpu_match.py)
    kept = rm.MatchAndSetKeypoints(prev, cur, None, None, (kp0, kp1), inlier_mask=[True, False])
    assert len(kept) == 1 and prev.n_matches_ == cur.n_matches_ == 1
    assert np.array_equal(prev.keypoints_, kp0[[0]]) and np.array_equal(cur.keypoints_, kp1[[2]])


def test_match_mirror_compiles_and_links(capi, tmp_path):
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_match")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_match.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
