"""CPU-side checks of the SURF surface: include/uwt.h declares the entries and states the contract, the library exports them, the
record is the 32 bytes the header lays out, the literal tables of the header equal those of the restatement (read from the
header's text), the ABI stays 4, both mirrors carry the reference's DetectAndTrackFeatures(previous, current, usekeypoints), and the
C++ shim compiles and links.  No device calls here."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import surf_ref as S

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["uwt_default_surf_params", "uwt_surf_detect_describe_batch", "uwt_surf_detect_describe_batch_async",
           "uwt_surf_describe_batch", "uwt_surf_integral", "uwt_surf_response_layer"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "uwt.h")).read()


def test_header_declares_and_library_exports_the_surf_entries(capi, header):
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert re.search(r"\bdouble uwt_keypoint_angle_deg\s*\(", code)
    assert "uwt_keypoint_angle_deg" in capi.SYMBOLS and hasattr(capi.lib(), "uwt_keypoint_angle_deg")
    assert capi.lib().uwt_abi_version() == 4   # additions only: no struct of the existing ABI changed
    assert int(re.search(r"#define UWT_MATCH_MAX_ROWS (\d+)", code).group(1)) == capi.UWT_MATCH_MAX_ROWS
    for phrase in ("src/Tracker.cpp:186-206", "(9 + 6 i) << o", "p(c) = (c s + 4) / 9", "100 Dxx Dyy - 81 Dxy Dxy", "all 26",
                   "(octave, layer i, gy, gx) ascending", "rnd(v) = (int)floorf(v + 0.5f)", "UWT_SURF_ORI_WEIGHT", "UWT_SURF_ORI_DIR",
                   "UWT_SURF_DESC_GAUSS", "q[l] = q[l] + q[l ^ m]", "since round 11"):
        assert phrase in header, phrase
    assert "NOT built, the caller's: detection and description" not in header


def test_record_layouts_match_the_header(capi, header):
    assert capi.KEYPOINT.itemsize == 32 and S.KEYPOINT == capi.KEYPOINT
    assert capi.KEYPOINT.names == ("x", "y", "size", "response", "dir_x", "dir_y", "octave", "laplacian")
    assert [capi.KEYPOINT.fields[n][1] for n in capi.KEYPOINT.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    body = re.search(r"typedef struct uwt_keypoint \{(.*?)\} uwt_keypoint;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "float x, y, size, response, dir_x, dir_y; int32_t octave, laplacian;"
    assert C.sizeof(capi.SurfParams) == 24
    assert [f[0] for f in capi.SurfParams._fields_] == ["hessian_threshold", "n_octaves", "n_octave_layers", "upright"]
    p = capi.default_surf_params()
    assert (p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.upright) == (100.0, 4, 2, 0)
    assert capi.lib().uwt_default_surf_params(None) == capi.ERR_INVALID_ARG
    d = S.default_params()
    assert (d["hessian_threshold"], d["n_octaves"], d["n_octave_layers"], d["upright"]) == (100.0, 4, 2, 0)


def table_after(header, name, count):
    """the `count` float literals printed in the header's comment after the table's name"""
    at = header.index(name)
    vals = re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f\b", header[at:])
    assert len(vals) >= count, name
    return np.array([float(v) for v in vals[:count]], np.float32)


def test_literal_tables_of_the_header_equal_the_restatement(header):
    w = table_after(header, "UWT_SURF_ORI_WEIGHT", 49)
    u = table_after(header, "UWT_SURF_ORI_DIR", 72)
    g = table_after(header, "UWT_SURF_DESC_GAUSS", 10)
    assert w.tobytes() == S.ORI_WEIGHT.tobytes()
    assert u.tobytes() == S.ORI_DIR.tobytes()
    assert g.tobytes() == S.DESC_GAUSS.tobytes()
    assert "0.13333334f" in header and S.SCALE == np.float32(0.13333334)
    # and the tables are what the header says they are, to f32 rounding
    i = np.arange(7)
    assert np.array_equal(S.ORI_WEIGHT, np.exp(-np.add.outer(i * i, i * i) / 12.5).astype(np.float32))
    assert np.allclose(S.ORI_DIR, np.stack([np.cos(np.deg2rad(10.0 * np.arange(36))), np.sin(np.deg2rad(10.0 * np.arange(36)))], 1), atol=1e-7)
    assert np.array_equal(S.DESC_GAUSS, np.exp(-((np.arange(10) + 0.5) ** 2) / (2 * 3.3 ** 2)).astype(np.float32))
    assert len(S.ORI_I) == 109


def test_keypoint_angle_is_a_host_function(capi):
    rng = np.random.default_rng(5)
    for a in list(rng.uniform(0, 360, 200)) + [0.0, 90.0, 180.0, 270.0, 359.999]:
        dx, dy = np.float32(np.cos(np.deg2rad(a))), np.float32(np.sin(np.deg2rad(a)))
        got = capi.keypoint_angle_deg(dx, dy)
        assert 0.0 <= got < 360.0
        assert abs(got - float(S.angle_deg(dx, dy))) <= 1e-6
        assert min(abs(got - a), 360.0 - abs(got - a)) <= 1e-4   # the direction is f32
    assert capi.keypoint_angle_deg(1.0, 0.0) == 0.0 and capi.keypoint_angle_deg(0.0, -1.0) == 270.0


def test_wrappers_exist(capi):
    for name in ("surf_detect_describe_batch", "surf_detect_describe_batch_async", "surf_describe_batch", "surf_integral",
                 "surf_response_layer"):
        assert callable(getattr(capi.Context, name)), name


def test_python_mirror_carries_the_reference_signature(capi):
    tracker = importlib.import_module("uw-slam_amd.tracker")
    calls = []
    kp = np.zeros(5, capi.KEYPOINT)
    kp["x"], kp["y"], kp["size"] = np.arange(5), 10 + np.arange(5), 15.0
    desc = np.eye(5, 64, dtype=np.float32)

    class Ctx:
        def surf_detect_describe_batch(self, slots, params=None, **kw):
            calls.append(("detect", list(slots), params.hessian_threshold, params.n_octaves, params.n_octave_layers, params.upright))
            return [(kp.copy(), desc.copy()) for _ in slots]

        def surf_describe_batch(self, slots, kps, params=None, **kw):
            calls.append(("describe", list(slots), [len(k) for k in kps]))
            return [(np.array(k, capi.KEYPOINT), desc[:len(k)].copy()) for k in kps]

        def match_descriptors_batch(self, pairs, ratio=0.65):
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
    rm = tracker.RobustMatcher(FakeTracker())
    sig = list(inspect.signature(rm.DetectAndTrackFeatures).parameters)
    assert sig[:2] == ["_previous_frame", "_current_frame"] and "usekeypoints" in sig
    good = rm.DetectAndTrackFeatures(prev, cur, False)            # the reference's call: (previous, current, usekeypoints)
    assert calls == [("detect", [0, 1], 100.0, 4, 2, 0)]
    assert len(good) == 3 and prev.n_matches_ == cur.n_matches_ == 3
    assert np.array_equal(prev.keypoints_, np.stack([kp["x"][:3], kp["y"][:3]], 1)) and len(prev.surf_keypoints_) == 3
    del calls[:]
    rm.DetectAndTrackFeatures(prev, cur, True)                    # the kept key points are described again, the current frame detected
    assert calls[0] == ("describe", [0], [3]) and calls[1][:2] == ("detect", [1])
    del calls[:]
    prev.surf_keypoints_ = prev.surf_keypoints_[:0]
    rm.DetectAndTrackFeatures(prev, cur, usekeypoints=True)       # nothing kept: detection
    assert calls == [("detect", [0, 1], 100.0, 4, 2, 0)]
    # the descriptor-taking form stays
    kept = rm.DetectAndTrackFeatures(prev, cur, desc, desc, (np.zeros((5, 2), np.float32), np.ones((5, 2), np.float32)))
    assert len(kept) == 3 and np.array_equal(cur.keypoints_, np.ones((3, 2), np.float32))
    with pytest.raises(TypeError):
        rm.DetectAndTrackFeatures(prev, cur, desc, desc)


def test_cpp_mirror_carries_the_reference_signature_and_shim_compiles(capi, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "uw_tracker.hpp")).read()
    assert re.search(r"DetectAndTrackFeatures\(Frame\* _previous_frame, Frame\* _current_frame, bool usekeypoints\)", hpp)
    assert re.search(r"DetectAndTrackFeatures\(Frame\* _previous_frame, Frame\* _current_frame, const T\* desc_prev", hpp)   # the overload stays
    for phrase in ("uwt_surf_detect_describe_batch(", "uwt_surf_describe_batch(", "surf_keypoints_", "hessian_threshold_ = 100.0"):
        assert phrase in hpp, phrase
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_surf")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_surf.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
