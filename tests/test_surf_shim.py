"""The C++ side of SURF (tests/cpp/shim_surf.cpp over include/uw_tracker.hpp and the C ABI): on the GPU the shim's key points and
descriptors equal the restatement's bits, and uw::RobustMatcher::DetectAndTrackFeatures(previous, current, usekeypoints) keeps what
the Python chain keeps."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import match_ref as M
import ransac_ref as R
import surf_cases as K
import surf_ref as S

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(path, native=True):
    if native:
        importlib.import_module("uw-slam_amd").build_native()
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_surf.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_shim_surf_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_surf")))


@pytest.mark.gpu
def test_shim_surf_equals_restatement(synth, tmp_path):
    exe = build_exe(str(tmp_path / "shim_surf"), native=False)   # against the library that is there: one g++ call
    w, h = 160, 96
    ref, tgt, _, _, _ = synth.render_pair(w, h, 131.25, 131.25, 79.5, 47.5, seed=9)
    (tmp_path / "ref.u8").write_bytes(ref.tobytes())
    (tmp_path / "tgt.u8").write_bytes(tgt.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(w), str(h), str(tmp_path / "ref.u8"), str(tmp_path / "tgt.u8"), str(out)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    n = struct.unpack_from("<i", b, 0)[0]
    o = 4
    kp = np.frombuffer(b, S.KEYPOINT, n, o); o += 32 * n
    desc = np.frombuffer(b, np.float32, n * 64, o).reshape(n, 64); o += 256 * n
    ng = struct.unpack_from("<i", b, o)[0]; o += 4
    good = np.frombuffer(b, M.MATCH, ng, o); o += 12 * ng
    kept = np.frombuffer(b, np.float32, ng * 2, o).reshape(ng, 2); o += 8 * ng
    ng2 = struct.unpack_from("<i", b, o)[0]; o += 4
    angle = struct.unpack_from("<d", b, o)[0]
    (wk0, wd0), (wk1, wd1) = S.detect_describe(ref), S.detect_describe(tgt)
    assert K.same_keypoints(kp, wk0) is None, K.same_keypoints(kp, wk0)
    assert K.same_descriptors(desc, wd0) is None
    m, _, _ = M.match(wd0, wd1, 0.65)
    xy0, xy1 = np.stack([wk0["x"], wk0["y"]], 1), np.stack([wk1["x"], wk1["y"]], 1)
    _, wgood, _ = R.ransac(m, xy0, xy1)
    assert good.tobytes() == wgood.tobytes() and len(good) >= 8
    assert kept.tobytes() == xy0[wgood["query_idx"]].tobytes()
    assert abs(angle - float(S.angle_deg(wk0["dir_x"][0], wk0["dir_y"][0]))) <= 1e-6
    # the second call described the previous frame at its kept key points: the same descriptors there, so every kept match is found
    # again unless the ratio test now fails among fewer rows; it cannot gain matches
    assert 8 <= ng2 <= ng
