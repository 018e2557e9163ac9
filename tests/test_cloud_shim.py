"""The C++ side of the point-cloud map (tests/cpp/shim_cloud.cpp over include/uw_tracker.hpp and the C ABI): uw::Tracker::PointCloudBatch,
uw::Visualizer::AddPointCloudFromRGBD and uw::Map::AddPointCloudFromRGBD compile and link, and on the GPU their bytes are those of the
Python mirror (uw-slam_amd/tracker.py)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(path, native=True):
    if native:
        importlib.import_module("uw-slam_amd").build_native()
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_cloud.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.one_arith
def test_shim_cloud_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_cloud")))


@pytest.mark.gpu
def test_shim_cloud_equals_the_python_mirror(synth, tmp_path, arith):
    capi = importlib.import_module("uw-slam_amd.capi")
    M = importlib.import_module("uw-slam_amd.tracker")
    exe = build_exe(str(tmp_path / "shim_cloud"), native=False)   # against the library that is there: one g++ call
    w, h = 160, 96
    ia, ib, _, _, _ = synth.render_pair(w, h, 131.25, 131.25, 79.5, 47.5, seed=5)
    ys, xs = np.mgrid[0:h, 0:w]
    da = (3000 + 17 * xs + 29 * ys).astype(np.uint16)
    da[30:40, 50:120] = 0
    db = (da + 500).astype(np.uint16)
    db[:, 0:9] = 0
    for name, arr in (("a.u8", ia), ("b.u8", ib), ("a.u16", da), ("b.u16", db)):
        (tmp_path / name).write_bytes(arr.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(w), str(h)] + [str(tmp_path / n) for n in ("a.u8", "b.u8", "a.u16", "b.u16")] + [str(out)] +
                       (["legacy"] if arith == "legacy" else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    n1, n2, n3, n4 = (int(v) for v in np.frombuffer(b, np.int64, 4, 0))
    at = 32
    batch = np.frombuffer(b, capi.CLOUD_POINT, n1, at); at += 16 * n1
    info = np.frombuffer(b, capi.CLOUD_INFO, 3, at); at += 32 * 3
    dense = np.frombuffer(b, capi.CLOUD_POINT, n2, at); at += 16 * n2
    cand = np.frombuffer(b, capi.CLOUD_POINT, n3, at); at += 16 * n3
    recent = np.frombuffer(b, np.float32, 3 * n4, at).reshape(-1, 3); at += 12 * n4
    assert at == len(b)

    fl = float(np.float32(525.0) * np.float32(w) / np.float32(640.0))
    tr = M.Tracker(True, max_frames=4, n_levels=3, first_level=2, last_level=0)
    tr.InitializePyramid(w, h, np.array([[fl, 0, w / 2 - 0.5], [0, fl, h / 2 - 0.5], [0, 0, 1]], np.float32))
    fa, fb = M.Frame(ia, da), M.Frame(ib, db)
    pa = np.array([0, 0, 0, 1, 0.5, -0.25, 1.5], np.float32)
    pb = np.array([0, 0, 0.0871557, 0.9961947, -1.0, 0.75, 2.0], np.float32)
    pts, inf, call = tr.PointCloudBatch([fa, fb], np.stack([pa, pb]), capi.default_cloud_params(mode=1, stride=7, skip_invalid=1))
    assert 0 < inf[0]["n_points"] < inf[0]["n_selected"] and 0 < inf[1]["n_points"] < inf[1]["n_selected"]
    assert batch.tobytes() == pts.tobytes() and info[:2].tobytes() == inf.tobytes() and info[2].tobytes() == call.tobytes()
    vis = M.Visualizer(tr)
    vis.AddPointCloudFromRGBD(fa, pa)
    vis.AddPointCloudFromRGBD(fb, pb)
    assert vis.point_cloud_.size == 2 * -(-(w * h) // 100) and dense.tobytes() == vis.point_cloud_.tobytes()
    assert np.array_equal(vis.point_cloud_["tag"] >> 8, [0] * (n2 // 2) + [1] * (n2 // 2))
    tr.ApplyGradient(fa)
    tr.ObtainCandidatePoints(fa, 5.0)
    vis2 = M.Visualizer(tr)
    vis2.AddPointCloudFromRGBD(fa, pb)
    assert n3 == -(-fa.candidatePoints_[0].shape[0] // 100) > 0 and cand.tobytes() == vis2.point_cloud_.tobytes()
    m = M.Map(tr)
    m.AddPointCloudFromRGBD(fa)
    assert m.recent_cloud_points_.shape == (n4, 3) and recent.tobytes() == np.ascontiguousarray(m.recent_cloud_points_).tobytes()
    assert np.array_equal(m.recent_cloud_points_, fa.candidatePoints_[0][:, :3])
