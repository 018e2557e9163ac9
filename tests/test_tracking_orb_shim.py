"""uw::Tracker::TrackingBatch with uw::RobustMatcher(&tracker, 1) (include/uw_tracker.hpp over uwt_tracking_orb_batch) through
tests/cpp/shim_tracking_orb.cpp: over the frames of a rendered sequence it leaves every frame field as the stage-by-stage loop of the
C++ mirror leaves it, and as the Python mirror's Tracking loop with RobustMatcher(detector=1) does."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import orb_ref as O
import tracking_ref as TR
from test_tracking_shim import read_run

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 240


def build_exe(path, native=True):
    if native:
        importlib.import_module("uw-slam_amd").build_native()
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_tracking_orb.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_shim_tracking_orb_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_tracking_orb")))


@pytest.mark.gpu
def test_shim_tracking_orb_equals_the_loops(synth, tmp_path):
    exe = build_exe(str(tmp_path / "shim_tracking_orb"), native=False)   # against the library that is there: one g++ call
    intr = TR.INTR[(W, H)]
    frames = synth.render_sequence(W, H, *intr, 5, seed=3)[0]
    (tmp_path / "frames.u8").write_bytes(np.ascontiguousarray(frames, np.uint8).tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(W), str(H)] + [repr(float(v)) for v in intr] + ["5", str(tmp_path / "frames.u8"), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    loop, loop_stats, o = read_run(b, 0, 5)
    batch, batch_stats, o = read_run(b, o, 5)
    assert o == len(b)
    assert [f[0] for f in loop] == [262, 163, 108, 379, 379]   # both paths of usekeypoints: detected, provided, provided, detected
    assert batch == loop and batch_stats == loop_stats
    # the Python mirror's loop over the same frames
    T = importlib.import_module("uw-slam_amd.tracker")
    tracker = T.Tracker(False, max_frames=6)
    tracker.InitializePyramid(W, H, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    rm = T.RobustMatcher(tracker, detector=1)
    fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
    for k in range(4):
        T.Tracking(tracker, rm, fr[k], fr[k + 1])
    tracker._ctx.close()
    for f, g in zip(fr, batch):
        assert (f.n_matches_, np.asarray(f.keypoints_, np.float32).tobytes(), np.asarray(f.orb_keypoints_, O.KEYPOINT).tobytes(),
                np.asarray(f.rigid_transformation_, np.float32).tobytes()) == g
