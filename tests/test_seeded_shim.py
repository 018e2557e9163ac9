"""The seeded overloads of include/uw_tracker.hpp (EstimatePoseSeeded, EstimatePoseFeaturesBatch / EstimatePoseCandidatesBatch with
seeds, TrackingBatch with seeds, PredictSeeds) through tests/cpp/shim_seeded.cpp: compiled and linked without a GPU, and on the GPU
bit for bit what the Python mirror (uw-slam_amd/tracker.py) gives for the same frames and seeds."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import seeded_cases as SC
import tracking_ref as TR

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 256, 240, 4


def build_exe(path, native=True):
    if native:
        importlib.import_module("uw-slam_amd").build_native()
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_seeded.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


def test_shim_seeded_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_seeded")))


@pytest.mark.gpu
def test_shim_seeded_equals_the_python_mirror(O, synth, tmp_path):
    exe = build_exe(str(tmp_path / "shim_seeded"), native=False)   # against the library that is there: one g++ call
    intr = TR.INTR[(W, H)]
    frames = synth.render_sequence(W, H, *intr, N, seed=3)[0]
    seeds = SC.seeds(O, 2 * (N - 1))
    (tmp_path / "frames.u8").write_bytes(np.ascontiguousarray(frames, np.uint8).tobytes())
    (tmp_path / "seeds.f32").write_bytes(seeds.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(W), str(H)] + [repr(float(v)) for v in intr] + [str(N), str(tmp_path / "frames.u8"),
                                                                                 str(tmp_path / "seeds.f32"), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    P = N - 1
    block = 28 * P + 16 * P
    assert len(b) == 5 * block + 28 * P
    got = [(b[i * block:i * block + 28 * P], b[i * block + 28 * P:(i + 1) * block]) for i in range(5)]
    predicted = b[5 * block:]

    T = importlib.import_module("uw-slam_amd.tracker")
    tracker = T.Tracker(False, max_frames=2 * N)
    tracker.InitializePyramid(W, H, np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], np.float32))
    first, second = seeds[:P], seeds[P:]
    grid = np.array([[np.float32(W * (x + 1)) / np.float32(7.0), np.float32(H * (y + 1)) / np.float32(6.0)]
                     for y in range(5) for x in range(6)], np.float32)

    def fresh(keypoints=True):
        fr = [T.Frame(f, None, i) for i, f in enumerate(frames)]
        for f in fr:
            f.keypoints_ = grid.copy() if keypoints else np.zeros((0, 2), np.float32)
        return fr, [(fr[k], fr[k + 1]) for k in range(P)]

    def record(pairs, stats):
        return (b"".join(np.asarray(a.rigid_transformation_, np.float32).tobytes() for a, _ in pairs),
                b"".join(np.array([s["status"], s["iterations"], s["n_valid"]], np.int32).tobytes() + np.float32(s["error"]).tobytes()
                         for s in stats))

    want = []
    for handoff in (0, 1):
        fr, pairs = fresh()
        stats = []
        for k, (a, c) in enumerate(pairs):
            tracker.ApplyGradient(a)
            stats.append(tracker.EstimatePoseSeeded(a, c, first[k], handoff))
        want.append(record(pairs, stats))
    fr, pairs = fresh()
    for a, _ in pairs:
        tracker.ApplyGradient(a)
    want.append(record(pairs, tracker.EstimatePoseCandidatesBatch(pairs, seeds=first, handoff=1)))
    fr, pairs = fresh()
    for a, _ in pairs:
        tracker.ApplyGradient(a)
    want.append(record(pairs, tracker.EstimatePoseFeaturesBatch(pairs, seeds=first)))
    fr, pairs = fresh(keypoints=False)
    want.append(record(pairs, T.TrackingBatch(tracker, T.RobustMatcher(tracker), pairs, seeds=first)))
    for i, name in enumerate(("EstimatePoseSeeded 0", "EstimatePoseSeeded 1", "EstimatePoseCandidatesBatch", "EstimatePoseFeaturesBatch",
                              "TrackingBatch")):
        assert got[i] == want[i], name
    assert all(np.frombuffer(g[1], np.int32).reshape(P, 4)[:, 0].tolist() == [0] * P for g in got)
    assert got[0][0] != got[1][0]   # the hand-off choice shows
    assert predicted == tracker.PredictSeeds(first, second).tobytes()
    # a seeded TrackingBatch differs from the unseeded one in the poses alone
    fr, pairs = fresh(keypoints=False)
    unseeded = record(pairs, T.TrackingBatch(tracker, T.RobustMatcher(tracker), pairs))
    assert unseeded[0] != want[4][0]
    tracker._ctx.close()
