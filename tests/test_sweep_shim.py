"""The C++ side of the depth sweep (tests/cpp/shim_sweep.cpp over include/uw_tracker.hpp and the C ABI): the mirror's SweepDepth compiles
and links, and on the GPU its bytes are the C ABI's."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import depth_sweep_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_exe(path, native=True):
    if native:
        importlib.import_module("uw-slam_amd").build_native()
    libdir = os.path.join(ROOT, "uw-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_sweep.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.one_arith
def test_shim_sweep_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_sweep")))


@pytest.mark.gpu
def test_shim_sweep_equals_the_c_abi(synth, tmp_path, arith):
    capi = importlib.import_module("uw-slam_amd.capi")
    exe = build_exe(str(tmp_path / "shim_sweep"), native=False)   # against the library that is there: one g++ call
    w, h = 64, 48
    fl = float(np.float32(525.0) * np.float32(w) / np.float32(640.0))
    intr = (fl, fl, w / 2 - 0.5, h / 2 - 0.5)
    ref = synth.texture(w, h, 33, sigma=1.5)
    poses = np.array([[0, 0, 0, 1, 0.2, 0.02, 0.0], [0, 0, 0, 1, -0.15, 0.05, 0.01]], np.float32)
    views = [DC.render_view(synth, ref, intr, np.zeros(3), poses[i, 4:], 1.0)[0] for i in range(2)]
    for name, img in (("ref", ref), ("v0", views[0]), ("v1", views[1])):
        (tmp_path / (name + ".u8")).write_bytes(img.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(w), str(h)] + [str(tmp_path / (n + ".u8")) for n in ("ref", "v0", "v1")] + [str(out)] +
                       (["legacy"] if arith == "legacy" else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    n = w * h
    assert len(b) == 2 * n + 2 * n + n + 64
    depth, cost = np.frombuffer(b, np.uint16, n, 0), np.frombuffer(b, np.uint16, n, 2 * n)
    outcome = np.frombuffer(b, np.uint8, n, 4 * n)
    info = np.frombuffer(b, capi.SWEEP_INFO, 1, 5 * n)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=4, max_pairs=1, n_levels=2, first_level=1, last_level=0))
    ctx.upload_frames(0, np.stack([ref] + views))
    ctx.build_pyramids(0, 3)
    ctx.apply_gradient(0, 1)
    want = ctx.sweep_depth([0], [[1, 2]], poses, capi.sweep_hypotheses(0.5, 2.5, 0.0002, 32))
    assert want["info"]["n_outcome"][0][capi.SWEEP_ESTIMATED] > 0
    assert depth.tobytes() == want["depth"].tobytes() and cost.tobytes() == want["cost"].tobytes()
    assert outcome.tobytes() == want["outcome"].tobytes() and info.tobytes() == want["info"].tobytes()
    ctx.close()
