"""The C++ side of the image warp (tests/cpp/shim_warp_image.cpp over include/uw_tracker.hpp and the C ABI): the mirror's
ObtainImageTransformed, DebugShowWarpedPerspective and WarpedImageBatch compile and link, and on the GPU their bytes are the C ABI's."""
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
                           os.path.join(ROOT, "tests", "cpp", "shim_warp_image.cpp"), "-o", path,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return path


@pytest.mark.one_arith
def test_shim_warp_image_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(str(tmp_path / "shim_warp_image")))


@pytest.mark.gpu
def test_shim_warp_image_equals_the_c_abi(synth, tmp_path, arith):
    capi = importlib.import_module("uw-slam_amd.capi")
    exe = build_exe(str(tmp_path / "shim_warp_image"), native=False)   # against the library that is there: one g++ call
    w, h = 160, 96
    ref, tgt, _, _, _ = synth.render_pair(w, h, 131.25, 131.25, 79.5, 47.5, seed=5)
    (tmp_path / "ref.u8").write_bytes(ref.tobytes())
    (tmp_path / "tgt.u8").write_bytes(tgt.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(w), str(h), str(tmp_path / "ref.u8"), str(tmp_path / "tgt.u8"), str(out)] +
                       (["legacy"] if arith == "legacy" else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = out.read_bytes()
    n = w * h
    assert len(b) == 2 * n + 48 + 2 * n + 4 * n
    warped, valid = np.frombuffer(b, np.uint8, n, 0), np.frombuffer(b, np.uint8, n, n)
    quality = np.frombuffer(b, capi.WARP_QUALITY, 1, 2 * n)
    out_img, out_valid = np.frombuffer(b, np.uint8, n, 2 * n + 48), np.frombuffer(b, np.uint8, n, 3 * n + 48)
    mosaic = np.frombuffer(b, np.uint8, 4 * n, 4 * n + 48)
    fl = np.float32(525.0) * np.float32(w) / np.float32(640.0)
    ctx = capi.Context(capi.default_params(w, h, float(fl), float(fl), w / 2 - 0.5, h / 2 - 0.5, max_frames=2, max_pairs=1, n_levels=3,
                                           first_level=2, last_level=0))
    ctx.upload_frames(0, np.stack([ref, tgt]))
    ctx.build_pyramids(0, 2)
    pose = np.array([[0, 0, 0, 1, 0.02, -0.01, 0.3]], np.float32)
    want = ctx.warp_image_batch([0], [1], pose)
    assert warped.tobytes() == want["warped"].tobytes() and valid.tobytes() == want["valid"].tobytes()
    assert quality.tobytes() == want["quality"].tobytes()
    # the explicit form over the same rows: the same mask, the same bytes where a row landed, the pre-filled 7 elsewhere
    assert out_valid.tobytes() == valid.tobytes()
    assert np.array_equal(out_img, np.where(valid == 1, warped, 7))
    assert mosaic.tobytes() == ctx.warp_mosaic(0, 1, 0, want["warped"][0]).tobytes()
    ctx.close()
