"""Semi-dense tracking for a batch of pairs (uwt_track_candidates_batch_async, uwt_estimate_pose_candidates_batch) on the CPU
side: declared, bound, exported, the ABI unchanged, and the C++ mirror's EstimatePoseCandidatesBatch compiles and links."""
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["uwt_track_candidates_batch_async", "uwt_estimate_pose_candidates_batch"]
ARITH_INDEPENDENT = True


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def test_candidates_entry_points_are_declared_bound_and_exported(capi):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uwt_[a-z0-9_]+)\s*\(", src))
    lib = capi.lib()
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.uwt_abi_version() == 4


def test_candidates_context_methods_exist(capi):
    for m in ("estimate_pose_candidates_batch", "track_candidates_batch_async"):
        assert callable(getattr(capi.Context, m)), m


def test_candidates_batch_mirror_compiles_and_links(capi, tmp_path):
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_candidates_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_candidates_batch.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
