"""CPU-side checks of the batched table calls' options (uwt_table_options; uwt_*_features_batch_opt*, uwt_*_candidates_batch_opt*):
the five new symbols are declared in include/uwt.h, bound in capi.SYMBOLS and exported by the library, the struct is 32 bytes on
both sides, the ABI version has not moved, and the C++ mirror's overloads compile and link.  No compute calls here."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

ARITH_INDEPENDENT = True   # nothing here depends on the arithmetic set (tests/conftest.py): run once

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["uwt_default_table_options", "uwt_track_features_batch_opt_async", "uwt_estimate_pose_features_batch_opt",
       "uwt_track_candidates_batch_opt_async", "uwt_estimate_pose_candidates_batch_opt"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


def test_new_symbols_are_declared_bound_and_exported(capi):
    src = open(os.path.join(ROOT, "include", "uwt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.uwt_abi_version() == 4 and re.search(r"#define\s+UWT_ABI_VERSION\s+4\b", src)


def test_table_options_layout_and_defaults(capi):
    assert C.sizeof(capi.TableOptions) == 32
    assert [f[0] for f in capi.TableOptions._fields_] == ["weights", "sampler", "reserved"]
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwt.h")).read(), flags=re.S)
    m = re.search(r"typedef struct uwt_table_options \{(.*?)\} uwt_table_options;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int32_t weights; int32_t sampler; int32_t reserved[6];"
    o = capi.TableOptions(weights=7, sampler=7)
    o.reserved[3] = 5
    assert capi.lib().uwt_default_table_options(C.byref(o)) == 0 and bytes(o) == bytes(32)
    assert capi.lib().uwt_default_table_options(None) == capi.ERR_INVALID_ARG
    o = capi.table_options(weights=2, sampler=1)
    assert (o.weights, o.sampler, list(o.reserved)) == (2, 1, [0] * 6)


def test_python_layers_take_the_options(capi):
    tracker = importlib.import_module("uw-slam_amd.tracker")
    for fn in (capi.Context.estimate_pose_features_batch, capi.Context.track_features_batch_async,
               capi.Context.estimate_pose_candidates_batch, capi.Context.track_candidates_batch_async,
               tracker.Tracker.EstimatePoseFeaturesBatch, tracker.Tracker.EstimatePoseCandidatesBatch):
        par = inspect.signature(fn).parameters
        assert par["weights"].default is None and par["sampler"].default is None, fn


def test_existing_refusal_names_both_ways_out():
    """uwt_estimate_pose_candidates_batch still refuses a context with weights or a sampler; its message keeps the per-pair path
    and adds the new entries."""
    txt = open(os.path.join(ROOT, "uw-slam_amd", "csrc", "uwt_capi_tables.hip")).read()
    m = re.search(r"identity weights and the nearest sampler only;(.*?)\);", txt, flags=re.S)
    assert m and "uwt_estimate_pose_points" in m.group(1) and "uwt_estimate_pose_candidates_batch_opt" in m.group(1)


def test_cpp_mirror_compiles_and_links(capi, tmp_path):
    libdir = os.path.join(ROOT, "uw-slam_amd")
    exe = str(tmp_path / "shim_tables_robust")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_tables_robust.cpp"), "-o", exe,
                           "-L", libdir, "-luwt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "LINK 4", (out.returncode, out.stdout, out.stderr)
