"""CPU-side checks of the image-warp surface: include/uwt.h declares the entries and cites the reference, the library exports them,
uw-slam_amd.capi wraps them, and both mirrors carry the three methods.  No compute calls here."""
import importlib
import os
import re

import pytest

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["uwt_obtain_image_transformed", "uwt_warp_image_batch_async", "uwt_warp_image_batch", "uwt_warp_mosaic"]
METHODS = ["ObtainImageTransformed", "DebugShowWarpedPerspective", "WarpedImageBatch"]


@pytest.fixture(scope="module")
def capi():
    importlib.import_module("uw-slam_amd").build_native()
    return importlib.import_module("uw-slam_amd.capi")


def test_header_declares_and_library_exports_the_entries(capi):
    src = open(os.path.join(ROOT, "include", "uwt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert capi.lib().uwt_abi_version() == 4 and "#define UWT_ABI_VERSION 4" in code   # additions only
    # the contract is stated where the other entries cite the reference, with both deviations
    for phrase in ("src/Tracker.cpp:1473-1525", ":1694-1737", "largest i wins", "halves away from zero", "2^31 - 128",
                   "would read out of bounds", "atomicMax"):
        assert phrase in src, phrase


def test_quality_record_layout_matches_the_header(capi):
    src = open(os.path.join(ROOT, "include", "uwt.h")).read()
    body = re.search(r"typedef struct uwt_warp_quality \{(.*?)\} uwt_warp_quality;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", body)
    assert [n for _, n in fields] == list(capi.WARP_QUALITY.names)
    assert [capi.WARP_QUALITY[n].itemsize for _, n in fields] == [4 if t == "int32_t" else 8 for t, _ in fields]
    assert capi.WARP_QUALITY.itemsize == 48 == sum(4 if t == "int32_t" else 8 for t, _ in fields)
    io = re.search(r"typedef struct uwt_warp_image_io \{(.*?)\} uwt_warp_image_io;", src, flags=re.S).group(1)
    io = re.sub(r"/\*.*?\*/", "", io, flags=re.S)
    assert re.findall(r"\*\s+(\w+);", io) == [n for n, _ in capi.WarpImageIO._fields_]


def test_wrappers_and_mirrors_carry_the_methods(capi):
    for name in ("obtain_image_transformed", "warp_image_batch", "warp_image_batch_async", "warp_mosaic"):
        assert callable(getattr(capi.Context, name)), name
    tracker = importlib.import_module("uw-slam_amd.tracker")
    hpp = open(os.path.join(ROOT, "include", "uw_tracker.hpp")).read()
    for name in METHODS:
        assert callable(getattr(tracker.Tracker, name)), name
        assert re.search(r"\b%s\(" % name, hpp), name
    # the reference's argument order (include/Tracker.h:188, 257)
    import inspect
    assert list(inspect.signature(tracker.Tracker.ObtainImageTransformed).parameters)[1:] == [
        "_originalImage", "_candidatePoints", "_warpedPoints", "_outputImage"]
    assert list(inspect.signature(tracker.Tracker.DebugShowWarpedPerspective).parameters)[1:] == [
        "_image1", "_image2", "_imageWarped", "_lvl"]
    assert re.search(r"ObtainImageTransformed\(const ImageView& _originalImage, const std::vector<float>& _candidatePoints,\s*"
                     r"const std::vector<float>& _warpedPoints, std::vector<uint8_t>& _outputImage\)", hpp)


def test_tool_has_the_quality_switch():
    src = open(os.path.join(ROOT, "tools", "track_sequence.py")).read()
    assert "--quality" in src and "warp_image_batch" in src
