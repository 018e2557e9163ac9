"""The point-cloud map without a device: the argument checks the library makes before it touches one, the struct layouts, the PLY
writer, and the flags of tools/track_sequence.py (without --cloud nothing changes)."""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

ARITH_INDEPENDENT = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("track_sequence", os.path.join(ROOT, "tools", "track_sequence.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_struct_sizes(capi):
    assert capi.CLOUD_POINT.itemsize == 16 and C.sizeof(capi.CloudParams) == 32 and capi.CLOUD_INFO.itemsize == 32
    assert capi.CloudParams.threshold.offset == 16 and capi.CloudParams.reserved.offset == 24
    assert capi.CLOUD_INFO.fields["offset"][1] == 16 and capi.CLOUD_INFO.fields["written"][1] == 24
    assert capi.CLOUD_POINT.fields["tag"][1] == 12


def test_default_params_are_the_reference_call(capi):
    p = capi.default_cloud_params()
    assert (p.mode, p.stride, p.skip_invalid, p.source, p.threshold, list(p.reserved)) == (0, 100, 0, 0, 20.0, [0, 0])
    assert capi.lib().uwt_default_cloud_params(None) == INVALID_ARG
    with pytest.raises(AttributeError):
        capi.default_cloud_params(strides=3)


def test_calls_without_a_context_are_refused(capi):
    lib = capi.lib()
    p = capi.default_cloud_params()
    buf = np.zeros(64, np.uint8)
    ptr = C.c_void_p(buf.ctypes.data)
    slots = (C.c_int32 * 1)(0)
    cnt = C.c_int64(-1)
    assert lib.uwt_point_cloud_batch_async(None, 1, slots, ptr, C.byref(p), ptr, C.c_int64(1), ptr) == INVALID_ARG
    assert lib.uwt_point_cloud_batch(None, 1, slots, ptr, C.byref(p), ptr, C.c_int64(1), ptr) == INVALID_ARG
    assert lib.uwt_point_cloud_points(None, 0, ptr, 1, ptr, C.byref(p), ptr, C.c_int64(1), C.byref(cnt)) == INVALID_ARG
    assert lib.uwt_accumulate_trajectory_device_async(None, ptr, 1, ptr, C.c_float(1.0), 0, ptr) == INVALID_ARG
    assert lib.uwt_accumulate_trajectory_device_from_async(None, ptr, 1, ptr, C.c_float(1.0), 0, ptr) == INVALID_ARG
    assert cnt.value == -1 and not buf.any()


def test_new_symbols_are_listed(capi):
    for name in ("uwt_default_cloud_params", "uwt_point_cloud_batch_async", "uwt_point_cloud_batch", "uwt_point_cloud_points",
                 "uwt_accumulate_trajectory_device_async", "uwt_accumulate_trajectory_device_from_async"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)


@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_round_trip(capi, tmp_path, binary):
    T = importlib.import_module("uw-slam_amd.trajectory")
    rng = np.random.default_rng(1)
    pts = np.zeros(257, capi.CLOUD_POINT)
    for k in "xyz":
        pts[k] = rng.normal(0, 10, 257).astype(np.float32)
    pts["x"][0], pts["y"][0], pts["z"][0] = np.float32(1e-30), np.float32(-3.4e38), np.float32(0.1)
    pts["tag"] = rng.integers(0, 256, 257).astype(np.uint32) | (np.arange(257, dtype=np.uint32) << 8)
    path = str(tmp_path / "cloud.ply")
    T.write_ply(path, pts, binary=binary)
    head = open(path, "rb").read(200).decode("ascii", "replace")
    assert head.startswith("ply\nformat %s 1.0\nelement vertex 257\n" % ("binary_little_endian" if binary else "ascii"))
    assert "property float x\nproperty float y\nproperty float z\nproperty uchar intensity\nend_header\n" in head
    v = T.read_ply(path)
    assert v.size == 257 and all(v[k].tobytes() == pts[k].tobytes() for k in "xyz")   # bit for bit, the ASCII form too
    assert np.array_equal(v["intensity"], pts["tag"] & 255)
    T.write_ply(path, np.stack([pts["x"], pts["y"], pts["z"]], 1), binary=binary)   # plain n x 3: intensity 0
    v = T.read_ply(path)
    assert v["x"].tobytes() == pts["x"].tobytes() and not v["intensity"].any()
    T.write_ply(path, np.zeros(0, capi.CLOUD_POINT), binary=binary)
    assert T.read_ply(path).size == 0


def test_track_sequence_flags(tool):
    base = ["--images", "rgb", "--fx", "525", "--fy", "525", "--cx", "319.5", "--cy", "239.5"]
    ap = tool.build_parser()
    a = ap.parse_args(base)
    assert a.cloud is None and a.cloud_stride == 100 and a.cloud_mode == "reference"   # without --cloud nothing is asked for
    today = dict(images="rgb", depth=None, fx=525.0, fy=525.0, cx=319.5, cy=239.5, width=640, height=480, distortion="", rectified_size="",
                 start=0, count=0, weights="identity", bilinear=False, arith="opencv", fixed_iters=0, groundtruth=None, euroc=False,
                 tum=False, live=False, detector="surf", chained=False, quality=False, out="trajectory")
    got = vars(a)
    assert {k: got[k] for k in today} == today and sorted(set(got) - set(today)) == ["cloud", "cloud_mode", "cloud_stride"]
    b = ap.parse_args(base + ["--cloud", "map.ply", "--cloud-stride", "7", "--cloud-mode", "world", "--live", "--chained"])
    assert (b.cloud, b.cloud_stride, b.cloud_mode) == ("map.ply", 7, "world")
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--cloud-mode", "elsewhere"])
    assert tool.CLOUD_MODES == {"reference": 0, "world": 1}
    assert tool.cloud_accumulation(0) == (40.0, False) and tool.cloud_accumulation(1) == (1.0, False)
