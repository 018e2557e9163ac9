"""Golden vectors dumped from the REAL reference (tools/ref_dump/): consumed when tests/golden/ref_<case>.npz exist.

The reference holds no test vectors of its own and cannot be built in this image (no OpenCV / Eigen), so no such file is
committed yet — parity with the reference stays unpinned until a maintainer runs tools/ref_dump against an OpenCV-3.2 build
(README there) and commits the result.  What runs here regardless: the insertion points of the instrumentation are found
in a Tracker.cpp-shaped source (built here from the tool's own patterns), the input export round-trips, and the whole
dump -> loader -> comparison pipeline is exercised on a dump fabricated from the oracle in the reference-side format.
"""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "ref_dump", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ulps(a, b):
    """Distance in units of the last place between two f32 arrays (same sign assumed where it matters)."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def _pose_distance(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    qa, qb = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])
    dot = min(1.0, abs(float(qa @ qb)))
    return 2.0 * np.arccos(dot), float(np.linalg.norm(a[4:] - b[4:]))


PICK_X = np.array([-0.5, -0.5, -0.5, 0.5, 0, 0, 0], np.float32)   # R = [[0,1,0],[0,0,1],[1,0,0]]: row 2 of the rigid product picks X
PICK_Y = np.array([0.5, 0.5, 0.5, 0.5, 0, 0, 0], np.float32)      # the transpose: row 2 picks Y


def _under_both_sets(O, fn):
    """fn() evaluated with the oracle's per-stage switch at either arithmetic set: {"opencv": value, "legacy": value}."""
    out = {}
    prev = O.set_arith(O.ARITH_OPENCV)
    try:
        for name, a in (("opencv", O.ARITH_OPENCV), ("legacy", O.ARITH_LEGACY)):
            O.set_arith(a)
            out[name] = fn()
    finally:
        O.set_arith(prev)
    return out


def _verdict(ulps):
    """which arithmetic set a reference record equals bit for bit: 'opencv', 'legacy', 'both' or 'neither (<ulps>)'"""
    hit = [k for k in ("opencv", "legacy") if ulps[k] == 0]
    return "both" if len(hit) == 2 else hit[0] if hit else "neither (opencv %d ulps, legacy %d ulps)" % (ulps["opencv"], ulps["legacy"])


UNIT_CAMERA = dict(w=64, h=64, fx=1.0, fy=1.0, cx=0.0, cy=0.0, invfx=1.0, invfy=1.0)


def unit_level(O):
    L = O.Level()
    for k, v in UNIT_CAMERA.items():
        setattr(L, k, v)
    return L


def fold_verdict(O, ref):
    """The `foldprobe` record (tools/ref_dump/fold_probe.h): how the build's gemm folds the four partial sums of the rigid product.
    'published' = "s0 += s1 + s2 + s3" (the oracle's and the kernels' fold 0), 'left_to_right' = ((s0 + s1) + s2) + s3;
    'matrix differs' when row 2 of the build's rigid matrix is not the oracle's (S6 comes first then); 'neither' otherwise."""
    r, pt, lo, hi, out = ref["foldprobe"][:3], ref["foldprobe"][3:6], ref["foldprobe"][6], ref["foldprobe"][7], ref["foldprobe"][8]
    T = O.se3_matrix(ref["testpose"]).reshape(4, 4)
    if not np.array_equal(T[2, :3].view(np.uint32), np.asarray(r, np.float32).view(np.uint32)):
        return "matrix differs (S6: the quaternion-to-matrix arithmetic), fold undetermined"
    pts = np.array([[pt[0], pt[1], pt[2], 0.0]], np.float32)
    mine = {}
    prev_a = O.set_arith(O.ARITH_OPENCV)
    try:
        for fold in (0, 1):
            prev = O.set_gemm_fold(fold)
            try:
                mine[fold] = O.warp(pts, ref["testpose"], unit_level(O))[0][2]
            finally:
                O.set_gemm_fold(prev)
    finally:
        O.set_arith(prev_a)
    assert mine[0] == lo and mine[1] == hi, (mine, lo, hi)   # the construction itself, re-checked against the oracle
    return "published" if out == lo else "left_to_right" if out == hi else "neither (%s)" % float(out).hex()


def diagnose_arithmetic(O, ref, pair, p):
    """The records that separate the two arithmetic sets (uwt_oracle.h G1-G3 against S1, S3, S4), each compared with the oracle
    under BOTH sets — what a maintainer's first real dump says about the OpenCV build it came from:
      unproject   column 2 of WarpFunction at the axis permutations = X * z, Y * z of Tracker.cpp:1439-1444
                  (G3: x * invfx + beta  /  legacy: (x - cx) * invfx)
      rigid_row   column 2 of WarpFunction at the generic test pose = one row of rigid * points.t() before the divide (:1450)
                  (G1: double accumulation  /  S1: f32 FMA chain) — meaningful once `unproject` is settled
      delta       "A.inv() * b" from the reference's A and b (:564)   (G2: cv::solve  /  S3 + S4: inverse, then product)
      delta_unfolded   the same through two statements: must be the inverse-then-product whatever the build folds
      rigid_fold  the one-point fold probe (fold_verdict)
    Returns {record: verdict string}; asserts nothing."""
    h, w = pair["ref"].shape
    depth = pair["depth"] if "depth" in pair.files else None
    rep = {}
    img, dep = pair["ref"], depth
    un, rr = {"opencv": 0, "legacy": 0}, {"opencv": 0, "legacy": 0}
    seen_un = seen_rr = False
    for l in range(p.n_levels):
        if l:
            img = O.halve_u8(img)
            dep = O.halve_u16(dep) if dep is not None else None
        pts = O.dense_points(dep, img.shape[1], img.shape[0], l)
        L = O.level_intrinsics(p, l)
        for key, pose in (("stage_unpx%d" % l, PICK_X), ("stage_unpy%d" % l, PICK_Y)):
            if key in ref.files:
                seen_un = True
                mine = _under_both_sets(O, lambda: O.warp(pts, pose, L)[:, 2])
                for k in un:
                    un[k] = max(un[k], int(_ulps(ref[key].reshape(-1, 4)[:, 2], mine[k]).max()))
        if "stage_warp%d" % l in ref.files and "testpose" in ref.files:
            seen_rr = True
            mine = _under_both_sets(O, lambda: O.warp(pts, ref["testpose"], L)[:, 2])
            for k in rr:
                rr[k] = max(rr[k], int(_ulps(ref["stage_warp%d" % l].reshape(-1, 4)[:, 2], mine[k]).max()))
    if "foldprobe" in ref.files and ref["foldprobe"].shape == (9,):
        rep["rigid_fold"] = fold_verdict(O, ref)
    if seen_un:
        rep["unproject"] = _verdict(un)
    if seen_rr:
        rep["rigid_row"] = _verdict(rr)
    upd = [i for i in range(len(ref["level"])) if int(ref["updated"][i])]
    if upd:
        dl = {"opencv": 0, "legacy": 0}
        for i in upd:
            mine = _under_both_sets(O, lambda: O.solve_delta(ref["A"][i].reshape(36), ref["b"][i]))
            for k in dl:
                dl[k] = max(dl[k], int(_ulps(ref["delta"][i], mine[k]).max()))
        rep["delta"] = _verdict(dl)
        if "delta_unfolded" in ref.files:
            prev = O.set_arith(O.ARITH_LEGACY)
            try:
                u = max(int(_ulps(ref["delta_unfolded"][i], O.solve_delta(ref["A"][i].reshape(36), ref["b"][i])).max()) for i in upd)
            finally:
                O.set_arith(prev)
            rep["delta_unfolded_vs_inverse_then_product_ulps"] = u
    return rep


def compare_with_oracle(O, ref, pair):
    """ref: a loaded ref_<case>.npz; pair: the tests/golden/pair_<case>.npz it was dumped from.  Integer stages and counts
    must be identical; float records are reported in ulps; the final pose must meet the north-star tolerance
    (<= 1e-4 rad, <= 1e-4 m).  Returns the report."""
    h, w = pair["ref"].shape
    fx, fy, cx, cy = [float(v) for v in pair["intr"]]
    depth = pair["depth"] if "depth" in pair.files else None
    p = O.default_params(w, h, fx, fy, cx, cy, has_depth=int(depth is not None))
    rep = {}
    img, dep = pair["ref"], depth
    for l in range(p.n_levels):
        if l:
            img = O.halve_u8(img)
            dep = O.halve_u16(dep) if dep is not None else None
        hl, wl = img.shape
        k = "stage_img%d" % l
        if k in ref.files:
            assert np.array_equal(ref[k].reshape(hl, wl), img), "pyramid level %d (cv::resize vs 2x2 mean)" % l
        if dep is not None and "stage_dep%d" % l in ref.files:
            assert np.array_equal(ref["stage_dep%d" % l].reshape(hl, wl), dep), "depth pyramid level %d" % l
        gx, gy = O.scharr3(img)
        if "stage_gx%d" % l in ref.files:
            assert np.array_equal(ref["stage_gx%d" % l].reshape(hl, wl), gx), "gradientX_ level %d (cv::Scharr scale 3)" % l
            assert np.array_equal(ref["stage_gy%d" % l].reshape(hl, wl), gy), "gradientY_ level %d" % l
        pts = O.dense_points(dep, wl, hl, l)
        if "stage_pts%d" % l in ref.files:
            assert np.array_equal(ref["stage_pts%d" % l].reshape(-1, 4).view(np.uint32), pts.view(np.uint32)), "candidatePoints_ level %d" % l
        if "stage_warp%d" % l in ref.files and "testpose" in ref.files:
            mine = O.warp(pts, ref["testpose"], O.level_intrinsics(p, l))
            rep["warp_ulps_l%d" % l] = int(_ulps(ref["stage_warp%d" % l].reshape(-1, 4)[:, :3], mine[:, :3]).max())
    st, pose, tr = O.align_pair(p, pair["ref"], pair["tgt"], depth, want_trace=True)
    assert st == 0
    n = len(ref["level"])
    rep["evaluations"] = (n, len(tr))
    assert n == len(tr), "number of evaluations: reference %d, oracle %d" % (n, len(tr))
    for i, t in enumerate(tr):
        assert (int(ref["level"][i]), int(ref["iter"][i]), int(ref["exited"][i])) == (t["level"], t["iter"], t["exited"]), i
        assert int(ref["n_valid"][i]) == t["n_valid"] and int(ref["sum_r2"][i]) == t["sum_r2"], (i, "valid points / sum r^2")
    upd = [i for i in range(n) if int(ref["updated"][i])]
    for k in ("A", "b", "delta", "pose"):
        mine = np.stack([tr[i][k] for i in upd]) if upd else np.zeros(0, np.float32)
        rep[k + "_ulps"] = int(_ulps(ref[k][upd].reshape(mine.shape), mine).max()) if upd else 0
    rep["error_ulps"] = int(_ulps(ref["error"], np.array([t["error"] for t in tr], np.float32)).max())
    rep["final_rot_rad"], rep["final_trans_m"] = _pose_distance(ref["final"], pose)
    rep["final_bitwise"] = bool(np.array_equal(np.asarray(ref["final"], np.float32).view(np.uint32), pose.view(np.uint32)))
    rep["arithmetic"] = diagnose_arithmetic(O, ref, pair, p)
    assert rep["final_rot_rad"] <= 1e-4 and rep["final_trans_m"] <= 1e-4, rep
    return rep


_PROBE_CLI = None


def fold_probe(row):
    """tools/ref_dump/fold_probe.h run on one matrix row through tests/cpp/fold_probe_cli.cpp: (x, y, z, lo, hi) or None"""
    global _PROBE_CLI
    import subprocess
    import tempfile
    if _PROBE_CLI is None:
        exe = os.path.join(tempfile.mkdtemp(prefix="uwt_probe_"), "fold_probe_cli")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tools", "ref_dump"),
                               os.path.join(ROOT, "tests", "cpp", "fold_probe_cli.cpp"), "-o", exe])
        _PROBE_CLI = exe
    t = subprocess.run([_PROBE_CLI] + [float(v).hex() for v in np.asarray(row, np.float32)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in t[1:]], np.float32) if int(t[0]) else None


def fabricate_dump(O, pair, name, out_dir):
    """The oracle's own results written in the reference-side formats (ref_dump_hooks.h records + raw stage files)."""
    h, w = pair["ref"].shape
    fx, fy, cx, cy = [float(v) for v in pair["intr"]]
    depth = pair["depth"] if "depth" in pair.files else None
    p = O.default_params(w, h, fx, fy, cx, cy, has_depth=int(depth is not None))
    testpose = O.se3_exp(np.array([0.01, -0.02, 0.015, 0.004, -0.003, 0.002], np.float32))
    img, tgt, dep = pair["ref"], pair["tgt"], depth
    for l in range(p.n_levels):
        if l:
            img, tgt = O.halve_u8(img), O.halve_u8(tgt)
            dep = O.halve_u16(dep) if dep is not None else None
        gx, gy = O.scharr3(img)
        pts = O.dense_points(dep, img.shape[1], img.shape[0], l)
        pre = os.path.join(out_dir, "%s_" % name)
        img.tofile(pre + "img%d.u8" % l); tgt.tofile(pre + "tgt%d.u8" % l)
        gx.tofile(pre + "gx%d.i16" % l); gy.tofile(pre + "gy%d.i16" % l)
        pts.tofile(pre + "pts%d.f32" % l)
        O.warp(pts, testpose, O.level_intrinsics(p, l)).tofile(pre + "warp%d.f32" % l)
        O.warp(pts, PICK_X, O.level_intrinsics(p, l)).tofile(pre + "unpx%d.f32" % l)
        O.warp(pts, PICK_Y, O.level_intrinsics(p, l)).tofile(pre + "unpy%d.f32" % l)
        if dep is not None:
            dep.tofile(pre + "dep%d.u16" % l)
    st, pose, tr = O.align_pair(p, pair["ref"], pair["tgt"], depth, want_trace=True)
    hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v, np.float32).ravel())
    with open(os.path.join(out_dir, "dump.txt"), "a") as f:
        f.write("case %s\ntestpose %s\n" % (name, hx(testpose)))
        fp = fold_probe(O.se3_matrix(testpose).reshape(4, 4)[2, :3])
        if fp is not None:   # what the driver writes: the probe built for the matrix, and the (here: the oracle's) warped z
            z = O.warp(np.array([[fp[0], fp[1], fp[2], 0.0]], np.float32), testpose, unit_level(O))[0][2]
            f.write("foldprobe row %s pt %s lo %s hi %s out %s\n" % (hx(O.se3_matrix(testpose).reshape(4, 4)[2, :3]), hx(fp[:3]), hx(fp[3:4]), hx(fp[4:5]), hx([z])))
        for t in tr:
            f.write("eval %d %d %d %.17g %s\n" % (t["level"], t["iter"], t["n_valid"], float(t["sum_r2"]), hx([t["error"]])))
            if t["exited"]:
                f.write("exit\n")
            else:
                prev = O.set_arith(O.ARITH_LEGACY)   # "Mat Ai = A.inv(); Mat d = Ai * b;": the inverse formed, then multiplied
                d2 = O.solve_delta(t["A"], t["b"])
                O.set_arith(prev)
                f.write("solve A %s b %s delta %s\nsolve2 delta %s\npose %s\n" % (hx(t["A"]), hx(t["b"]), hx(t["delta"]), hx(d2), hx(t["pose"])))
        f.write("final %s\n" % hx(pose))
    return pose


# A source shaped like the reference's src/Tracker.cpp around Tracker::EstimatePose, written for this test: one statement for
# each insertion point of tools/ref_dump/instrument.py, and decoys it must leave alone (a commented-out statement inside the
# function, the same statements in the definitions before and after it).
HOOK_STATEMENTS = ["error = errorMat.at<float>(0, 0);", "if (error >= last_error) {", "deltaMat = A.inv() * b;",
                   "current_pose = current_pose * SE3::exp(deltaVector);", "_previous_frame->rigid_transformation_ = current_pose;"]
TRACKER_SHAPED = """#include "Tracker.h"
void Tracker::WarpFunction(Mat points, SE3 rigid, int lvl) {
    deltaMat = A.inv() * b;
}
void Tracker::EstimatePose(Frame* _previous_frame, Frame* _current_frame) {
    SE3 current_pose = SE3(_previous_frame->rigid_transformation_);
    for (int lvl = 4; lvl >= 1; lvl--) {
        float last_error = FLT_MAX;
        for (int k = 0; k < 50; k++) {
            // error = errorMat.at<float>(0, 0);
            %s
            %s
                break;
            }
            Mat A = J.t() * J;
            Mat b = -J.t() * Residuals;
            %s
            %s
            last_error = error;
        }
    }
    %s
}
Mat Tracker::AddPatchPointsFeatures(Mat candidatePoints, int lvl) {
    current_pose = current_pose * SE3::exp(deltaVector);
}
""" % tuple(HOOK_STATEMENTS)


def test_instrumentation_finds_every_insertion_point():
    ins = _tool("instrument")
    text = TRACKER_SHAPED
    assert len(HOOK_STATEMENTS) == len(ins.HOOKS)
    out = ins.instrument(text)
    added = [l for l in out.split("\n") if "tools/ref_dump" in l]
    assert len(added) == len(ins.HOOKS) + 1                      # the hooks and the #include
    # nothing else changes: removing the added lines gives the file back
    assert "\n".join(l for l in out.split("\n") if "tools/ref_dump" not in l) == text
    # each hook right behind its statement inside EstimatePose, at the statement's indentation
    lines = out.split("\n")
    for stmt, (_, hook) in zip(HOOK_STATEMENTS, ins.HOOKS):
        i = next(i for i, l in enumerate(lines) if l.strip() == stmt and "EstimatePose" in "".join(lines[:i]) and "AddPatchPointsFeatures" not in "".join(lines[:i]))
        assert lines[i + 1] == lines[i][:len(lines[i]) - len(lines[i].lstrip())] + hook + "   // tools/ref_dump", (stmt, lines[i + 1])
    # an insertion point that is missing (or found twice) is an error, not a silently uninstrumented copy
    with pytest.raises(SystemExit):
        ins.instrument(text.replace(HOOK_STATEMENTS[2], "deltaMat = solve(A, b);"))
    with pytest.raises(SystemExit):
        ins.instrument(text.replace("last_error = error;", HOOK_STATEMENTS[0]))


def test_driver_passes_a_syntax_check_against_interface_stubs():
    """tools/ref_dump/ref_dump.cpp is built by a maintainer against the real reference (OpenCV, Eigen, Sophus, the reference's
    headers) — none of which exist here.  tests/cpp/stubs/ref/ declares only the members the driver and its hooks touch, so that
    at least the parser and overload resolution have seen the file."""
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "stubs", "ref"),
                        "-I", os.path.join(ROOT, "tools", "ref_dump"), os.path.join(ROOT, "tools", "ref_dump", "ref_dump.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_input_export_round_trips(tmp_path):
    from PIL import Image
    exp = _tool("export_inputs")
    old = sys.argv
    sys.argv = ["export_inputs.py", str(tmp_path)]
    try:
        exp.main()
    finally:
        sys.argv = old
    cases = [l.split() for l in open(tmp_path / "cases.txt").read().splitlines()]
    names = [c[0] for c in cases]
    assert "pair_160x96_ref5" in names and "pair_160x96_ref5_depth" in names and "pair_160x96_fixed" not in names
    for c in cases:
        d = np.load(os.path.join(GOLDEN, c[0] + ".npz"))
        assert np.array_equal(np.asarray(Image.open(tmp_path / c[0] / "ref.png")), d["ref"])
        assert np.array_equal(np.asarray(Image.open(tmp_path / c[0] / "tgt.png")), d["tgt"])
        assert (int(c[1]), int(c[2])) == d["ref"].shape[::-1] and np.allclose([float(v) for v in c[3:7]], d["intr"])
        if int(c[7]):
            dp = np.asarray(Image.open(tmp_path / c[0] / "depth.png"))
            assert dp.dtype == np.uint16 and np.array_equal(dp, d["depth"])


def test_axis_permutation_poses_expose_the_unprojection_exactly(O, arith):
    """WarpFunction at q = (-+1/2, -+1/2, -+1/2, 1/2): the rigid matrix has entries 0 and 1 only, so row 2 of rigid * points.t()
    is X * z (resp. Y * z) whatever the gemm accumulates in — the two sets differ there only through the unprojection."""
    assert np.array_equal(O.se3_matrix(PICK_X)[:3, :3], np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float32))
    assert np.array_equal(O.se3_matrix(PICK_Y)[:3, :3], np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float32))
    p = O.default_params(160, 96, 131.25, 131.25, 79.5, 47.5)
    rng = np.random.default_rng(5)
    dep = rng.integers(1, 20000, (48, 80)).astype(np.uint16)
    pts = O.dense_points(dep, 80, 48, 1)
    L = O.level_intrinsics(p, 1)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    if arith == "opencv":
        X = x * np.float32(L.invfx) + np.float32(-np.float64(L.cx) * np.float64(L.invfx))
        Y = y * np.float32(L.invfy) + np.float32(-np.float64(L.cy) * np.float64(L.invfy))
    else:
        X = (x - np.float32(L.cx)) * np.float32(L.invfx)
        Y = (y - np.float32(L.cy)) * np.float32(L.invfy)
    assert np.array_equal(O.warp(pts, PICK_X, L)[:, 2], (X * z).astype(np.float32))
    assert np.array_equal(O.warp(pts, PICK_Y, L)[:, 2], (Y * z).astype(np.float32))


def test_dump_loader_and_comparison_on_a_fabricated_dump(tmp_path, O, arith):
    """The pipeline a real dump goes through, fed with the oracle's own numbers in the reference-side format: every
    comparison must come out exact (0 ulps), which checks the formats, the loader and the comparison — not parity."""
    load = _tool("load_dump")
    out = tmp_path / "dump"; out.mkdir()
    gold = tmp_path / "golden"; gold.mkdir()
    for name in ("pair_160x96_ref5", "pair_160x96_ref5_depth"):
        fabricate_dump(O, np.load(os.path.join(GOLDEN, name + ".npz")), name, str(out))
    old = sys.argv
    sys.argv = ["load_dump.py", str(out), str(gold)]
    try:
        load.main()
    finally:
        sys.argv = old
    for name in ("pair_160x96_ref5", "pair_160x96_ref5_depth"):
        ref = np.load(gold / ("ref_" + name + ".npz"))
        rep = compare_with_oracle(O, ref, np.load(os.path.join(GOLDEN, name + ".npz")))
        assert rep["final_bitwise"] and all(v == 0 for k, v in rep.items() if k.endswith("_ulps")), rep
        # the diagnosis names the set the (fabricated) dump was made under, record by record
        ar = rep["arithmetic"]
        assert ar["unproject"] in (arith, "both") and ar["rigid_row"] == arith and ar["delta"] in (arith, "both"), ar
        assert ar["delta_unfolded_vs_inverse_then_product_ulps"] == 0, ar
        # (the legacy set has no partial sums: its f32 FMA chain lands on the probe's upper value)
        assert ar["rigid_fold"] == ("published" if arith == "opencv" else "left_to_right"), ar
    # a perturbed record is caught: one more valid point in one evaluation
    bad = dict(np.load(gold / "ref_pair_160x96_ref5.npz"))
    bad["n_valid"] = bad["n_valid"].copy(); bad["n_valid"][1] += 1
    np.savez(tmp_path / "bad.npz", **bad)
    with pytest.raises(AssertionError):
        compare_with_oracle(O, np.load(tmp_path / "bad.npz"), np.load(os.path.join(GOLDEN, "pair_160x96_ref5.npz")))


@pytest.mark.one_arith
def test_fold_probe_separates_the_two_folds(O):
    """fold_probe.h builds, for the rigid matrix of a generic pose, a point whose warped z is `lo` under the published fold and
    `hi` = the next float under the left-to-right one — checked here against the oracle for a few poses."""
    rng = np.random.default_rng(5)
    for i in range(4):
        xi = np.array([0.01, -0.02, 0.015, 0.004, -0.003, 0.002], np.float32) if i == 0 else rng.normal(0, 0.05, 6).astype(np.float32)
        pose = O.se3_exp(xi)
        fp = fold_probe(O.se3_matrix(pose).reshape(4, 4)[2, :3])
        assert fp is not None
        assert fp[4] == np.nextafter(fp[3], np.float32(4))
        pts = np.array([[fp[0], fp[1], fp[2], 0.0]], np.float32)
        for fold, want in ((0, fp[3]), (1, fp[4])):
            prev = O.set_gemm_fold(fold)
            try:
                assert O.warp(pts, pose, unit_level(O))[0][2] == want
            finally:
                O.set_gemm_fold(prev)


REF_FILES = sorted(glob.glob(os.path.join(GOLDEN, "ref_*.npz")))


@pytest.mark.skipif(not REF_FILES, reason="no tests/golden/ref_*.npz: nobody has run tools/ref_dump against the real reference yet")
@pytest.mark.parametrize("path", REF_FILES)
def test_oracle_against_reference_vectors(path, O):
    name = os.path.basename(path)[len("ref_"):-len(".npz")]
    rep = compare_with_oracle(O, np.load(path), np.load(os.path.join(GOLDEN, name + ".npz")))
    print(name, rep)


@pytest.mark.gpu
@pytest.mark.skipif(not REF_FILES, reason="no tests/golden/ref_*.npz: nobody has run tools/ref_dump against the real reference yet")
@pytest.mark.parametrize("path", REF_FILES)
def test_hip_path_against_reference_vectors(path):
    import importlib
    capi = importlib.import_module("uw-slam_amd.capi")
    name = os.path.basename(path)[len("ref_"):-len(".npz")]
    ref, pair = np.load(path), np.load(os.path.join(GOLDEN, name + ".npz"))
    h, w = pair["ref"].shape
    depth = pair["depth"] if "depth" in pair.files else None
    ctx = capi.Context(capi.default_params(w, h, *[float(v) for v in pair["intr"]], max_frames=2, max_pairs=1,
                                           has_depth=int(depth is not None)))
    ctx.upload_frames(0, np.stack([pair["ref"], pair["tgt"]]), None if depth is None else np.stack([depth, depth]))
    ctx.build_pyramids(0, 2)
    ctx.apply_gradient(0, 2)
    poses, stats = ctx.estimate_pose_batch([0], [1], raise_on_pair_failure=True)
    rot, trans = _pose_distance(ref["final"], poses[0])
    assert rot <= 1e-4 and trans <= 1e-4, (rot, trans)       # north-star tolerance against the reference's own pose
    assert stats[0]["iterations"] == len(ref["level"])
    ctx.close()
