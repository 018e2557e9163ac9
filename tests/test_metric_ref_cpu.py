"""The metric Jacobian's restatement (tests/metric_ref.py) pinned on the CPU: its Jw is the closed form and the reference's expression
with the 3-D point substituted, its row product is the oracle's own in both arithmetic sets, with the mode off it is the oracle, it
recovers the rendered rotation where the reference Jacobian does not, and the ABI and the mirrors carry the mode."""
import ctypes
import importlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import metric_ref as MR
import seeded_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def random_warped(O, n=4000, seed=5):
    """n valid warped points (inside the level, z2 > 0) of level 1 of a 200 x 150 camera with fx != fy"""
    p = O.default_params(200, 150, 171.3, 168.9, 101.2, 73.6, n_levels=3)
    L = O.level_intrinsics(p, 1)
    rng = np.random.default_rng(seed)
    x2 = rng.uniform(0.01, L.iw - 0.01, n).astype(f32)
    y2 = rng.uniform(0.01, L.ih - 0.01, n).astype(f32)
    z2 = rng.uniform(0.3, 6.0, n).astype(f32)
    return L, x2, y2, z2


# ---- 1. the contract is the closed form -----------------------------------------------------------------------------------------------
@pytest.mark.one_arith
def test_jw_is_the_closed_form(O):
    """every entry within 16 * 2^-24 relative of the closed form in f64 (at most 8 roundings per entry — x2 - cx, * invfx, 1 / z2 and up
    to five products and sums — doubled), fx != fy, factors (0.5, 1.25); and the closed form is the reference's expression with
    X = xn * z2, Y = yn * z2 in place of x2, y2 (f64 against f64: 1e-12 relative)"""
    L, x2, y2, z2 = random_warped(O)
    assert L.fx != L.fy
    zf, af = 0.5, 1.25
    got = MR.jw_terms(x2, y2, z2, L, zf, af)
    want = MR.jw_closed_f64(x2, y2, z2, L, zf, af)
    sub = MR.jw_reference_substituted_f64(x2, y2, z2, L, zf, af)
    worst = 0.0
    for row in range(2):
        for k in range(5):
            g, w, s = got[row][k].astype(np.float64), want[row][k], sub[row][k]
            assert np.all(w != 0)
            rel = np.abs(g - w) / np.abs(w)
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 16 * 2.0 ** -24, (row, k, rel.max())
            assert (np.abs(s - w) / np.abs(w)).max() <= 1e-12, (row, k)
    print("worst relative error %.3g (bound %.3g)" % (worst, 16 * 2.0 ** -24))
    # unit factors are multiplied in and change nothing; the reference's own Jw differs from the metric one in columns 2..5 only
    unit = MR.jw_terms(x2, y2, z2, L, 1.0, 1.0)
    iz = (f32(1) / z2)
    assert np.array_equal(unit[0][0], f32(L.fx) * iz) and np.array_equal(unit[1][0], f32(L.fy) * iz)
    assert not np.array_equal(unit[0][3], (f32(L.fx) * (f32(1) + ((x2 * x2) * iz) * iz)))


def test_fma32_is_exact():
    """fma32 against exact rational arithmetic rounded once, on products that cancel against the addend, ties and plain cases"""
    rng = np.random.default_rng(3)
    n = 3000
    a = rng.integers(-20000, 20000, n).astype(f32)                        # gradients
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    c = (a * rng.standard_normal(n).astype(f32) * f32(3)).astype(f32)
    c[::3] = -(a[::3] * b[::3])                                           # near-total cancellation
    c[1::7] = (a[1::7] * b[1::7]) * f32(2.0 ** 24)                         # the product decides a tie of the addend
    got = MR.fma32(a, b, c)
    double_rounded = 0
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = f32(exact)   # Fraction -> float64 -> float32 rounds twice: redo it exactly below where that can matter
        lo, hi = np.nextafter(want, f32(-np.inf)), np.nextafter(want, f32(np.inf))
        best = min((lo, want, hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i].tobytes() == f32(best).tobytes(), (i, a[i], b[i], c[i], got[i], best)
        double_rounded += f32(np.float64(a[i]) * np.float64(b[i]) + np.float64(c[i])).tobytes() != f32(best).tobytes()
    print("cases a float64 sum rounded twice gets wrong:", double_rounded)


def reference_jw(x2, y2, z2, L, zf, af):
    """the reference's Jw (oracle/uwt_oracle.c:509-520) in numpy float32, C's left-to-right order"""
    fx, fy, zf, af, one = f32(L.fx), f32(L.fy), f32(zf), f32(af), f32(1)
    iz = one / z2
    iz = np.where(iz < 0, f32(0), iz).astype(f32)
    return ((fx * iz, -(((fx * x2) * iz) * iz) * zf, -((((fx * x2) * y2) * iz) * iz) * af, (fx * (one + ((x2 * x2) * iz) * iz)) * af,
             (((-fx) * y2) * iz) * af),
            (fy * iz, -(((fy * y2) * iz) * iz) * zf, -(fy * (one + ((y2 * y2) * iz) * iz)) * af, ((((fy * x2) * y2) * iz) * iz) * af,
             ((fy * x2) * iz) * af))


def test_row_product_is_the_oracles(O, synth, arith):
    """jacobian_rows over the REFERENCE Jw gives the oracle's J bit for bit in the test's arithmetic set (dense points of a rendered
    pair at a pose that is not the identity, fx != fy, factors (0.5, 1.25)): the row product the metric mode keeps is restated right"""
    w, h, intr = 96, 64, (80.0, 77.5, 47.5, 31.5)
    ref, tgt, dep = synth.render_pair(w, h, *intr, seed=9100, with_depth=True, max_t=0.015, max_deg=0.8)[:3]
    p = O.default_params(w, h, *intr, n_levels=2, has_depth=1)
    L = O.level_intrinsics(p, 0)
    gx, gy = O.scharr3(ref)
    pts = O.dense_points(dep, L.w, L.h, 0, p.depth_scale)
    pose = O.se3_exp(np.array([0.01, -0.006, 0.004, 0.003, -0.002, 0.004], f32))
    warped = O.warp(pts, pose, L)
    J, r, idx = O.residual_jacobian_ex(ref, tgt, gx, gy, pts, warped, L, 0.5, 1.25, 0)
    assert len(idx) > 3000
    at = pts[idx, 1].astype(np.int64) * L.iw + pts[idx, 0].astype(np.int64)
    g0, g1 = gx.reshape(-1)[at].astype(f32), gy.reshape(-1)[at].astype(f32)
    wp = warped[idx]
    mine = MR.jacobian_rows(MR.current_arith(O), g0, g1, reference_jw(wp[:, 0], wp[:, 1], wp[:, 2], L, 0.5, 1.25))
    assert np.array_equal(mine.view(np.uint32), J.view(np.uint32))
    # and the wrapper replaces J alone
    Jm, rm, im = MR.MetricOracle(O).residual_jacobian_ex(ref, tgt, gx, gy, pts, warped, L, 0.5, 1.25, 0)
    assert np.array_equal(rm, r) and np.array_equal(im, idx) and Jm.shape == J.shape
    assert np.array_equal(Jm[:, :2].view(np.uint32), J[:, :2].view(np.uint32)) and not np.array_equal(Jm[:, 2:], J[:, 2:])


# ---- 2. with the mode off the wrapper is the oracle -------------------------------------------------------------------------------------
def test_reference_mode_is_unchanged(O, synth, arith):
    w, h, intr = 96, 64, (78.0, 78.0, 47.5, 31.5)
    ref, tgt, dep = synth.render_pair(w, h, *intr, seed=9100, with_depth=True, max_t=0.015, max_deg=0.8)[:3]
    off = MR.MetricOracle(O, metric=False)
    for depth, weights, early in ((True, 0, 1), (False, 2, 0), (True, 1, 0)):
        p = O.default_params(w, h, *intr, n_levels=3, first_level=2, last_level=0, has_depth=int(depth), weights=weights,
                             early_exit=early, max_iters=50 if early else 4)
        d = dep if depth else None
        st, pose, tr = SR.align(off, p, ref, tgt, d)
        st0, pose0, tr0 = O.align_pair(p, ref, tgt, d, want_trace=True)
        assert st == st0 == 0 and pose.tobytes() == pose0.tobytes() and len(tr) == len(tr0)
        assert all(a["n_valid"] == b["n_valid"] and f32(a["error"]).tobytes() == f32(b["error"]).tobytes() for a, b in zip(tr, tr0))
        assert SR.align(MR.MetricOracle(O), p, ref, tgt, d)[1].tobytes() != pose0.tobytes()   # and the mode shows when it is on


# ---- 3. what the mode is for --------------------------------------------------------------------------------------------------------------
EVIDENCE = dict(w=320, h=240, intr=(262.5, 262.5, 159.5, 119.5), seeds=range(8), max_deg=2.0, max_t=0.03)


def evidence_pairs(synth):
    e = EVIDENCE
    return [synth.render_pair(e["w"], e["h"], *e["intr"], seed=s, z=1.0, max_t=e["max_t"], max_deg=e["max_deg"], with_depth=True)
            for s in e["seeds"]]


@pytest.mark.one_arith
@pytest.mark.parametrize("depth", [True, False], ids=["depth", "none"])
def test_metric_mode_recovers_the_rotation(O, synth, depth):
    """320 x 240, fx = fy = 262.5, seeds 0..7, motions up to 2 degrees and 0.03, 4 levels x 10 iterations without early exit, default
    arithmetic: the median rotation error of metric + keep is below half that of the reference Jacobian under the reference hand-off on
    the same pairs (measured: 0.086 against 1.034 degrees with depth, 0.074 against 0.909 without — the reference Jacobian leaves the
    rotation where the identity leaves it, 1.071)"""
    e = EVIDENCE
    p = O.default_params(e["w"], e["h"], *e["intr"], n_levels=4, first_level=3, last_level=0, max_iters=10, early_exit=0,
                         has_depth=int(depth))
    M = MR.MetricOracle(O)
    rows = {"identity": [], "reference": [], "metric+keep": []}
    for ref, tgt, dep, R, t in evidence_pairs(synth):
        d = dep if depth else None
        rows["identity"].append(MR.pose_errors(SR.IDENTITY, R, t))
        st, pose, _ = SR.align(O, p, ref, tgt, d)
        assert st == 0
        rows["reference"].append(MR.pose_errors(pose, R, t))
        st, pose, _ = SR.align(M, p, ref, tgt, d, keep=True)
        assert st == 0
        rows["metric+keep"].append(MR.pose_errors(pose, R, t))
    med = {k: (float(np.median([r for r, _ in v])), float(np.median([t for _, t in v])), max(r for r, _ in v)) for k, v in rows.items()}
    for k, (r, t, rmax) in med.items():
        print("%-12s rot err median %.3f deg  max %.3f deg   t err median %.4f" % (k, r, rmax, t))
    assert med["metric+keep"][0] < 0.5 * med["reference"][0], med


# ---- 4. the surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.one_arith
def test_abi_and_mirrors_carry_the_mode():
    importlib.import_module("uw-slam_amd").build_native()
    capi = importlib.import_module("uw-slam_amd.capi")
    hdr = open(os.path.join(ROOT, "include", "uwt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uwt_[a-z0-9_]+)\s*\(", src))
    lib = capi.lib()
    for name in ("uwt_set_jacobian", "uwt_get_jacobian"):
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"enum\s+uwt_jacobian\s*\{\s*UWT_JACOBIAN_REFERENCE\s*=\s*0\s*,\s*UWT_JACOBIAN_METRIC\s*=\s*1\s*\}", src)
    assert re.search(r"#define UWT_ABI_VERSION 4\b", src) and lib.uwt_abi_version() == 4
    assert (capi.JACOBIAN_REFERENCE, capi.JACOBIAN_METRIC) == (0, 1)
    assert "handoff = 1" in hdr and "z_factor = 1" in hdr   # the header names the intended hand-off and the live call's exception
    assert lib.uwt_set_jacobian(None, 1) == 1 and lib.uwt_get_jacobian(None, ctypes.byref(ctypes.c_int32())) == 1   # null context
    assert all(hasattr(capi.Context, m) for m in ("set_jacobian", "get_jacobian"))
    T = importlib.import_module("uw-slam_amd.tracker")
    assert hasattr(T.Tracker, "SetJacobian")
    hpp = open(os.path.join(ROOT, "include", "uw_tracker.hpp")).read()
    assert "void SetJacobian(int mode)" in hpp and "uwt_set_jacobian" in hpp
    tool = open(os.path.join(ROOT, "tools", "track_sequence.py")).read()
    assert "--jacobian" in tool
    assert "--jacobian" in open(os.path.join(ROOT, "tools", "uwt_bench.cpp")).read()
