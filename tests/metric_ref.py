"""The metric Jacobian (include/uwt.h "the metric Jacobian") restated on the CPU.  A helper of the tests, not a test.

The contract.  Inputs: the values the reference-mode Jw reads — x2, y2, iz behind the validity test and iz <- max(1 / z2, 0); the level's
fx, fy, cx, cy, invfx, invfy; the factors zf, af.  Everything f32, every operation rounded once, in the written order, the same in both
arithmetic sets:

    xn = (x2 - cx) * invfx                                 yn = (y2 - cy) * invfy
    row 0:  a0 = fx * iz      0      a2 = -(((fx * xn) * iz) * zf)   a3 = -(((fx * xn) * yn) * af)
            a4 = (fx * (1 + xn * xn)) * af                            a5 = -((fx * yn) * af)
    row 1:  0      b1 = fy * iz      b2 = -(((fy * yn) * iz) * zf)   b3 = -((fy * (1 + yn * yn)) * af)
            b4 = ((fy * xn) * yn) * af                                b5 = (fy * xn) * af

(the reference's Jw, src/Tracker.cpp:455-467, with X = xn * z2, Y = yn * z2 in place of x2, y2).  Jacobian_row = Jl * Jw keeps the
arithmetic set's own form (oracle/uwt_oracle.c, residual_jacobian_ar):
    OpenCV set   J[k] = (float)((0 + (double)g0 * Jw0k) + (double)g1 * Jw1k)   — a cv::gemm with double accumulation;
    legacy set   J[k] = fmaf(g1, Jw1k, g0 * Jw0k)                              — an f32 product and one fused multiply-add.

MetricOracle wraps the oracle module: validity, r and the point order come from its residual_jacobian_ex, J is replaced.
seeded_ref.align(MetricOracle(O), ...) then gives metric alignments with any seed, hand-off, weights, sampler or tables.
"""
import numpy as np

f32, f64 = np.float32, np.float64


def jw_terms(x2, y2, z2, L, zf, af):
    """The ten non-zero entries of Jw for warped points (x2, y2, z2) of level L, as float32 arrays:
    (a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5).  numpy rounds every float32 operation once; the order is the contract's."""
    x2, y2, z2 = (np.asarray(v, f32) for v in (x2, y2, z2))
    fx, fy, cx, cy, invfx, invfy = (f32(v) for v in (L.fx, L.fy, L.cx, L.cy, L.invfx, L.invfy))
    zf, af, one = f32(zf), f32(af), f32(1)
    with np.errstate(all="ignore"):
        iz = one / z2
        iz = np.where(iz < 0, f32(0), iz).astype(f32)       # "if (inv_z2 < 0) inv_z2 = 0" (:452-453)
        xn = (x2 - cx) * invfx
        yn = (y2 - cy) * invfy
        a0 = fx * iz
        a2 = -(((fx * xn) * iz) * zf)
        a3 = -(((fx * xn) * yn) * af)
        a4 = (fx * (one + xn * xn)) * af
        a5 = -((fx * yn) * af)
        b1 = fy * iz
        b2 = -(((fy * yn) * iz) * zf)
        b3 = -((fy * (one + yn * yn)) * af)
        b4 = ((fy * xn) * yn) * af
        b5 = (fy * xn) * af
    out = (a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5)
    assert all(v.dtype == f32 for row in out for v in row)
    return out


def jw_closed_f64(x2, y2, z2, L, zf, af):
    """The same entries in closed form, evaluated in float64 from the same float32 inputs (iz = 1 / z2, z2 > 0)."""
    x2, y2, z2 = (np.asarray(v, f32).astype(f64) for v in (x2, y2, z2))
    fx, fy, cx, cy, invfx, invfy, zf, af = (f64(f32(v)) for v in (L.fx, L.fy, L.cx, L.cy, L.invfx, L.invfy, zf, af))
    iz = 1.0 / z2
    xn, yn = (x2 - cx) * invfx, (y2 - cy) * invfy
    return ((fx * iz, -fx * xn * iz * zf, -fx * xn * yn * af, fx * (1 + xn * xn) * af, -fx * yn * af),
            (fy * iz, -fy * yn * iz * zf, -fy * (1 + yn * yn) * af, fy * xn * yn * af, fy * xn * af))


def jw_reference_substituted_f64(x2, y2, z2, L, zf, af):
    """The reference's expressions (oracle/uwt_oracle.c:509-520) in float64 with X = xn * z2, Y = yn * z2 where it has x2, y2."""
    x2, y2, z2 = (np.asarray(v, f32).astype(f64) for v in (x2, y2, z2))
    fx, fy, cx, cy, invfx, invfy, zf, af = (f64(f32(v)) for v in (L.fx, L.fy, L.cx, L.cy, L.invfx, L.invfy, zf, af))
    iz = 1.0 / z2
    X, Y = (x2 - cx) * invfx * z2, (y2 - cy) * invfy * z2
    return ((fx * iz, -(fx * X * iz * iz) * zf, -(fx * X * Y * iz * iz) * af, (fx * (1 + X * X * iz * iz)) * af, -fx * Y * iz * af),
            (fy * iz, -(fy * Y * iz * iz) * zf, -(fy * (1 + Y * Y * iz * iz)) * af, fy * X * Y * iz * iz * af, fy * X * iz * af))


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: a * b is exact in float64 (48 bits), the sum with c is formed in float64 with its
    rounding error recovered (two-sum) and, where it is inexact, forced to an odd last bit — a float64 rounded to odd rounds to the
    float32 the exact sum rounds to (29 spare bits), which a plain float64 sum rounded twice does not."""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        t = p + c
        bb = t - p
        e = (p - (t - bb)) + (c - bb)
    bits = np.ascontiguousarray(t).view(np.int64).copy()
    fix = np.isfinite(t) & (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (t > 0)                                # the exact sum lies further from zero than t
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(f64).astype(f32)


def jacobian_rows(arith, g0, g1, jw):
    """Jacobian_row = Jl * Jw for Jl = (g0, g1) (float32 arrays: the gradients) in arithmetic set `arith` (0 OpenCV, 1 legacy): [n, 6]"""
    (a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5) = jw
    g0, g1 = np.asarray(g0, f32), np.asarray(g1, f32)
    zero = np.zeros_like(g0)
    A, B = (a0, zero, a2, a3, a4, a5), (zero, b1, b2, b3, b4, b5)
    J = np.empty((len(g0), 6), f32)
    with np.errstate(all="ignore"):
        for k in range(6):
            if arith == 1:
                J[:, k] = fma32(g1, B[k], g0 * A[k])
            else:
                s = np.zeros(len(g0), f64)
                s = s + g0.astype(f64) * A[k].astype(f64)      # exact products
                s = s + g1.astype(f64) * B[k].astype(f64)
                J[:, k] = s.astype(f32)
    return J


def current_arith(O):
    """the arithmetic set the oracle's per-stage functions are in"""
    ar = O.set_arith(0)
    O.set_arith(ar)
    return ar


class MetricOracle:
    """The oracle module with residual_jacobian_ex's J in metric mode (metric False: the module unchanged)."""

    def __init__(self, O, metric=True):
        self._O, self.metric = O, metric

    def __getattr__(self, name):
        return getattr(self._O, name)

    def residual_jacobian_ex(self, img1, img2, gx1, gy1, pts, warped, L, z_factor=1.0, angle_factor=1.0, sampler=0):
        J, r, idx = self._O.residual_jacobian_ex(img1, img2, gx1, gy1, pts, warped, L, z_factor, angle_factor, sampler)
        if not self.metric or len(idx) == 0:
            return J, r, idx
        pts = np.ascontiguousarray(pts, f32).reshape(-1, 4)[idx]
        wp = np.ascontiguousarray(warped, f32).reshape(-1, 4)[idx]
        at = pts[:, 1].astype(np.int64) * L.iw + pts[:, 0].astype(np.int64)   # Mat::at(y1, x1) truncates (:476-477)
        g0 = np.ascontiguousarray(gx1, np.int16).reshape(-1)[at].astype(f32)
        g1 = np.ascontiguousarray(gy1, np.int16).reshape(-1)[at].astype(f32)
        jw = jw_terms(wp[:, 0], wp[:, 1], wp[:, 2], L, z_factor, angle_factor)
        return jacobian_rows(current_arith(self._O), g0, g1, jw), r, idx


def pose_errors(pose, R, t):
    """(rotation error in degrees, translation error) of pose = qx qy qz qw tx ty tz against the motion X' = R X + t"""
    from importlib import import_module
    q = import_module("uw-slam_amd.synth")._quat_from_R(R)
    p = np.asarray(pose, f64)
    d = min(1.0, abs(float(np.dot(p[:4] / np.linalg.norm(p[:4]), q))))
    return float(np.degrees(2.0 * np.arccos(d))), float(np.linalg.norm(p[4:] - np.asarray(t, f64)))
