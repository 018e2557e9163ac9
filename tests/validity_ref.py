"""The warp and validity stage restated in numpy, in both arithmetic sets.  A helper of the tests, not a test.

Written from the reference as the oracle cites it: Tracker::WarpFunction (src/Tracker.cpp:1439-1467) and the per-point body of
ComputeResidualJacobian (:447-479).  Every float32 operation is one numpy float32 operation (rounded once, in the written order); the
places where the reference widens are written as float64:

    unprojection   legacy: (x - c) * inv.   OpenCV: the MatExpr "(col - c) * inv" is folded to convertTo(alpha = inv, beta = -c * inv)
                   with alpha, beta formed in double and narrowed: x * (float)alpha + (float)beta; alpha == +-1 becomes an add / a subtract
    X = X * z      (:1440, :1444)
    rigid product  legacy: T0 * X, then three fused multiply-adds.  OpenCV: cv::gemm on CV_32F sums exact double products in the fold
                   s0 + ((s1 + s2) + s3) and narrows once
    u = o0 * fx;  u = u / o2;  u = u + cx;  u = u * o3      (:1454-1456, :1466; the division is the IEEE one, subnormals included)
    valid          y2 > 0 && y2 < rows && x2 > 0 && x2 < cols (:450, the IMAGE's size) && z2 != 0 (:451) && (x1, y1) truncated lies in the image
    iz             1 / z2, and 0 where that is negative (:447, :452-453)
    sample         (int)round(x2) (half away from zero), clamped to cols - 1 / rows - 1 (:472 and the clamp every implementation here has)
    (x1, y1)       truncated toward zero (Mat::at(float, float))
    Jw, Jl * Jw    :455-467, :479, written here; the metric mode's Jw alone comes from tests/metric_ref.py (its contract lives there)

`mut` names ONE deliberate mistake (MUTANTS); tests/test_validity_cpu.py shows that each is noticed by a named case of
tests/validity_cases.py.  None of this is a translation of oracle/uwt_oracle.c or of the kernels: it shares no code with either and
is held to the oracle bit for bit by the same test file."""
import numpy as np

import metric_ref as MR
import seeded_ref as SR

f32, f64 = np.float32, np.float64
OPENCV, LEGACY = 0, 1

MUTANTS = ("gt0_to_ge0", "lt_iw_to_le_iw", "iw_is_gw", "iw_is_ih", "round_half_even", "floor_of_f32_sum", "no_upper_clamp", "clamp_to_gw",
           "z2_ne0_removed", "iz_lt0_to_le0", "iz_abs", "sentinel_w_ignored", "x1y1_rounded", "u_times_w_dropped")


def rigid_matrix(pose):
    """SE3::matrix() of pose = qx qy qz qw tx ty tz: 3 x 4 float32"""
    R = SR.quat_to_rot(np.asarray(pose, f32)[:4]).reshape(3, 3)
    return np.concatenate([R, np.asarray(pose, f32)[4:].reshape(3, 1)], axis=1).astype(f32)


def unproject(x, c, inv, arith):
    x, c, inv = np.asarray(x, f32), f32(c), f32(inv)
    if arith == LEGACY:
        return (x - c) * inv
    alpha = f64(inv)
    beta = f32(-f64(c) * f64(inv))
    if alpha == 1.0:
        return x + beta
    if alpha == -1.0:
        return beta - x
    m = x * f32(alpha)
    return m + beta


def warp(pts, pose, L, arith, mut=None):
    """Tracker::WarpFunction on an n x 4 table: n x 4 float32 (u, v, z2, w2)"""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    T = rigid_matrix(pose)
    x, y, z, w = (np.ascontiguousarray(pts[:, k]) for k in range(4))
    if mut == "sentinel_w_ignored":
        w = np.ones_like(w)
    with np.errstate(all="ignore"):
        X = unproject(x, L.cx, L.invfx, arith) * z
        Y = unproject(y, L.cy, L.invfy, arith) * z
        o = []
        for k in range(3):
            if arith == LEGACY:
                s = T[k, 0] * X
                s = MR.fma32(np.full_like(X, T[k, 1]), Y, s)
                s = MR.fma32(np.full_like(X, T[k, 2]), z, s)
                s = MR.fma32(np.full_like(X, T[k, 3]), w, s)
            else:
                s0, s1 = f64(T[k, 0]) * X.astype(f64), f64(T[k, 1]) * Y.astype(f64)
                s2, s3 = f64(T[k, 2]) * z.astype(f64), f64(T[k, 3]) * w.astype(f64)
                s = (s0 + ((s1 + s2) + s3)).astype(f32)
            o.append(s.astype(f32))
        u = o[0] * f32(L.fx)
        u = u / o[2]
        u = u + f32(L.cx)
        v = o[1] * f32(L.fy)
        v = v / o[2]
        v = v + f32(L.cy)
        if mut != "u_times_w_dropped":
            u = u * w                                          # (the fourth row of the matrix is 0 0 0 1: w2 = w exactly)
            v = v * w
    out = np.stack([u, v, o[2], w], axis=1)
    assert out.dtype == f32
    return out


def c_round(x, mut=None):
    """(int)roundf(x) for finite x >= 0 as int64"""
    x = np.asarray(x, f32)
    if mut == "round_half_even":
        return np.rint(x.astype(f64)).astype(np.int64)
    if mut == "floor_of_f32_sum":
        return np.floor(x + f32(0.5)).astype(np.int64)         # the sum rounded to float32 first
    return np.floor(x.astype(f64) + 0.5).astype(np.int64)      # exact in double


def bilinear(img, x, y):
    """the bilinear sample (an extension of this project; the oracle's uwo_bilinear_u8): floorf, the low index clamped to the last
    column / row, the high one to the same, three fused multiply-adds"""
    h, w = img.shape
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    ix0 = np.minimum(x0.astype(np.int64), w - 1)
    iy0 = np.minimum(y0.astype(np.int64), h - 1)
    ix1, iy1 = np.minimum(ix0 + 1, w - 1), np.minimum(iy0 + 1, h - 1)
    a, b = img[iy0, ix0].astype(f32), img[iy0, ix1].astype(f32)
    c, d = img[iy1, ix0].astype(f32), img[iy1, ix1].astype(f32)
    top = MR.fma32(ax, b - a, a)
    bot = MR.fma32(ax, d - c, c)
    return MR.fma32(ay, bot - top, top)


def jw_reference(x2, y2, iz, L, zf, af):
    """Jw of :455-467, every product in the source's left-to-right order: ((a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5))"""
    fx, fy, zf, af, one = f32(L.fx), f32(L.fy), f32(zf), f32(af), f32(1)
    with np.errstate(all="ignore"):
        a0 = fx * iz
        a2 = -(fx * x2 * iz * iz) * zf
        a3 = -(fx * x2 * y2 * iz * iz) * af
        a4 = (fx * (one + x2 * x2 * iz * iz)) * af
        a5 = -fx * y2 * iz * af
        b1 = fy * iz
        b2 = -(fy * y2 * iz * iz) * zf
        b3 = -(fy * (one + y2 * y2 * iz * iz)) * af
        b4 = fy * x2 * y2 * iz * iz * af
        b5 = fy * x2 * iz * af
    return (a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5)


def jl_times_jw(arith, g0, g1, jw):
    """Jacobian_row = Jl * Jw (:479) for Jl = (g0, g1), written here from the reference and not taken from tests/metric_ref.py: [n, 6].
    OpenCV set: cv::gemm on CV_32F with a double accumulator that starts at 0, s += g0 * Jw0k, s += g1 * Jw1k, narrowed once; legacy set:
    the float product g0 * Jw0k and one fused multiply-add of g1 * Jw1k.  Columns 0 and 1 meet Jw's structural zeros (Jw01 = Jw10 = 0)."""
    (a0, a2, a3, a4, a5), (b1, b2, b3, b4, b5) = jw
    zero = np.zeros_like(g0)
    rows0, rows1 = (a0, zero, a2, a3, a4, a5), (zero, b1, b2, b3, b4, b5)
    J = np.empty((len(g0), 6), f32)
    with np.errstate(all="ignore"):
        for k in range(6):
            if arith == LEGACY:
                J[:, k] = MR.fma32(g1, rows1[k], g0 * rows0[k])          # (fma32: an exact float32 fused multiply-add, a numeric primitive)
            else:
                s = np.zeros(len(g0), f64) + g0.astype(f64) * rows0[k].astype(f64)
                J[:, k] = (s + g1.astype(f64) * rows1[k].astype(f64)).astype(f32)
    return J


def evaluate(img1, img2, gx1, gy1, pts, warped, L, arith, zf=1.0, af=1.0, sampler=0, metric=False, mut=None):
    """The per-point body of ComputeResidualJacobian over a table and its warp.  Returns a dict over ALL n rows: valid (bool), iz, ix2,
    iy2 (the sample, int64), ix1, iy1, r and J ([n, 6]); r, J and the indices are meaningful where valid is set."""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    wp = np.asarray(warped, f32).reshape(-1, 4)
    iw, ih, gw = int(L.iw), int(L.ih), int(L.w)
    cols, rows = iw, ih
    if mut == "iw_is_gw":
        cols = gw
    if mut == "iw_is_ih":
        cols, rows = ih, iw
    x1, y1 = pts[:, 0], pts[:, 1]
    x2, y2, z2 = (np.ascontiguousarray(wp[:, k]) for k in range(3))
    with np.errstate(all="ignore"):
        iz = f32(1) / z2
        lo_x, lo_y = (x2 >= 0, y2 >= 0) if mut == "gt0_to_ge0" else (x2 > 0, y2 > 0)
        hi_x, hi_y = (x2 <= f32(cols), y2 <= f32(rows)) if mut == "lt_iw_to_le_iw" else (x2 < f32(cols), y2 < f32(rows))
        valid = lo_y & hi_y & lo_x & hi_x
        if mut != "z2_ne0_removed":
            valid = valid & (z2 != 0)
        src = np.isfinite(x1) & np.isfinite(y1)
        tr = (lambda a: np.floor(np.where(src, a, 0).astype(f64) + 0.5)) if mut == "x1y1_rounded" else (lambda a: np.trunc(np.where(src, a, 0)))
        ix1, iy1 = tr(x1).astype(np.int64), tr(y1).astype(np.int64)
        valid = valid & src & (ix1 >= 0) & (ix1 < iw) & (iy1 >= 0) & (iy1 < ih)   # a row whose reference position is outside is dropped
        if mut == "iz_abs":
            iz = np.abs(iz)
        elif mut == "iz_lt0_to_le0":
            iz = np.where(iz <= 0, f32(0), iz).astype(f32)
        else:
            iz = np.where(iz < 0, f32(0), iz).astype(f32)
    xs, ys = np.where(valid, x2, f32(1)), np.where(valid, y2, f32(1))
    ix2, iy2 = c_round(xs, mut), c_round(ys, mut)
    if mut == "clamp_to_gw":
        ix2, iy2 = np.minimum(ix2, gw - 1), np.minimum(iy2, int(L.h) - 1)
    elif mut != "no_upper_clamp":
        ix2, iy2 = np.minimum(ix2, iw - 1), np.minimum(iy2, ih - 1)
    ix1, iy1 = np.where(valid, ix1, 0), np.where(valid, iy1, 0)
    at1 = iy1 * iw + ix1
    at2 = (iy2 * iw + ix2) % (iw * ih)                        # (a mutant's index past the plane wraps: it is compared, not trusted)
    i1 = np.asarray(img1, np.uint8).reshape(-1)[at1].astype(np.int64)
    i2 = np.asarray(img2, np.uint8).reshape(-1)[at2].astype(np.int64)
    r = (i2 - i1).astype(f32)
    if sampler == 1:
        r = bilinear(np.asarray(img2, np.uint8).reshape(ih, iw), xs, ys) - i1.astype(f32)
    g0 = np.asarray(gx1, np.int16).reshape(-1)[at1].astype(f32)
    g1 = np.asarray(gy1, np.int16).reshape(-1)[at1].astype(f32)
    if metric:
        jw = MR.jw_terms(x2, y2, z2, L, zf, af)              # (forms its own iz <- max(1 / z2, 0))
    else:
        jw = jw_reference(x2, y2, iz, L, zf, af)
    J = jl_times_jw(arith, g0, g1, jw)
    return dict(valid=valid, iz=iz, ix2=ix2, iy2=iy2, ix1=ix1, iy1=iy1, r=r, J=J)


def compressed(ev):
    """(J, r, idx) over the valid rows, as the oracle's residual_jacobian_ex returns them"""
    idx = np.nonzero(ev["valid"])[0].astype(np.int32)
    return ev["J"][idx], ev["r"][idx], idx


def same_bits(a, b, nan_equal=False):
    """a and b hold the same bits; nan_equal: a NaN matches a NaN of any payload"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    if nan_equal:
        both = np.isnan(a) & np.isnan(b)
        ua, ub = np.where(both, 0, ua), np.where(both, 0, ub)
    return bool(np.array_equal(ua, ub))


class Oracle:
    """This restatement behind the oracle module's names (warp, residual_jacobian_ex), so that tests/seeded_ref.py's loop can run on it;
    everything else is the oracle's"""

    def __init__(self, O, metric=False):
        self._O, self.metric = O, metric

    def __getattr__(self, name):
        return getattr(self._O, name)

    def warp(self, pts, pose, L):
        return warp(pts, pose, L, MR.current_arith(self._O))

    def residual_jacobian_ex(self, img1, img2, gx1, gy1, pts, warped, L, z_factor=1.0, angle_factor=1.0, sampler=0):
        return compressed(evaluate(img1, img2, gx1, gy1, pts, warped, L, MR.current_arith(self._O), z_factor, angle_factor, sampler, self.metric))
