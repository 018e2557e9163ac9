"""The restatement, in numpy, of the SURF contract of include/uwt.h (uwt_surf_*) and nothing else: integral image, fast-Hessian
responses, suppression, refinement, order and capacity, orientation, descriptor.  A helper module of the SURF tests and of nothing
else (not a test, not a conftest).  Every f32 / f64 step is one numpy ufunc on arrays of that type, so each rounds as the device's
does (no FMA anywhere); integers are int64.
"""
import numpy as np

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("dir_x", "<f4"), ("dir_y", "<f4"),
                     ("octave", "<i4"), ("laplacian", "<i4")])
F = np.float32

# the literal tables of include/uwt.h (tests/test_surf_cpu.py compares them with the header's text)
SCALE = F(0.13333334)   # 1.2 / 9
ORI_WEIGHT = np.array([
    1.0, 0.923116326, 0.726149023, 0.486752242, 0.27803731, 0.135335281, 0.0561347641,
    0.923116326, 0.852143764, 0.670320034, 0.449328959, 0.256660789, 0.12493021, 0.0518189184,
    0.726149023, 0.670320034, 0.52729243, 0.353454679, 0.201896518, 0.0982735828, 0.0407622047,
    0.486752242, 0.449328959, 0.353454679, 0.236927763, 0.135335281, 0.0658747554, 0.0273237228,
    0.27803731, 0.256660789, 0.201896518, 0.135335281, 0.0773047432, 0.0376282558, 0.0156075582,
    0.135335281, 0.12493021, 0.0982735828, 0.0658747554, 0.0376282558, 0.0183156393, 0.00759701384,
    0.0561347641, 0.0518189184, 0.0407622047, 0.0273237228, 0.0156075582, 0.00759701384, 0.00315111154], F).reshape(7, 7)
ORI_DIR = np.array([
    1.0, 0.0, 0.98480773, 0.173648179, 0.939692616, 0.342020154, 0.866025388, 0.5,
    0.766044438, 0.642787635, 0.642787635, 0.766044438, 0.5, 0.866025388, 0.342020154, 0.939692616,
    0.173648179, 0.98480773, 0.0, 1.0, -0.173648179, 0.98480773, -0.342020154, 0.939692616,
    -0.5, 0.866025388, -0.642787635, 0.766044438, -0.766044438, 0.642787635, -0.866025388, 0.5,
    -0.939692616, 0.342020154, -0.98480773, 0.173648179, -1.0, 0.0, -0.98480773, -0.173648179,
    -0.939692616, -0.342020154, -0.866025388, -0.5, -0.766044438, -0.642787635, -0.642787635, -0.766044438,
    -0.5, -0.866025388, -0.342020154, -0.939692616, -0.173648179, -0.98480773, 0.0, -1.0,
    0.173648179, -0.98480773, 0.342020154, -0.939692616, 0.5, -0.866025388, 0.642787635, -0.766044438,
    0.766044438, -0.642787635, 0.866025388, -0.5, 0.939692616, -0.342020154, 0.98480773, -0.173648179], F).reshape(36, 2)
DESC_GAUSS = np.array([
    0.988587201, 0.901851177, 0.750541389, 0.569815516, 0.394651532,
    0.249352202, 0.143725067, 0.0755738765, 0.0362518989, 0.0158638898], F)

# the grid points of the radius-6 disc, j (y) outermost, both ascending: 109 samples
ORI_J, ORI_I = np.nonzero(np.add.outer(np.arange(-6, 7) ** 2, np.arange(-6, 7) ** 2) < 36)
ORI_J, ORI_I = ORI_J - 6, ORI_I - 6


def default_params():
    return dict(hessian_threshold=100.0, n_octaves=4, n_octave_layers=2, upright=0)


def integral(img):
    """(h+1) x (w+1) uint32, modulo 2^32: I[y, x] = the sum of img[:y, :x]"""
    h, w = img.shape
    out = np.zeros((h + 1, w + 1), np.uint64)
    out[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.uint64), axis=0), axis=1)
    return (out & 0xFFFFFFFF).astype(np.uint32)


def _box(I, x0, y0, x1, y1):
    """the sum over [x0, x1) x [y0, y1), modulo 2^32, as int64; the corners are inside the integral image"""
    s = I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]   # uint32 arithmetic wraps
    return s.astype(np.int64)


def _box_clip(I, x0, y0, x1, y1):
    h, w = I.shape[0] - 1, I.shape[1] - 1
    return _box(I, np.clip(x0, 0, w), np.clip(y0, 0, h), np.clip(x1, 0, w), np.clip(y1, 0, h))


def filter_size(octave, layer):
    return (9 + 6 * layer) << octave


def octaves_of(w, h, p):
    """the octaves that run: the largest filter fits in the frame"""
    top = p["n_octave_layers"] + 1
    return [o for o in range(p["n_octaves"]) if filter_size(o, top) <= min(w, h)]


def hessian_parts(I, octave, layer):
    """Dxx, Dyy, Dxy (int64) and the mask of existing responses on the octave's gw x gh grid"""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    s, step = filter_size(octave, layer), 1 << octave
    gw, gh = w >> octave, h >> octave
    gy, gx = np.mgrid[0:gh, 0:gw]
    x0, y0 = gx * step - (s >> 1), gy * step - (s >> 1)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + s <= w) & (y0 + s <= h)
    x0, y0 = np.where(ok, x0, 0), np.where(ok, y0, 0)
    if s > min(w, h):
        z = np.zeros((gh, gw), np.int64)
        return z, z, z, np.zeros((gh, gw), bool)
    p = [(c * s + 4) // 9 for c in range(10)]
    bx = lambda a, b, c, d: _box(I, x0 + a, y0 + b, x0 + c, y0 + d)
    dxx = bx(p[0], p[2], p[9], p[7]) - 3 * bx(p[3], p[2], p[6], p[7])
    dyy = bx(p[2], p[0], p[7], p[9]) - 3 * bx(p[2], p[3], p[7], p[6])
    dxy = bx(p[1], p[1], p[4], p[4]) + bx(p[5], p[5], p[8], p[8]) - bx(p[5], p[1], p[8], p[4]) - bx(p[1], p[5], p[4], p[8])
    return dxx, dyy, dxy, ok


def response_layer(I, octave, layer):
    """gh x gw f64, NaN where no response exists; and the sign of Dxx + Dyy"""
    dxx, dyy, dxy, ok = hessian_parts(I, octave, layer)
    s = filter_size(octave, layer)
    num = 100 * dxx * dyy - 81 * dxy * dxy
    den = 100.0 * float(s * s) * float(s * s)
    r = num.astype(np.float64) / den
    r[~ok] = np.nan
    return r, np.sign(dxx + dyy).astype(np.int32)


def detect(img, p=None, cap=4096):
    """key points without their direction (dir = (1, 0)), in contract order, at most cap"""
    p = p or default_params()
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    I = integral(img)
    L = p["n_octave_layers"] + 2
    thr = float(p["hessian_threshold"])
    out = []
    for o in octaves_of(w, h, p):
        lay = [response_layer(I, o, i) for i in range(L)]
        R = np.stack([r for r, _ in lay])
        step = 1 << o
        for i in range(1, L - 1):
            c = R[i, 1:-1, 1:-1]
            with np.errstate(invalid="ignore"):
                keep = c > thr
                for dl in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if dl or dy or dx:
                                nb = R[i + dl, 1 + dy:R.shape[1] - 1 + dy, 1 + dx:R.shape[2] - 1 + dx]
                                keep &= c > nb   # a NaN neighbour (absent) fails
            gy, gx = np.nonzero(keep)
            gy, gx = gy + 1, gx + 1
            if gy.size == 0:
                continue
            v = R[i, gy, gx]
            g = lambda dl, dy, dx: R[i + dl, gy + dy, gx + dx]
            dx_ = (g(0, 0, 1) - g(0, 0, -1)) * 0.5
            dy_ = (g(0, 1, 0) - g(0, -1, 0)) * 0.5
            ds_ = (g(1, 0, 0) - g(-1, 0, 0)) * 0.5
            dxx = (g(0, 0, 1) - 2.0 * v) + g(0, 0, -1)
            dyy = (g(0, 1, 0) - 2.0 * v) + g(0, -1, 0)
            dss = (g(1, 0, 0) - 2.0 * v) + g(-1, 0, 0)
            dxy = (((g(0, 1, 1) - g(0, 1, -1)) - g(0, -1, 1)) + g(0, -1, -1)) * 0.25
            dxs = (((g(1, 0, 1) - g(1, 0, -1)) - g(-1, 0, 1)) + g(-1, 0, -1)) * 0.25
            dys = (((g(1, 1, 0) - g(1, -1, 0)) - g(-1, 1, 0)) + g(-1, -1, 0)) * 0.25
            b0, b1, b2 = -dx_, -dy_, -ds_
            with np.errstate(all="ignore"):
                p0 = dxx
                m1, m2 = dxy / p0, dxs / p0
                a11, a12, c1 = dyy - m1 * dxy, dys - m1 * dxs, b1 - m1 * b0
                a21, a22, c2 = dys - m2 * dxy, dss - m2 * dxs, b2 - m2 * b0
                p1 = a11
                m3 = a21 / p1
                p2 = a22 - m3 * a12
                c2 = c2 - m3 * c1
                os_ = c2 / p2
                oy = (c1 - a12 * os_) / p1
                ox = ((b0 - dxy * oy) - dxs * os_) / p0
                good = (p0 != 0) & (p1 != 0) & (p2 != 0) & (np.abs(ox) <= 1) & (np.abs(oy) <= 1) & (np.abs(os_) <= 1)
            for k in np.nonzero(good)[0]:
                rec = np.zeros((), KEYPOINT)
                rec["x"] = F((float(gx[k]) + ox[k]) * float(step))
                rec["y"] = F((float(gy[k]) + oy[k]) * float(step))
                rec["size"] = F(float(filter_size(o, i)) + os_[k] * float(6 << o))
                rec["response"] = F(v[k])
                rec["dir_x"], rec["dir_y"] = 1.0, 0.0
                rec["octave"], rec["laplacian"] = o, lay[i][1][gy[k], gx[k]]
                out.append(((o, i, int(gy[k]), int(gx[k])), rec))
    out.sort(key=lambda e: e[0])   # the nested loops already give this order; stated, not relied upon
    kps = np.array([r for _, r in out], KEYPOINT) if out else np.zeros(0, KEYPOINT)
    if len(kps) > cap:
        idx = np.arange(len(kps))
        order = np.lexsort((idx, -kps["response"].astype(np.float64)))   # response descending, then order ascending
        kps = kps[np.sort(order[:cap])]
    return kps


def _rnd(v):
    """(int)floorf(v + 0.5f)"""
    return np.floor(v.astype(F) + F(0.5)).astype(np.int64)


def _haar(I, px, py, hh):
    """(right - left, bottom - top) of the 2hh x 2hh box centred on the pixel corner (px, py), clipped to the image; int64"""
    dx = _box_clip(I, px, py - hh, px + hh, py + hh) - _box_clip(I, px - hh, py - hh, px, py + hh)
    dy = _box_clip(I, px - hh, py, px + hh, py + hh) - _box_clip(I, px - hh, py - hh, px + hh, py)
    return dx, dy


def orientation(I, x, y, size):
    """(dir_x, dir_y) of key points (arrays of n)"""
    x, y, sc = np.asarray(x, F), np.asarray(y, F), np.asarray(size, F) * SCALE
    hh = np.maximum(1, _rnd(F(2.0) * sc))[:, None]
    px = _rnd(x[:, None] + ORI_I.astype(F)[None, :] * sc[:, None])
    py = _rnd(y[:, None] + ORI_J.astype(F)[None, :] * sc[:, None])
    dx, dy = _haar(I, px, py, hh)
    wgt = ORI_WEIGHT[np.abs(ORI_J), np.abs(ORI_I)][None, :]
    wx, wy = wgt * dx.astype(F), wgt * dy.astype(F)             # [n, 109]
    a, b = ORI_DIR, ORI_DIR[(np.arange(36) + 6) % 36]           # [36, 2]
    c0 = a[None, :, 0, None] * wy[:, None, :] - a[None, :, 1, None] * wx[:, None, :]   # cross(U[k], v)      [n, 36, 109]
    c1 = wx[:, None, :] * b[None, :, 1, None] - wy[:, None, :] * b[None, :, 0, None]   # cross(v, U[k + 6])
    m = (c0 >= 0) & (c1 > 0)
    sx, sy = np.zeros(m.shape[:2], F), np.zeros(m.shape[:2], F)
    for t in range(m.shape[2]):                                  # in sample order; a sample outside the window adds nothing
        sx = np.where(m[:, :, t], sx + wx[:, None, t], sx)
        sy = np.where(m[:, :, t], sy + wy[:, None, t], sy)
    n2 = sx * sx + sy * sy
    k = np.argmax(n2, axis=1)                                    # the first maximum: the lowest window wins a tie
    r = np.arange(len(k))
    bx, by = sx[r, k], sy[r, k]
    n = np.sqrt(bx * bx + by * by)
    with np.errstate(all="ignore"):
        return np.where(n == 0, F(1), bx / n).astype(F), np.where(n == 0, F(0), by / n).astype(F)


_T = np.arange(20)
_LOC = _T.astype(F) - F(9.5)
_GK = np.where(_T < 10, 9 - _T, _T - 10)


def descriptor(I, x, y, size, dir_x, dir_y):
    """[n, 64] floats of key points (arrays of n)"""
    e = lambda v: np.asarray(v, F)[:, None, None]
    x, y, sc, c, s = e(x), e(y), e(size) * SCALE, e(dir_x), e(dir_y)
    hh = np.maximum(1, _rnd(sc))
    ty_, tx_ = np.meshgrid(_T, _T, indexing="ij")   # [row t_y, column t_x]
    rx, ry = _LOC[tx_][None] * sc, _LOC[ty_][None] * sc
    sx = x + (rx * c - ry * s)
    sy = y + (rx * s + ry * c)
    dx, dy = _haar(I, _rnd(sx), _rnd(sy), hh)
    g = (DESC_GAUSS[_GK[tx_]] * DESC_GAUSS[_GK[ty_]])[None]
    wdx, wdy = g * dx.astype(F), g * dy.astype(F)
    tx = wdx * c + wdy * s
    ty = wdy * c - wdx * s
    n = tx.shape[0]
    # [n, b, v, a, u] -> [n, b, a, v, u]: sub-region (b, a), v outermost, u innermost
    tx = tx.reshape(n, 4, 5, 4, 5).transpose(0, 1, 3, 2, 4).reshape(n, 16, 25)
    ty = ty.reshape(n, 4, 5, 4, 5).transpose(0, 1, 3, 2, 4).reshape(n, 16, 25)
    acc = np.zeros((n, 16, 4), F)
    for t in range(25):
        acc = acc + np.stack([tx[:, :, t], ty[:, :, t], np.abs(tx[:, :, t]), np.abs(ty[:, :, t])], axis=2)
    out = acc.reshape(n, 64)
    q = out * out
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        q = q + q[:, lane ^ m]
    nrm = np.sqrt(q[:, :1])
    with np.errstate(all="ignore"):
        return np.where(nrm == 0, F(0), out / nrm).astype(F)


def describe(img, kps, p=None):
    """orientation (unless upright) and descriptors at the key points (x, y, size); the other fields pass through"""
    p = p or default_params()
    I = integral(np.ascontiguousarray(img, np.uint8))
    kps = np.array(kps, KEYPOINT)
    if len(kps) == 0:
        return kps, np.zeros((0, 64), F)
    if p["upright"]:
        kps["dir_x"], kps["dir_y"] = 1.0, 0.0
    else:
        kps["dir_x"], kps["dir_y"] = orientation(I, kps["x"], kps["y"], kps["size"])
    return kps, descriptor(I, kps["x"], kps["y"], kps["size"], kps["dir_x"], kps["dir_y"])


def detect_describe(img, p=None, cap=4096):
    p = p or default_params()
    return describe(img, detect(img, p, cap), p)


def angle_deg(dir_x, dir_y):
    """uwt_keypoint_angle_deg: atan2 in double, degrees in [0, 360)"""
    a = np.degrees(np.arctan2(np.float64(dir_y), np.float64(dir_x)))
    a = np.where(a < 0, a + 360.0, a)
    return np.where(a >= 360.0, 0.0, a)
