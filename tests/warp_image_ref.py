"""numpy restatement of Tracker::ObtainImageTransformed (src/Tracker.cpp:1473-1525) and of the image DebugShowWarpedPerspective builds
(:1694-1737), as include/uwt.h states them: the literal sequential loop, the same result through a winner plane, the integer sums of
uwt_warp_quality and the four-panel mosaic.  Test infrastructure: the library computes none of this here."""
import math

import numpy as np

LIMIT = 2147483520.0   # 2^31 - 128: the largest magnitude whose conversion to int the contract defines

QUALITY_FIELDS = ("status", "n_points", "n_landed", "n_covered", "sum_abs", "sum_sq", "sum_abs_unaligned", "reserved")


def c_round(u):
    """(int)round(u) of C for one float32 (halves away from zero), or None where the contract skips the row"""
    u = float(np.float32(u))
    if not math.isfinite(u) or abs(u) >= LIMIT:
        return None
    r = math.floor(abs(u) + 0.5)   # exact in double for a float32 u
    return int(r) if u >= 0 else -int(r)


def obtain_image_transformed(original, pts, warped, out):
    """The literal loop.  `out` is written in place; returns validPixel."""
    rows, cols = original.shape
    valid = np.zeros(out.shape, np.uint8)
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    warped = np.asarray(warped, np.float32).reshape(-1, 4)
    for i in range(warped.shape[0]):
        px, py = float(pts[i, 0]), float(pts[i, 1])
        if not (px > -1.0 and px < cols and py > -1.0 and py < rows):   # deviation: the reference would read out of bounds
            continue
        x1, y1 = int(px), int(py)   # truncation toward zero
        x2, y2 = c_round(warped[i, 0]), c_round(warped[i, 1])
        if x2 is None or y2 is None:   # deviation: the conversion is undefined
            continue
        if y2 > 0 and y2 < rows and x2 > 0 and x2 < cols:
            out[y2, x2] = original[y1, x1]
            valid[y2, x2] = 1
    return valid


def landing(original_shape, pts, warped):
    """Vectorised: (landed mask over rows, x1, y1, x2, y2); the coordinates are meaningful where the mask is set."""
    rows, cols = original_shape
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    warped = np.asarray(warped, np.float32).reshape(-1, 4)
    px, py = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        src_ok = (px > -1.0) & (px < cols) & (py > -1.0) & (py < rows)
        u, v = warped[:, 0].astype(np.float64), warped[:, 1].astype(np.float64)
        fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
    ok = src_ok & fin
    x1 = np.where(ok, np.trunc(np.where(ok, px, 0)), 0).astype(np.int64)
    y1 = np.where(ok, np.trunc(np.where(ok, py, 0)), 0).astype(np.int64)
    ru = np.where(ok, u, 0)
    rv = np.where(ok, v, 0)
    x2 = (np.sign(ru) * np.floor(np.abs(ru) + 0.5)).astype(np.int64)
    y2 = (np.sign(rv) * np.floor(np.abs(rv) + 0.5)).astype(np.int64)
    landed = ok & (y2 > 0) & (y2 < rows) & (x2 > 0) & (x2 < cols)
    return landed, x1, y1, x2, y2


def winner_form(original, pts, warped, out):
    """The same through an index plane: the largest landed i of each pixel (np.maximum.at), then one gather.  Writes `out` in place;
    returns (validPixel, n_landed)."""
    rows, cols = original.shape
    landed, x1, y1, x2, y2 = landing(original.shape, pts, warped)
    idx = np.nonzero(landed)[0]
    win = np.full(rows * cols, -1, np.int64)
    np.maximum.at(win, y2[idx] * cols + x2[idx], idx)
    win = win.reshape(rows, cols)
    cov = win >= 0
    w = win[cov]
    out[cov] = original[y1[w], x1[w]]
    return cov.astype(np.uint8), int(idx.size)


def quality(image1, image2, warped_img, valid, n_points, n_landed):
    """uwt_warp_quality in integers; also the |warped - image2| plane (0 where not covered)"""
    cov = valid.astype(bool)
    d = np.abs(warped_img.astype(np.int64) - image2.astype(np.int64))
    un = np.abs(image1.astype(np.int64) - image2.astype(np.int64))
    q = dict(status=0, n_points=int(n_points), n_landed=int(n_landed), n_covered=int(cov.sum()), sum_abs=int(d[cov].sum()),
             sum_sq=int((d[cov] ** 2).sum()), sum_abs_unaligned=int(un[cov].sum()), reserved=0)
    return q, np.where(cov, d, 0).astype(np.uint8)


def blend(a, b):
    """addWeighted(a, 0.5, b, 0.5, 1.0) on u8 in integers: saturate(cvRound(0.5 a + 0.5 b + 1)), halves to the even neighbour"""
    s = np.asarray(a, np.int64) + np.asarray(b, np.int64)
    m = s // 2 + 1
    m = np.where(s % 2 == 1, m + (m % 2), m)   # m + 0.5 -> the even one of m, m + 1
    return np.minimum(m, 255).astype(np.uint8)


def mosaic(image1, image2, warped_img):
    """[image1 | image2] over [blend(warped, image2) | blend(image1, image2)]"""
    return np.vstack([np.hstack([image1, image2]), np.hstack([blend(warped_img, image2), blend(image1, image2)])])


def dense_table(O, p, lvl, depth_lvl, pose):
    """ObtainAllPoints and WarpFunction of the oracle for one level: (L, pts, warped); depth_lvl: the reference frame's depth image at
    that level (its own row length), or None"""
    L = O.level_intrinsics(p, lvl)
    pts = O.dense_points(depth_lvl, L.w, L.h, lvl, p.depth_scale)
    return L, pts, O.warp(pts, np.asarray(pose, np.float32), L)


def dense_reference(O, p, lvl, image1, image2, depth_lvl, pose):
    """What uwt_warp_image_batch states for one pair: dict(warped, valid, absdiff, quality)"""
    L, pts, wp = dense_table(O, p, lvl, depth_lvl, pose)
    out = np.zeros(image1.shape, np.uint8)
    valid, n_landed = winner_form(image1, pts, wp, out)
    q, d = quality(image1, image2, out, valid, pts.shape[0], n_landed)
    return dict(warped=out, valid=valid, absdiff=d, quality=q)
