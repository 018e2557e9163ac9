"""The sparse point producers restated in plain numpy: Tracker::ObtainCandidatePoints with gradient_ (src/Tracker.cpp:1139-1142,
1314-1362), ObtainPatchesPoints (:1178-1257) and AddPatchPointsFeatures (:599-629).  Integers and float64 throughout; the float32 steps
the reference takes are written out as np.float32 operations.  Independent of the C oracle; tests/test_points_cpu.py asserts the two equal
bit for bit on every case of tests/points_cases.py.

MUTANTS names deliberate mistakes: every function takes mut=<name> and then computes what an implementation with that one mistake would.
A mutant that a function does not know leaves it unchanged.

Not a mutant, because it is EQUIVALENT — `floor` for the truncating cast (int)(x - 5).  Proof: let v = x - 5 (or round(x) - start) in
float32.  floor(v) and (int)v differ only for v < 0 and not an integer, and then floor(v) = (int)v - 1 <= -1.  The loop that starts one
cell earlier visits exactly one more cell, i = floor(v) <= -1, and the cell test `i > 0` (:1206, :613) rejects it; every other cell is
visited by both loops in the same order.  The same holds for j.  So rows, order and count are the same for every float32 input."""
import numpy as np

F32 = np.float32
DEPTH_FACTOR = F32(0.0002)          # factor_depth (:1189, :1320)
MAX_KEYPOINTS = 200                 # min(num_max_keypoints, 200) (:1194)
K_BLOCK = 256                       # the candidate kernels' block: columns per column block

MUTANTS = {
    # candidate selection
    "ge_for_gt": "gradient_ >= mean + threshold",
    "compare_f32": "the comparison made in float32",
    "mean_over_pitch": "the mean taken over pitch x ih elements (pad columns counted as zeros)",
    "mean_over_grid": "the mean taken over the gw x gh point grid instead of the iw x ih image",
    # magnitude
    "half_up": "(|gx| + |gy|) / 2 rounded half up instead of half to even",
    "saturate_after": "|g| saturated to 255 after the halving instead of each side before it",
    # depth and order
    "depth_low_byte_of_pixel": "the depth byte is the low byte of pixel x, not byte x of the row",
    "z_scaled_by_level": "z = byte * 0.0002 / 2^lvl",
    "y_major": "rows pushed y outer, x inner",
    "band_row_lost": "the first row of every row band but the first is skipped",
    "band_row_doubled": "the first row of every row band but the first is also taken by the band above it",
    # patches
    "i_ge_0": "cells with i >= 0 and j >= 0 kept",
    "i_le_w": "cells with i <= w and j <= h kept",
    "upper_lt": "(float)i < x + 5 at the upper patch bound",
    "depth_unsigned": "the key point's depth read as unsigned 16 bit",
    "d_le_0_skips": "key points with depth <= 0 skipped",
    "kp_201_used": "no cut at 200 key points",
    "patch_y_outer": "patch cells pushed y outer, x inner",
    # add_patch_points
    "rint_for_roundf": "round half to even instead of half away from zero",
    "centre_kept": "the centre cell is not excluded",
    "centre_by_unrounded": "the centre excluded by the unrounded coordinates",
    "count_clipped_at_cap": "the returned count clipped at cap",
}


def gradient_magnitude(gx, gy, mut=None):
    """gradient_ = addWeighted(convertScaleAbs(gx), 0.5, convertScaleAbs(gy), 0.5): each side saturated to u8 first, the half sum rounded
    half to even (cvRound)."""
    ax = np.abs(np.asarray(gx, np.int64))
    ay = np.abs(np.asarray(gy, np.int64))
    if mut != "saturate_after":
        ax, ay = np.minimum(ax, 255), np.minimum(ay, 255)
    s = ax + ay
    m = s >> 1
    if mut == "half_up":
        m = m + (s & 1)
    else:
        m = m + ((s & 1) & (m & 1))      # x.5 goes to the even neighbour
    return np.minimum(m, 255).astype(np.uint8)


def pitch_of(iw):
    """device rows are pitched to whole groups of four elements"""
    return (iw + 3) // 4 * 4


def bands_of(gw, gh, n_frames):
    """the row bands of the device's candidate producer for n_frames frames in one call: (bands, rows per band)"""
    col_blocks = (gw + K_BLOCK - 1) // K_BLOCK
    bands = max(1, min(gh // 8, 512 // max(1, col_blocks * n_frames)))
    return bands, (gh + bands - 1) // bands


def candidate_mean(mag, grid=None, mut=None):
    """cuda::meanStdDev over the whole gradient_ Mat: an integer sum, one float64 division"""
    mag = np.asarray(mag, np.uint8)
    ih, iw = mag.shape
    gw, gh = grid if grid is not None else (iw, ih)
    if mut == "mean_over_grid":
        return float(int(mag[:gh, :gw].astype(np.int64).sum())) / float(gw * gh)
    total = int(mag.astype(np.int64).sum())
    if mut == "mean_over_pitch":
        return float(total) / float(pitch_of(iw) * ih)
    return float(total) / float(iw * ih)


def depth_bytes(depth):
    """at<uchar>(y, x) of a 16-bit image: byte x of row y, for x below the image width (little endian: even x the low byte of pixel
    x / 2, odd x its high byte)"""
    depth = np.ascontiguousarray(depth, "<u2")
    return depth.view(np.uint8).reshape(depth.shape[0], 2 * depth.shape[1])[:, :depth.shape[1]]


def candidate_points(mag, depth=None, threshold=20.0, grid=None, lvl=0, n_frames=1, mut=None):
    """mag: the level's gradient_ (ih x iw, u8); depth: its 16-bit plane or None; grid = (gw, gh): the level's point grid.  n_frames
    only matters to the two band mutants (the band split depends on the call's frame count).  Returns (rows [n, 4] float32, n)."""
    mag = np.asarray(mag, np.uint8)
    ih, iw = mag.shape
    gw, gh = grid if grid is not None else (iw, ih)
    thres = candidate_mean(mag, (gw, gh), mut) + float(threshold)          # float64 (:1325-1327)
    cells = mag[:gh, :gw]
    if mut == "compare_f32":
        with np.errstate(over="ignore"):
            keep = cells.astype(F32) > F32(thres)
    elif mut == "ge_for_gt":
        keep = cells.astype(np.float64) >= thres
    else:
        keep = cells.astype(np.float64) > thres
    z = np.ones((gh, gw), F32)
    if depth is not None:
        if mut == "depth_low_byte_of_pixel":
            b = (np.asarray(depth, np.uint16)[:gh, :gw] & 0xFF).astype(np.uint8)
        else:
            b = depth_bytes(depth)[:gh, :gw]
        keep = keep & (b != 0)
        z = b.astype(F32) * DEPTH_FACTOR                                   # float32 product, no level factor (:1344)
        if mut == "z_scaled_by_level":
            z = z * F32(1.0 / 2.0 ** lvl)
    ys = np.arange(gh)
    if mut in ("band_row_lost", "band_row_doubled"):
        bands, rows = bands_of(gw, gh, n_frames)
        first = ys[(ys % rows == 0) & (ys > 0)]
        ys = np.setdiff1d(ys, first) if mut == "band_row_lost" else np.sort(np.concatenate([ys, first]))
    if mut == "y_major":
        yy, xx = np.meshgrid(ys, np.arange(gw), indexing="ij")
    else:
        xx, yy = np.meshgrid(np.arange(gw), ys, indexing="ij")            # x outer, y inner (:1334-1335)
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    k = keep[yy, xx]
    xx, yy = xx[k], yy[k]
    out = np.empty((xx.size, 4), F32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = xx, yy, z[yy, xx], 1.0
    return out, int(xx.size)


def _patch_range(c, start, mut):
    """the loop `for (i = (int)(c - start); (float)i <= c + start; i++)` with c and start float32: (first i, last i)"""
    lo = int(np.trunc(F32(c) - F32(start)))          # float32 difference, truncating cast
    top = float(F32(c) + F32(start))                 # float32 sum; (float)i is exact for these i, so the comparison is one of reals
    hi = int(np.floor(top))
    if mut == "upper_lt" and hi == top:
        hi -= 1
    return lo, hi


def _patch_cells(x, y, start, w, h, mut, y_outer=False):
    """the cells of one patch in push_back order, strictly inside the level: (i, j) integer arrays"""
    ilo, ihi = _patch_range(x, start, mut)
    jlo, jhi = _patch_range(y, start, mut)
    i0, j0 = (0, 0) if mut == "i_ge_0" else (1, 1)
    i1, j1 = (w, h) if mut == "i_le_w" else (w - 1, h - 1)
    ii = np.arange(max(ilo, i0), min(ihi, i1) + 1)
    jj = np.arange(max(jlo, j0), min(jhi, j1) + 1)
    if y_outer:
        J, I = np.meshgrid(jj, ii, indexing="ij")
    else:
        I, J = np.meshgrid(ii, jj, indexing="ij")   # x outer, y inner (:1204-1206, :611-612)
    return I.reshape(-1), J.reshape(-1)


def patch_points(kp, depth0, w, h, cap=None, mut=None):
    """kp: [n, 2] float32 (x, y) with 0 <= x < w, 0 <= y < h (-0.0 included); depth0: level 0's 16-bit plane or None.  Returns
    (rows [min(n, cap), 4], the full count n)."""
    kp = np.asarray(kp, F32).reshape(-1, 2)
    n_used = kp.shape[0] if mut == "kp_201_used" else min(kp.shape[0], MAX_KEYPOINTS)
    parts = []
    for q in range(n_used):
        x, y = kp[q]
        z = F32(1.0)
        if depth0 is not None:
            d = int(np.asarray(depth0, np.uint16)[int(y), int(x)])        # at<short>((int)y, (int)x): truncation
            if mut != "depth_unsigned" and d >= 0x8000:
                d -= 0x10000
            if d == 0 or (mut == "d_le_0_skips" and d < 0):
                continue
            z = F32(d) * DEPTH_FACTOR * F32(1.0)                          # float32 products (:1204)
        I, J = _patch_cells(x, y, 5, w, h, mut, y_outer=mut == "patch_y_outer")
        rows = np.empty((I.size, 4), F32)
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = I, J, z, 1.0
        parts.append(rows)
    out = np.concatenate(parts) if parts else np.zeros((0, 4), F32)
    n = out.shape[0]
    return (out if cap is None else out[:cap]).copy(), n


def c_roundf(v):
    """roundf of float32 values: half away from zero (exact: |v| + 0.5 is taken in float64)"""
    v = np.asarray(v, F32).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(F32)


def add_patch_points(pts, w, h, patch_size=5, cap=None, mut=None):
    """pts: [n, 4] float32 rows of one level (w x h).  Returns (rows [min(count, cap), 4], the full count)."""
    pts = np.asarray(pts, F32).reshape(-1, 4)
    start = (patch_size - 1) // 2
    parts = [pts.copy()]                                                   # candidatePoints.clone() (:601)
    for q in range(pts.shape[0]):
        if mut == "rint_for_roundf":
            x, y = F32(np.rint(pts[q, 0])), F32(np.rint(pts[q, 1]))
        else:
            x, y = c_roundf(pts[q, 0]), c_roundf(pts[q, 1])                # (:607-608)
        I, J = _patch_cells(x, y, start, w, h, mut)
        if mut == "centre_kept":
            keep = np.ones(I.size, bool)
        elif mut == "centre_by_unrounded":
            keep = ~((I.astype(F32) == pts[q, 0]) & (J.astype(F32) == pts[q, 1]))
        else:
            keep = ~((I.astype(F32) == x) & (J.astype(F32) == y))          # (:613)
        rows = np.empty((int(keep.sum()), 4), F32)
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = I[keep], J[keep], pts[q, 2], 1.0
        parts.append(rows)
    out = np.concatenate(parts)
    n = out.shape[0]
    if cap is not None:
        out = out[:cap]
        if mut == "count_clipped_at_cap":
            n = min(n, cap)
    return out.copy(), n


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
