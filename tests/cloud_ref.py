"""numpy restatement of the point-cloud map as include/uwt.h states it: Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446)
for one table — the column operations of :429-434 and the loop of :437-445 — in both modes, both unprojections in f32, the f64 row
product of the world mode, and the bookkeeping of a batch (offsets, the records, the cap).  Test infrastructure: the library computes
none of this here.  Tables come from oracle.dense_points / oracle.candidate_points, the rigid matrix from oracle.se3_matrix."""
import numpy as np

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tag", "<u4")])   # uwt_cloud_point
INFO_FIELDS = ("status", "n_rows", "n_selected", "n_points", "offset", "written")   # uwt_cloud_info
OK, INVALID_ARG, CAPACITY = 0, 1, 5   # uwt_status_code


def unproject(pts, L, arith):
    """X = ((x - cx) invfx) z, Y = ((y - cy) invfy) z of every row, f32 operation by f32 operation.  arith "legacy": as written;
    "opencv": the MatExpr-folded x * invfx + (float)(-(double)cx * invfx)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    cx, cy, ifx, ify = np.float32(L.cx), np.float32(L.cy), np.float32(L.invfx), np.float32(L.invfy)
    with np.errstate(all="ignore"):
        if arith == "legacy":
            X = (x - cx) * ifx
            Y = (y - cy) * ify
        else:
            bx = np.float32(-float(cx) * float(ifx))
            by = np.float32(-float(cy) * float(ify))
            X = x * ifx
            X = X + bx
            Y = y * ify
            Y = Y + by
        X = X * z
        Y = Y * z
    assert X.dtype == np.float32 and Y.dtype == np.float32
    return X, Y, z.copy()


def rigid_rows_f64(T, X, Y, Z, w):
    """(float)(T0 X + ((T1 Y + T2 Z) + T3 w)) for the first three rows of T, formed in f64 (one definition for both sets)"""
    T = np.asarray(T, np.float32).astype(np.float64)
    X, Y, Z, w = (np.asarray(v, np.float32).astype(np.float64) for v in (X, Y, Z, w))
    with np.errstate(all="ignore"):
        return [(T[k, 0] * X + ((T[k, 1] * Y + T[k, 2] * Z) + T[k, 3] * w)).astype(np.float32) for k in range(3)]


def intensities(pts, image):
    """image[(int)y][(int)x] (truncation toward zero), 0 outside the image or for a coordinate that is not a number"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    rows, cols = image.shape
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x > -1.0) & (x < cols) & (y > -1.0) & (y < rows)
    xi = np.trunc(np.where(ok, x, 0)).astype(np.int64)
    yi = np.trunc(np.where(ok, y, 0)).astype(np.int64)
    return np.where(ok, image[yi, xi], 0).astype(np.uint32)


def pose_finite(pose):
    return bool(np.all(np.isfinite(np.asarray(pose, np.float32))))


def frame_points(O, pts, pose, L, arith, mode=0, image=None, frame_index=0):
    """Every row of a table as a record (no selection yet): the reference's column operations, then the point of each mode"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    pose = np.asarray(pose, np.float32)
    X, Y, Z = unproject(pts, L, arith)
    out = np.zeros(pts.shape[0], POINT)
    with np.errstate(all="ignore"):
        if mode == 0:
            out["x"] = (-X) - pose[4]
            out["y"] = (-Z) - pose[6]
            out["z"] = (-Y) - pose[5]
        else:
            out["x"], out["y"], out["z"] = rigid_rows_f64(O.se3_matrix(pose), X, Y, Z, pts[:, 3])
    inten = intensities(pts, image) if image is not None else np.zeros(pts.shape[0], np.uint32)
    out["tag"] = inten | np.uint32(frame_index << 8)
    return out


def visualizer_loop(O, pts, pose, L, arith, mode=0, stride=100, skip_invalid=0, image=None, frame_index=0):
    """The loop of src/Visualizer.cpp:437-445, literally: for (i = 0; i < rows; i += stride) push_back.  Returns (records, n_selected)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    every = frame_points(O, pts, pose, L, arith, mode, image, frame_index)
    cloud, n_selected = [], 0
    i = 0
    while i < pts.shape[0]:
        n_selected += 1
        if not (skip_invalid and pts[i, 3] == 0):
            cloud.append(every[i])
        i += stride
    return (np.array(cloud, POINT) if cloud else np.zeros(0, POINT)), n_selected


def frame_cloud(O, pts, pose, L, arith, mode=0, stride=100, skip_invalid=0, image=None, frame_index=0):
    """The same with the selection vectorised (equal to visualizer_loop, pinned in tests/test_cloud_ref_cpu.py)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    sel = np.arange(0, pts.shape[0], stride)
    rec = frame_points(O, pts[sel], pose, L, arith, mode, image, frame_index)
    if skip_invalid:
        rec = rec[~(pts[sel, 3] == 0)]
    return rec, int(sel.size)


def batch_cloud(O, frames, L, arith, mode=0, stride=100, skip_invalid=0, cap=None):
    """A call over frames = [(table, pose, image or None), ...]: (records in cloud order, the FULL cloud; info: a list of per-frame
    tuples in INFO_FIELDS order; call: the call's tuple).  cap None: room for everything."""
    parts, info, offset = [], [], 0
    for f, (pts, pose, image) in enumerate(frames):
        if pose_finite(pose):
            rec, n_sel = frame_cloud(O, pts, pose, L, arith, mode, stride, skip_invalid, image, f)
            row = [OK, int(np.asarray(pts).reshape(-1, 4).shape[0]), n_sel, int(rec.size)]
        else:   # deviation: a pose with a non-finite entry contributes nothing
            rec, row = np.zeros(0, POINT), [INVALID_ARG, 0, 0, 0]
        parts.append(rec)
        info.append(row + [offset])
        offset += int(rec.size)
    total = offset
    room = total if cap is None else cap
    info = [tuple(r + [min(max(room - r[4], 0), r[3])]) for r in info]
    call = (CAPACITY if total > room else OK, len(frames), 0, 0, total, min(total, room))
    return (np.concatenate(parts) if parts else np.zeros(0, POINT)), info, call
