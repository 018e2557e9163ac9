"""The specification of the seeded calls (include/uwt.h "seeded calls") restated on the CPU.  A helper of the tests, not a test.

align: the loop of uwo_estimate_pose_points (oracle/uwt_oracle.c:853-940) written out over the oracle's STAGE functions — pyramid,
scharr3, dense_points, warp, residual_jacobian_ex, tukey_weights / huber_weights, error, normal_equations, solve_delta, se3_exp,
se3_mul, se3_handoff — with two things the oracle's own loop does not have: the pose in front of the first evaluation (`seed`, used
exactly as given; None = the identity of src/Tracker.cpp:385) and the hand-off choice (`keep`: the pose crosses every level boundary
unchanged).  With seed None and keep False it gives the bits of oracle.align_pair / align_pair_points (tests/test_seeded_ref_cpu.py).

predict_seeds: uwt_predict_seeds_device_async in numpy, operation by operation as the header lists them.
"""
import numpy as np

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
ERR_INVALID_ARG, ERR_NO_VALID_POINTS = 1, 2
TRANSLATION_MAX = np.float32(2.0 ** 125)   # include/uwt.h: UWT_TRANSLATION_MAX


def frame_planes(O, p, gray, depth=None):
    """images_, gradientX_ / gradientY_ and depths_ of one frame on every level: System::AddFrame's pyramid + Tracker::ApplyGradient"""
    imgs = O.pyramid(np.ascontiguousarray(gray, np.uint8), p.n_levels)
    grads = [O.scharr3(im) for im in imgs]
    deps = O.pyramid(np.ascontiguousarray(depth, np.uint16), p.n_levels) if depth is not None else None
    return imgs, grads, deps


def align(O, p, ref_gray, tgt_gray, ref_depth=None, seed=None, keep=False, tables=None):
    """Tracker::EstimatePose over dense points (tables None) or explicit per-level tables ({level: n x 4}) from `seed`.
    Returns (status, pose [7] float32, trace): trace one dict per evaluation — level, iter, n_valid, error, exited, pose (the pose
    behind the evaluation's update, or the unchanged one where it exited), as oracle.align_pair's.
    A seed with a non-finite entry, or with a translation entry above UWT_TRANSLATION_MAX = 2^125 in magnitude: (ERR_INVALID_ARG, the
    identity, []) — the pair runs no evaluation."""
    if seed is not None and not (np.isfinite(np.asarray(seed, np.float32)).all() and
                                 (np.abs(np.asarray(seed, np.float32).reshape(7)[4:]) <= TRANSLATION_MAX).all()):
        return ERR_INVALID_ARG, IDENTITY.copy(), []
    prev = O.set_arith(p.arith)
    try:
        return _align(O, p, ref_gray, tgt_gray, ref_depth, seed, keep, tables)
    finally:
        O.set_arith(prev)


def _align(O, p, ref_gray, tgt_gray, ref_depth, seed, keep, tables):
    depth = ref_depth if p.has_depth else None
    rimg, rgrad, rdep = frame_planes(O, p, ref_gray, depth)
    timg = O.pyramid(np.ascontiguousarray(tgt_gray, np.uint8), p.n_levels)
    pose = IDENTITY.copy() if seed is None else np.array(seed, np.float32).reshape(7)   # :385, or the seed as it is
    trace, status = [], 0
    for lvl in range(p.first_level, p.last_level - 1, -1):   # :389
        L = O.level_intrinsics(p, lvl)
        last_error = np.float32(p.initial_error)             # :393
        if tables is not None:
            pts = np.ascontiguousarray(tables[lvl], np.float32).reshape(-1, 4)
        else:
            pts = O.dense_points(rdep[lvl] if rdep is not None else None, L.w, L.h, lvl, p.depth_scale)
        for k in range(p.max_iters):                         # :414
            warped = O.warp(pts, pose, L) if len(pts) else np.zeros((0, 4), np.float32)
            if len(pts):
                J, r, _ = O.residual_jacobian_ex(rimg[lvl], timg[lvl], rgrad[lvl][0], rgrad[lvl][1], pts, warped, L, p.z_factor,
                                                 p.angle_factor, p.sampler)
            else:
                r = np.zeros(0, np.float32)
            if len(r) == 0:
                status = ERR_NO_VALID_POINTS
                break
            W = O.tukey_weights(r) if p.weights == 1 else O.huber_weights(r) if p.weights == 2 else None   # :495-496
            err = np.float32(O.error(r, W)[0])               # :499-502
            row = dict(level=lvl, iter=k, n_valid=len(r), error=err, exited=0)
            if p.early_exit and (err >= last_error or k == p.max_iters - 1 or abs(np.float32(err - last_error)) < np.float32(p.epsilon)):
                row.update(exited=1, pose=pose.copy())       # :508
                trace.append(row)
                break
            last_error = err                                 # :529
            A, b = O.normal_equations(J, r, W, p.gain)       # :554-561
            pose = O.se3_mul(pose, O.se3_exp(O.solve_delta(A, b)))   # :564, :574
            row["pose"] = pose.copy()
            trace.append(row)
        if status:
            break
        if lvl != 0 and not keep:                            # :580-590; keep: the pose crosses unchanged
            try:
                pose = O.se3_handoff(pose, p.handoff_scale_t)
            except ValueError:
                status = ERR_INVALID_ARG
    return status, pose, trace


def stats_of(status, trace):
    """uwt_stats of a result: (status, evaluations over all levels, valid points and error bits of the last evaluation)"""
    if not trace:
        return (status, 0, 0, 0)
    return (status, len(trace), trace[-1]["n_valid"], int(np.float32(trace[-1]["error"]).view(np.uint32)))


def level_evaluations(trace):
    """{level: evaluations the pair spent on it}"""
    out = {}
    for t in trace:
        out[t["level"]] = out.get(t["level"], 0) + 1
    return out


def quat_to_rot(q):
    """the rotation uwt_se3_matrix gives (Eigen's toRotationMatrix), float32 operation by operation, row-major [9]"""
    f = np.float32
    x, y, z, w = (f(v) for v in q)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([f(1) - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, f(1) - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, f(1) - (txx + tyy)], np.float32)


def se3_inverse(pose):
    """the inverse as uwt_predict_seeds_device_async defines it: the conjugate, and each translation row formed in f64 in the order
    ((R0 t0 + R1 t1) + R2 t2), negated, rounded once"""
    pose = np.asarray(pose, np.float32)
    qi = np.array([-pose[0], -pose[1], -pose[2], pose[3]], np.float32)
    R = quat_to_rot(qi).astype(np.float64)
    t = pose[4:].astype(np.float64)
    ti = [np.float32(-((R[3 * k] * t[0] + R[3 * k + 1] * t[1]) + R[3 * k + 2] * t[2])) for k in range(3)]
    return np.concatenate([qi, np.array(ti, np.float32)])


def predict_seeds(O, prev, cur):
    """seed_i = (cur_i * prev_i^-1) * cur_i, the products uwt_se3_mul's; a non-finite input row gives an all-NaN row"""
    prev = np.asarray(prev, np.float32).reshape(-1, 7)
    cur = np.asarray(cur, np.float32).reshape(-1, 7)
    out = np.empty_like(cur)
    with np.errstate(all="ignore"):
        for i in range(len(cur)):
            if not (np.isfinite(prev[i]).all() and np.isfinite(cur[i]).all()):
                out[i] = np.float32(np.nan)
                continue
            out[i] = O.se3_mul(O.se3_mul(cur[i], se3_inverse(prev[i])), cur[i])
    return out
