"""Designed inputs of the depth-sweep tests (tests/test_depth_sweep_cpu.py shows on the restatement alone what they reach;
tests/test_gpu_depth_sweep.py runs the same cases on the device).  A case is a textured plane seen from a reference camera and 1..4
views rendered through the plane's homography (as synth.render_pair renders), the views' poses in the tracker's convention
X_view = T X_ref, the depth codes and the sweep's parameters.  Small frames: 64 x 48 (pitch = width) and 61 x 45 (pitch 64, odd rows,
img_w > w at level 1)."""
import numpy as np
from scipy import ndimage

import depth_sweep_ref as SR

INTR = {(64, 48): (52.5, 52.5, 31.5, 23.5), (61, 45): (50.0, 50.0, 30.0, 22.0), (320, 240): (262.5, 262.5, 159.5, 119.5)}
DEPTH_SCALE = 0.0002
N_LEVELS = 2


def render_view(synth, ref, intr, rvec, t, z):
    """(view u8, pose [7] f32): view(u') = ref(H^-1 u'), H = K (R + t n^T / z) K^-1, for the plane at depth z in front of ref"""
    fx, fy, cx, cy = intr
    h, w = ref.shape
    R = synth.rodrigues(np.asarray(rvec, np.float64))
    t = np.asarray(t, np.float64)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Hi = np.linalg.inv(K @ (R + np.outer(t, [0, 0, 1.0]) / z) @ np.linalg.inv(K))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    den = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
    u = (Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]) / den
    v = (Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]) / den
    img = ndimage.map_coordinates(ref.astype(np.float32), [v, u], order=1, mode="reflect")
    pose = np.concatenate([synth._quat_from_R(R), t]).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), pose


def axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    return a / np.linalg.norm(a) * np.deg2rad(deg)


ROT = axis_angle((0.3, -0.5, 0.8), 0.5)
CODES32 = SR.hypotheses(0.5, 2.5, DEPTH_SCALE, 32)

# name -> size, plane depth, texture seed and blur, the views' (rotation vector, translation), the codes, the parameters that differ from
# the defaults (source 0 unless named), and what is done to the images afterwards
CASES = {
    "one_view_32": dict(size=(64, 48), z=1.0, seed=21, views=[(ROT, (0.25, 0.05, 0.0))], codes=CODES32, params=dict(source=0)),
    "two_views_64_ties": dict(size=(64, 48), z=1.1, seed=22, views=[(ROT, (0.1, 0.0, 0.0)), (-ROT, (-0.08, 0.03, 0.0))],
                              codes=SR.hypotheses(0.5, 2.5, DEPTH_SCALE, 64), params=dict(source=0, radius=1, refine=0)),
    "two_views_64_refined": dict(size=(61, 45), z=0.9, seed=23, views=[(ROT, (0.12, 0.0, 0.0)), (-ROT, (-0.1, -0.04, 0.0))],
                                 codes=SR.hypotheses(0.5, 2.5, DEPTH_SCALE, 64), params=dict(source=0, radius=2)),
    "four_views_17": dict(size=(61, 45), z=1.3, seed=24,
                          views=[(ROT, (0.2, 0.0, 0.0)), (-ROT, (-0.2, 0.0, 0.01)), (0 * ROT, (0.0, 0.18, 0.0)), (ROT, (0.1, -0.15, 0.0))],
                          codes=SR.hypotheses(0.6, 3.0, DEPTH_SCALE, 17), params=dict(source=1, threshold=2.0)),
    "level1_3": dict(size=(64, 48), z=1.0, seed=25, views=[(0 * ROT, (0.3, 0.0, 0.0))], codes=np.array([5000, 10000, 20000], np.uint16),
                     params=dict(source=0, lvl=1, radius=1)),
    "odd_level1_32": dict(size=(61, 45), z=1.6, seed=26, views=[(ROT, (0.3, 0.1, 0.0)), (-ROT, (-0.25, 0.0, 0.0))],
                          codes=SR.hypotheses(0.5, 2.5, DEPTH_SCALE / 2, 32), params=dict(source=1, threshold=0.0, lvl=1)),
    "parallax_mixed": dict(size=(64, 48), z=0.8, seed=27, views=[(0 * ROT, (0.004, 0.0, 0.0)), (ROT, (0.2, 0.0, 0.0))], codes=CODES32,
                           params=dict(source=0)),
    "low_parallax": dict(size=(61, 45), z=1.0, seed=28, views=[(ROT, (0.01, 0.0, 0.0))], codes=CODES32, params=dict(source=0, radius=1)),
    "behind": dict(size=(64, 48), z=1.0, seed=29, views=[(ROT, (0.2, 0.0, 0.0)), (0 * ROT, (0.02, 0.0, -0.8))], codes=CODES32,
                   params=dict(source=0, radius=1)),
    "poor": dict(size=(64, 48), z=1.0, seed=30, views=[(ROT, (0.2, 0.02, 0.0))], codes=CODES32, params=dict(source=1, threshold=5.0),
                 noise=40),
    "flat": dict(size=(61, 45), z=1.0, seed=31, views=[(0 * ROT, (0.2, 0.0, 0.0))], codes=CODES32, params=dict(source=0), flat=True),
}

_built = {}


def build(synth, name):
    """dict(size, intr, frames [1 + n_views] u8 level-0 images (the reference first), poses [n_views, 7] f32, codes u16, params dict)"""
    if name not in _built:
        c = CASES[name]
        w, h = c["size"]
        intr = INTR[(w, h)]
        ref = synth.texture(w, h, c["seed"], sigma=1.5)
        frames, poses = [ref], []
        for rvec, t in c["views"]:
            img, pose = render_view(synth, ref, intr, rvec, t, c["z"])
            frames.append(img)
            poses.append(pose)
        if c.get("noise"):   # the views no longer match: mean absolute differences above max_mean_abs
            rng = np.random.default_rng(c["seed"])
            for i in range(1, len(frames)):
                frames[i] = np.clip(frames[i].astype(np.int64) + rng.integers(-c["noise"], c["noise"] + 1, frames[i].shape), 0, 255).astype(np.uint8)
        if c.get("flat"):   # a constant block in every frame: all costs 0 there, uniq_den * cost == uniq_num * c2
            for f in frames:
                f[10:36, 8:52] = 77
        params = dict(SR.DEFAULTS)
        params.update(c["params"])
        _built[name] = dict(size=(w, h), intr=intr, frames=frames, poses=np.stack(poses), codes=np.asarray(c["codes"], np.uint16),
                            params=params)
    return _built[name]


def oracle_params(O, case):
    w, h = case["size"]
    return O.default_params(w, h, *case["intr"], n_levels=N_LEVELS, first_level=N_LEVELS - 1, last_level=0, has_depth=0,
                            depth_scale=DEPTH_SCALE)


def level_images(O, case):
    """the case's frames at its level, as the device's pyramid holds them (oracle.pyramid)"""
    lvl = case["params"]["lvl"]
    return [O.pyramid(f, N_LEVELS)[lvl] for f in case["frames"]]


_refs = {}


def reference(O, arith, synth, name, variant=None):
    """the restatement's result of a case under the active arithmetic set, computed once"""
    key = (name, arith, variant)
    if key not in _refs:
        case = build(synth, name)
        imgs = level_images(O, case)
        _refs[key] = SR.sweep(O, oracle_params(O, case), imgs[0], imgs[1:], case["poses"], case["codes"], variant=variant, **case["params"])
    return _refs[key]
