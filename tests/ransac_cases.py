"""Inputs of the RANSAC tests (tests/test_ransac_ref_cpu.py, tests/test_gpu_ransac.py): synthetic two-view scenes with known inliers,
and constructed cases with known answers.  Everything is generated from fixed seeds; nothing here calls the library."""
import numpy as np

import ransac_ref as R

W, H, FX, FY, CX, CY = 640, 480, 525.0, 525.0, 319.5, 239.5


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(seed, n, outliers=0.3, noise=0.3, motion="general", planar=False):
    """Two views of n random 3-D points (depth 1..6, seen by both pinhole 640 x 480 cameras), Gaussian pixel noise, a share of the
    matches replaced by uniform random points in the second view.  Returns (matches, kp_prev [n, 2] f32, kp_cur [n, 2] f32, truth
    [n] bool: the match is a true correspondence).  The key points of the second frame are shuffled, so the match indices are not
    the identity."""
    rng = np.random.default_rng(seed)
    if motion == "general":
        Rm, t = rodrigues(rng.normal(0, 0.03, 3)), rng.normal(0, 0.15, 3)
    elif motion == "x":
        Rm, t = np.eye(3), np.array([0.2, 0.0, 0.0])
    elif motion == "forward":
        Rm, t = np.eye(3), np.array([0.0, 0.0, 0.25])
    elif motion == "none":
        Rm, t = np.eye(3), np.zeros(3)
    else:
        raise ValueError(motion)
    p0 = np.zeros((0, 2))
    p1 = np.zeros((0, 2))
    while p0.shape[0] < n:
        z = rng.uniform(1, 6, 4 * n)
        u, v = rng.uniform(0, W, 4 * n), rng.uniform(0, H, 4 * n)
        if planar:
            z = 3.0 + 0.002 * (u - CX) + 0.001 * (v - CY)
        X = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
        Y = X @ Rm.T + t
        u1, v1 = FX * Y[:, 0] / Y[:, 2] + CX, FY * Y[:, 1] / Y[:, 2] + CY
        ok = (Y[:, 2] > 0.1) & (u1 >= 0) & (u1 < W) & (v1 >= 0) & (v1 < H)
        p0 = np.concatenate([p0, np.stack([u, v], axis=1)[ok]])
        p1 = np.concatenate([p1, np.stack([u1, v1], axis=1)[ok]])
    p0, p1 = p0[:n], p1[:n]
    p0 = p0 + rng.normal(0, noise, p0.shape) if noise else p0
    p1 = p1 + rng.normal(0, noise, p1.shape) if noise else p1
    truth = np.ones(n, bool)
    bad = rng.permutation(n)[:int(round(outliers * n))]
    truth[bad] = False
    p1[bad] = np.stack([rng.uniform(0, W, bad.size), rng.uniform(0, H, bad.size)], axis=1)
    perm = rng.permutation(n)            # key point j of the current frame is point perm[j]
    inv = np.argsort(perm)
    matches = np.zeros(n, R.MATCH)
    matches["query_idx"] = np.arange(n)
    matches["train_idx"] = inv
    matches["distance"] = rng.uniform(0, 1, n).astype(np.float32)
    return matches, p0.astype(np.float32), p1[perm].astype(np.float32), truth


# (name, N, outlier share, noise, motion, planar, number of scenes): the families of the issue's table
FAMILIES = [
    ("n200_o30", 200, 0.30, 0.3, "general", False, 6),
    ("n200_o50", 200, 0.50, 0.3, "general", False, 4),
    ("n2000_o30", 2000, 0.30, 0.3, "general", False, 4),
    ("n2000_o45", 2000, 0.45, 0.5, "general", False, 4),
    ("n4096_o20", 4096, 0.20, 0.3, "general", False, 4),
    ("n8_clean", 8, 0.0, 0.2, "general", False, 4),
    ("n9_clean", 9, 0.0, 0.2, "general", False, 4),
    ("n12_clean", 12, 0.0, 0.2, "general", False, 4),
    ("n200_planar", 200, 0.30, 0.3, "general", True, 4),
    ("n200_xtrans", 200, 0.30, 0.3, "x", False, 4),
    ("n200_forward", 200, 0.30, 0.3, "forward", False, 4),
    ("n200_still_noisy", 200, 0.30, 0.3, "none", False, 4),
    ("n200_still_exact", 200, 0.30, 0.0, "none", False, 4),
]


def family_scenes(name):
    i = [f[0] for f in FAMILIES].index(name)
    _, n, o, noise, motion, planar, count = FAMILIES[i]
    return [scene(1000 * (i + 1) + k, n, o, noise, motion, planar) for k in range(count)]


def identity_matches(n):
    m = np.zeros(n, R.MATCH)
    m["query_idx"] = m["train_idx"] = np.arange(n)
    return m


def _with_outliers(seed, kp0, kp1, share=0.3):
    rng = np.random.default_rng(seed)
    n = kp0.shape[0]
    truth = np.ones(n, bool)
    bad = rng.permutation(n)[:int(round(share * n))]
    truth[bad] = False
    kp1 = kp1.copy()
    kp1[bad] = np.stack([rng.uniform(0, W, bad.size), rng.uniform(0, H, bad.size)], axis=1).astype(np.float32)
    return kp1, truth


def known_cases():
    """(name, matches, kp_prev, kp_cur, truth or None, expectation): expectation is "nothing" (no inliers), "all_at_1" (every match
    an inlier, hypotheses_run 1), "truth_kept" (every true inlier kept) or "same" (whatever the restatement gives)."""
    rng = np.random.default_rng(77)
    cases = []
    m, k0, k1, _ = scene(5, 7, 0.0, 0.2)
    cases.append(("n7", m, k0, k1, None, "nothing"))
    m, k0, k1, _ = scene(6, 8, 0.0, 0.2)
    cases.append(("eight", m, k0, k1, None, "all_at_1"))
    still_f = np.stack([rng.uniform(0, W, 200), rng.uniform(0, H, 200)], axis=1).astype(np.float32)
    still_i = np.stack([rng.integers(0, W, 200), rng.integers(0, H, 200)], axis=1).astype(np.float32)
    cases.append(("still_float", identity_matches(200), still_f, still_f.copy(), None, "all_at_1"))
    cases.append(("still_integer", identity_matches(200), still_i, still_i.copy(), None, "all_at_1"))
    for name, kp in (("still_float_outliers", still_f), ("still_integer_outliers", still_i)):
        k1, truth = _with_outliers(11, kp, kp)
        cases.append((name, identity_matches(200), kp, k1, truth, "truth_kept"))
    shifted = still_i + np.array([2.0, 0.0], np.float32)
    cases.append(("shift2_integer", identity_matches(200), still_i, shifted, None, "all_at_1"))
    k1, truth = _with_outliers(12, still_i, shifted)
    cases.append(("shift2_integer_outliers", identity_matches(200), still_i, k1, truth, "truth_kept"))
    one = np.tile(np.array([[123.25, 77.5]], np.float32), (40, 1))
    cases.append(("one_point", identity_matches(40), one, one.copy(), None, "same"))
    m, k0, k1, truth = scene(9, 200, 0.3, 0.0, "x")
    cases.append(("x_translation_exact", m, k0, k1, truth, "truth_kept"))
    return cases
