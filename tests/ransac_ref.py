"""The RANSAC inlier selection of include/uwt.h (uwt_ransac_inliers_batch) restated in numpy, independently of the library:
float64 throughout, every expression in the order the contract writes it, one IEEE operation per numpy operation (numpy fuses
nothing), so that the device's outputs can be compared as integers.  Hypotheses are evaluated in groups, which changes no bit:
the selection over their counts is the contract's sequential loop."""
import math

import numpy as np

MATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
INFO = np.dtype([("status", "<i4"), ("n_inliers", "<i4"), ("best_hypothesis", "<i4"), ("hypotheses_run", "<i4"), ("F", "<f8", (9,))])
M32 = 0xFFFFFFFF


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample(seed, h, n):
    """the eight match indices of hypothesis h"""
    taken = []
    out = []
    for s in range(8):
        u = mix(seed ^ mix(8 * h + s))
        j = (u * (n - s)) >> 32
        for e in sorted(taken):
            if j >= e:
                j += 1
        taken.append(j)
        out.append(j)
    return out


def iterations(confidence, n, k, H):
    """need(k): uwt_ransac_iterations"""
    if confidence == 1 or k <= 0 or n <= 0:
        return H
    w = k / n
    w2 = w * w
    w4 = w2 * w2
    w8 = w4 * w4
    num = math.log(1 - confidence)
    den = math.log(1 - w8) if w8 < 1 else -math.inf
    if den >= 0 or -num >= H * (-den):
        return H
    return int(np.rint(num / den))


def hypotheses(pts, seed, hs):
    """F [len(hs), 9] and validity of the hypotheses hs; pts: [N, 4] float64 (x, y, x', y')"""
    n = pts.shape[0]
    idx = np.array([sample(seed, h, n) for h in hs], np.int64)          # [G, 8]
    x, y, xp, yp = (pts[idx, k] for k in range(4))                        # [G, 8]
    M = np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones_like(x)], axis=2)   # [G, 8, 9]
    G = len(hs)
    g_all = np.arange(G)
    rused = np.zeros((G, 8), bool)
    cused = np.zeros((G, 9), bool)
    row_of_col = np.full((G, 9), -1, np.int64)
    live = np.ones(G, bool)        # still eliminating
    valid = np.ones(G, bool)
    with np.errstate(all="ignore"):
        for _ in range(8):
            A = np.abs(M)
            A = np.where(np.isnan(A), -1.0, A)
            A = np.where(rused[:, :, None] | cused[:, None, :], -1.0, A).reshape(G, 72)
            arg = np.argmax(A, axis=1)         # the first of the largest: lowest row, then lowest column
            best = A[g_all, arg]
            live &= best > 0.0                 # nothing took over: ends early
            inf = live & np.isinf(best)
            valid &= ~inf
            live &= ~inf
            if not live.any():
                break
            br, bc = arg // 9, arg % 9
            piv = M[g_all, br, bc]
            row = M[g_all, br, :] / piv[:, None]                 # [G, 9]
            g = M[g_all[:, None], np.arange(8)[None, :], bc[:, None]]   # [G, 8], read before any row changes
            new = M - g[:, :, None] * row[:, None, :]
            new[g_all, br, :] = row
            M = np.where(live[:, None, None], new, M)
            rused[g_all[live], br[live]] = True
            cused[g_all[live], bc[live]] = True
            row_of_col[g_all[live], bc[live]] = br[live]
    cs = np.argmin(cused, axis=1)          # lowest unused column
    F = np.zeros((G, 9))
    for c in range(9):
        r = row_of_col[:, c]
        piv_val = -M[g_all, np.maximum(r, 0), cs]
        F[:, c] = np.where(cs == c, 1.0, np.where(cused[:, c], piv_val, 0.0))
    F[~valid] = 0.0
    return F, valid


def inliers(F, pts, distance):
    """[G, N] bool: the matches each F [G, 9] keeps"""
    x, y, xp, yp = (pts[None, :, k] for k in range(4))
    f = [F[:, k, None] for k in range(9)]
    t2 = distance * distance
    with np.errstate(all="ignore"):
        a = f[0] * x + f[1] * y + f[2]
        b = f[3] * x + f[4] * y + f[5]
        c = f[6] * x + f[7] * y + f[8]
        s2 = xp * a + yp * b + c
        d2 = s2 * s2 / (a * a + b * b)
        a1 = f[0] * xp + f[3] * yp + f[6]
        b1 = f[1] * xp + f[4] * yp + f[7]
        c1 = f[2] * xp + f[5] * yp + f[8]
        s1 = x * a1 + y * b1 + c1
        d1 = s1 * s1 / (a1 * a1 + b1 * b1)
        return (d1 <= t2) & (d2 <= t2)


def ransac(matches, kp_prev, kp_cur, distance=3.0, confidence=0.99, max_hypotheses=1000, seed=0, group=64):
    """(mask uint8 [N], good matches, info record) of one pair"""
    matches = np.asarray(matches, MATCH)
    n = len(matches)
    info = np.zeros((), INFO)
    info["best_hypothesis"] = -1
    mask = np.zeros(n, np.uint8)
    if n < 8:
        return mask, matches[:0].copy(), info
    kp_prev = np.asarray(kp_prev, np.float32).reshape(-1, 2)
    kp_cur = np.asarray(kp_cur, np.float32).reshape(-1, 2)
    pts = np.concatenate([kp_prev[matches["query_idx"]], kp_cur[matches["train_idx"]]], axis=1).astype(np.float64)
    H = max_hypotheses
    best, best_h, limit, h = 0, -1, H, 0
    best_F = np.zeros(9)
    while h < limit:
        hs = list(range(h, min(h + group, limit)))
        F, valid = hypotheses(pts, seed, hs)
        counts = np.where(valid, inliers(F, pts, distance).sum(axis=1), 0)
        for k, hh in enumerate(hs):
            h = hh
            if not h < limit:
                break
            if counts[k] > max(best, 7):
                best, best_h, best_F = int(counts[k]), h, F[k].copy()
                limit = min(limit, iterations(confidence, n, best, H))
            h = hh + 1
    info["hypotheses_run"] = h
    if best_h >= 0:
        mask = inliers(best_F[None], pts, distance)[0].astype(np.uint8)
        info["n_inliers"] = int(mask.sum())
        info["best_hypothesis"] = best_h
        info["F"] = best_F
    return mask, matches[mask.astype(bool)].copy(), info
