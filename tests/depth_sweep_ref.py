"""numpy restatement of the depth sweep (EXTENSION; the contract is the section "depth from tracked motion" of include/uwt.h): the
hypotheses' rows are made like oracle.dense_points makes a depth plane's and warped by oracle.warp (uwt_warp's arithmetic in the
active arithmetic set); everything behind the landing is integers, and the refinement six f64 operations.  Test infrastructure: the
library computes none of this here.

`variant` names one deliberately WRONG reading of the contract (tests/test_depth_sweep_cpu.py shows that the designed inputs tell
each of them from the contract): "tie_largest", "uniq_le", "index_distance", "parallax_view0", "truncate"."""
import numpy as np

LIMIT = 2147483520.0   # 2^31 - 128 (the image warp's rule)
OK, INVALID_ARG = 0, 1
NOT_SELECTED, ESTIMATED, BORDER, FEW, LOW_PARALLAX, EDGE, POOR, AMBIGUOUS = range(8)
INFO_FIELDS = ("status", "n_selected", "n_outcome", "sum_cost", "sum_code", "reserved")
VARIANTS = ("tie_largest", "uniq_le", "index_distance", "parallax_view0", "truncate")
DEFAULTS = dict(lvl=0, source=1, threshold=20.0, radius=2, max_mean_abs=12, uniq_num=3, uniq_den=4, min_parallax=4, refine=1)


def hypotheses(z_near, z_far, depth_scale, n):
    """uwt_sweep_hypotheses' formula in f64; None where the call refuses"""
    r0 = 1.0 / np.float64(z_near)
    step = (1.0 / np.float64(z_far) - r0) / np.float64(n - 1)
    rho = r0 + np.arange(n, dtype=np.float64) * step
    d = np.rint(1.0 / (rho * np.float64(depth_scale)))
    if not (np.all(d >= 1) and np.all(d <= 32767) and np.all(np.diff(d) > 0)):
        return None
    return d.astype(np.uint16)


def code_z(codes, lvl, depth_scale):
    """z(d) = (float)d * (float)((double)depth_scale / 2^lvl), as ObtainAllPoints computes it (oracle.dense_points)"""
    factor = np.float32(np.float64(np.float32(depth_scale)) / 2.0 ** lvl)
    return np.asarray(codes, np.uint16).astype(np.float32) * factor


def candidate_mask(O, ref_img, w, h, threshold):
    """the pixels of uwt_obtain_candidate_points' rows on a context without a depth plane: gradient_ > mean + threshold over the grid"""
    mag = O.gradient_mag(*O.scharr3(ref_img))
    thres = float(mag.astype(np.int64).sum()) / float(mag.size) + float(threshold)
    sel = np.zeros(ref_img.shape, bool)
    sel[:h, :w] = mag[:h, :w].astype(np.float64) > thres
    return sel


def c_round(u):
    """(int)round(u) of C, vectorised over float32 values held in f64 (exact); the caller masks what does not land"""
    return (np.sign(u) * np.floor(np.abs(u) + 0.5)).astype(np.int64)


def sweep(O, p, ref_img, view_imgs, poses, codes, variant=None, **kw):
    """One job.  p: oracle Params (intrinsics, depth_scale); ref_img / view_imgs: the level's u8 images; poses [n_views, 7].
    Returns dict(depth u16, cost u16, outcome u8 — img_h x img_w — info dict, diag dict)."""
    assert variant is None or variant in VARIANTS
    q = dict(DEFAULTS)
    q.update(kw)
    lvl, r = q["lvl"], q["radius"]
    L = O.level_intrinsics(p, lvl)
    ih, iw = ref_img.shape
    assert (L.iw, L.ih) == (iw, ih)
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    V, K = poses.shape[0], len(codes)
    assert len(view_imgs) == V and 1 <= V <= 4 and 3 <= K <= 64 and r in (1, 2)
    depth = np.zeros((ih, iw), np.uint16)
    cost_out = np.zeros((ih, iw), np.uint16)
    outcome = np.zeros((ih, iw), np.uint8)
    info = dict(status=OK, n_selected=0, n_outcome=[0] * 8, sum_cost=0, sum_code=0, reserved=0)
    diag = dict(landing_x=set(), z_nonpositive=False, view_disagree=False, tie_same_pixel=0, den_zero=0, cm_eq_cp=0, rint_ne_trunc=0,
                uniq_equal=0)
    if not np.isfinite(poses).all():
        info["status"] = INVALID_ARG
        return dict(depth=depth, cost=cost_out, outcome=outcome, info=info, diag=diag)

    sel = np.zeros((ih, iw), bool)
    sel[:L.h, :L.w] = True
    if q["source"] == 1:
        sel = candidate_mask(O, ref_img, L.w, L.h, q["threshold"])
    ys, xs = np.nonzero(sel)
    inside = (xs >= r) & (xs <= iw - 1 - r) & (ys >= r) & (ys <= ih - 1 - r)
    outcome[ys[~inside], xs[~inside]] = BORDER
    ys, xs = ys[inside], xs[inside]
    N = ys.size
    res = np.full(N, -1, np.int64)

    # landing
    z = code_z(codes, lvl, p.depth_scale)
    pts = np.empty((N, K, 4), np.float32)
    pts[:, :, 0] = xs[:, None]
    pts[:, :, 1] = ys[:, None]
    pts[:, :, 2] = z[None, :]
    pts[:, :, 3] = 1.0
    x2 = np.zeros((V, N, K), np.int64)
    y2 = np.zeros((V, N, K), np.int64)
    lands = np.zeros((V, N, K), bool)
    for v in range(V):
        wp = O.warp(pts.reshape(-1, 4), poses[v], L).reshape(N, K, 4).astype(np.float64)
        u, vv, zp = wp[:, :, 0], wp[:, :, 1], wp[:, :, 2]
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(u) & np.isfinite(vv) & (np.abs(u) < LIMIT) & (np.abs(vv) < LIMIT)
            xr, yr = c_round(np.where(fin, u, 0)), c_round(np.where(fin, vv, 0))
            ok = fin & (zp > 0) & (xr >= r) & (xr <= iw - 1 - r) & (yr >= r) & (yr <= ih - 1 - r)
            diag["z_nonpositive"] |= bool((fin & ~(zp > 0)).any())
        diag["landing_x"] |= set(np.unique(xr[fin & (zp > 0) & (yr >= r) & (yr <= ih - 1 - r)]).tolist()) & {r - 1, r, iw - 1 - r, iw - r}
        x2[v], y2[v], lands[v] = np.where(ok, xr, r), np.where(ok, yr, r), ok
    valid = lands.all(axis=0)
    diag["view_disagree"] = bool((lands.any(axis=0) & ~valid).any())

    # cost (invalid hypotheses gather at (r, r) and are masked)
    ref_i = ref_img.astype(np.int64)
    cost = np.zeros((N, K), np.int64)
    for v in range(V):
        img = view_imgs[v].astype(np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                cost += np.abs(img[y2[v] + dy, x2[v] + dx] - ref_i[ys + dy, xs + dx][:, None])
    BIG = np.int64(1) << 40
    nvalid = valid.sum(axis=1)
    res[nvalid < 3] = FEW
    live = res < 0
    first = np.argmax(valid, axis=1)
    last = K - 1 - np.argmax(valid[:, ::-1], axis=1)
    rows = np.arange(N)

    def dist_to(k):   # [N, K]: dist(j, k[n]) over the views
        d = np.zeros((N, K), np.int64)
        for v in range(V):
            d = np.maximum(d, np.abs(x2[v] - x2[v][rows, k][:, None]))
            d = np.maximum(d, np.abs(y2[v] - y2[v][rows, k][:, None]))
        return d

    par = np.zeros(N, np.int64)
    for v in range(1 if variant == "parallax_view0" else V):
        par = np.maximum(par, np.abs(x2[v][rows, first] - x2[v][rows, last]))
        par = np.maximum(par, np.abs(y2[v][rows, first] - y2[v][rows, last]))
    res[live & (par < q["min_parallax"])] = LOW_PARALLAX
    live = res < 0

    ks = np.arange(K, dtype=np.int64)
    tiebreak = (63 - ks) if variant == "tie_largest" else ks
    key = np.where(valid, cost * 64 + tiebreak[None, :], BIG)
    kw_ = np.argmin(key, axis=1)
    cw = cost[rows, kw_]
    km, kp = np.clip(kw_ - 1, 0, K - 1), np.clip(kw_ + 1, 0, K - 1)
    edge = (kw_ == 0) | (kw_ == K - 1) | ~valid[rows, km] | ~valid[rows, kp]
    res[live & edge] = EDGE
    live = res < 0
    res[live & (cw > q["max_mean_abs"] * (2 * r + 1) ** 2 * V)] = POOR
    live = res < 0

    d_w = dist_to(kw_)
    if variant == "index_distance":
        d_w = np.abs(ks[None, :] - kw_[:, None])
    comp = valid & (d_w >= 2)
    c2 = np.where(comp, cost, BIG).min(axis=1)
    lhs, rhs = q["uniq_den"] * cw, q["uniq_num"] * c2
    unique = comp.any(axis=1) & ((lhs <= rhs) if variant == "uniq_le" else (lhs < rhs))
    diag["uniq_equal"] = int((live & comp.any(axis=1) & (lhs == rhs)).sum())
    res[live & ~unique] = AMBIGUOUS
    est = res < 0
    res[est] = ESTIMATED
    # a cost tie at the winner between hypotheses that land on the same pixel in every view
    same = valid & (d_w == 0) & (cost == cw[:, None])
    diag["tie_same_pixel"] = int((est & (same.sum(axis=1) >= 2)).sum())

    # the estimate
    codes64 = np.asarray(codes, np.uint16).astype(np.float64)
    code = np.asarray(codes, np.uint16).astype(np.int64)[kw_]
    cm, cp = cost[rows, km], cost[rows, kp]
    den = cm - 2 * cw + cp
    diag["den_zero"] = int((est & (den == 0)).sum())
    diag["cm_eq_cp"] = int((est & (cm == cp)).sum())
    if q["refine"]:
        go = est & (den != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.abs(cm - cp).astype(np.float64) / (2 * den).astype(np.float64)
            n = np.where(cm > cp, kp, km)
            rho_k, rho_n = 1.0 / codes64[kw_], 1.0 / codes64[n]
            rho = rho_n - rho_k
            rho = a * rho
            rho = rho_k + rho
            inv = 1.0 / rho
            e = np.trunc(inv) if variant == "truncate" else np.rint(inv)
        diag["rint_ne_trunc"] = int((go & (np.rint(inv) != np.trunc(inv))).sum())
        refined = np.clip(np.where(go, e, 1), 1, 32767).astype(np.int64)
        code = np.where(go, refined, code)

    outcome[ys, xs] = res.astype(np.uint8)
    depth[ys[est], xs[est]] = code[est].astype(np.uint16)
    cost_out[ys[est], xs[est]] = cw[est].astype(np.uint16)
    counts = np.bincount(outcome.reshape(-1), minlength=8).astype(np.int64)
    counts[0] = 0
    info.update(n_selected=int(counts.sum()), n_outcome=[int(c) for c in counts], sum_cost=int(cw[est].sum()), sum_code=int(code[est].sum()))
    diag["winner_x2"] = np.where(est, x2[0][rows, kw_], -1), np.where(est, y2[0][rows, kw_], -1), xs, ys
    return dict(depth=depth, cost=cost_out, outcome=outcome, info=info, diag=diag)


def info_tuple(info):
    """a uwt_sweep_info record (numpy SWEEP_INFO row or the dict above) as a flat tuple of ints"""
    return (int(info["status"]), int(info["n_selected"])) + tuple(int(c) for c in info["n_outcome"]) + (
        int(info["sum_cost"]), int(info["sum_code"]), int(info["reserved"]))
