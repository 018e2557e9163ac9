"""The front end of System::Tracking restated on the CPU: steps 1-5 of uwt_tracking_batch (include/uwt.h) composed from the
restatements of its stages — surf_ref, match_ref, ransac_ref.  A helper of the tests, not a test.  Detection and description of a
frame are computed once per (image, parameters, cap) and shared: they are by far the slowest part."""
import hashlib

import numpy as np

import match_ref as M
import ransac_ref as R
import surf_ref as S

INTR = {(160, 96): (131.25, 131.25, 79.5, 47.5), (97, 61): (80.0, 80.0, 48.0, 30.0), (256, 240): (210.0, 210.0, 127.5, 119.5),
        (640, 480): (525.0, 525.0, 319.5, 239.5), (735, 479): (458.654, 457.296, 367.0, 239.0)}
DEFAULTS = dict(ratio=0.65, min_matches=110, cap=2048, surf=None, ransac=None)

_detected = {}


def detect_describe(img, surf=None, cap=2048):
    """surf_ref.detect_describe, remembered per image"""
    p = S.default_params()
    p.update(surf or {})
    img = np.ascontiguousarray(img, np.uint8)
    key = (hashlib.sha1(img.tobytes()).hexdigest(), img.shape, tuple(sorted(p.items())), cap)
    if key not in _detected:
        _detected[key] = S.detect_describe(img, p, cap)
    kp, desc = _detected[key]
    return kp.copy(), desc.copy()


def xy(kp):
    return np.stack([kp["x"], kp["y"]], 1).astype(np.float32).reshape(-1, 2)


def front_end(prev_img, cur_img, prev_kp=None, ratio=0.65, min_matches=110, cap=2048, surf=None, ransac=None):
    """Steps 1-5 for one pair.  prev_kp: the KEYPOINT records the previous frame kept, or None.  Returns a dict: used_provided, the
    query and train sets (kp_prev, desc_prev, kp_cur, desc_cur), sym, good, ransac (the info record), kept_prev, kept_cur and info,
    the fields of uwt_tracking_info."""
    p = S.default_params()
    p.update(surf or {})
    n_prev = 0 if prev_kp is None else len(prev_kp)
    use = prev_kp is not None and n_prev >= 1 and n_prev >= min_matches
    if use:
        kq, dq = S.describe(prev_img, np.asarray(prev_kp, S.KEYPOINT)[:cap], p)
    else:
        kq, dq = detect_describe(prev_img, surf, cap)
    kt, dt = detect_describe(cur_img, surf, cap)
    sym, _, _ = M.match(dq, dt, ratio)
    _, good, rinfo = R.ransac(sym, xy(kq), xy(kt), **(ransac or {}))
    kept_prev, kept_cur = kq[good["query_idx"]], kt[good["train_idx"]]
    info = dict(status=0, used_provided=int(use), n_kp_prev=len(kq), n_kp_cur=len(kt), n_symmetric=len(sym), n_matches=len(good),
                best_hypothesis=int(rinfo["best_hypothesis"]), hypotheses_run=int(rinfo["hypotheses_run"]))
    return dict(used_provided=int(use), kp_prev=kq, desc_prev=dq, kp_cur=kt, desc_cur=dt, sym=sym, good=good, ransac=rinfo,
                kept_prev=kept_prev, kept_cur=kept_cur, info=info)


def sequence(frames, **kw):
    """The live loop over frames[0], frames[1], ...: pair k is (k, k + 1) and takes what frame k kept as the current frame of
    pair k - 1 (kept_cur -> prev_kp).  Returns one front_end dict per pair."""
    out, prev = [], None
    for k in range(len(frames) - 1):
        r = front_end(frames[k], frames[k + 1], prev, **kw)
        out.append(r)
        prev = r["kept_cur"]
    return out
