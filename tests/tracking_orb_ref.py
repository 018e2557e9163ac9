"""The front end of System::Tracking under RobustMatcher(1) restated on the CPU: steps 1-5 of uwt_tracking_orb_batch (include/uwt.h)
composed from the restatements of its stages — orb_ref, match_ref (Hamming, by the rows' dtype), ransac_ref.  A helper of the tests,
not a test.  Detection and description of a frame are computed once per (image, parameters, cap, pattern) and shared."""
import hashlib

import numpy as np

import match_ref as M
import orb_ref as O
import ransac_ref as R
from tracking_ref import INTR, xy  # noqa: F401  (the intrinsics the tests render with)

_detected = {}


def params_of(orb=None):
    p = O.default_params()
    p.update(orb or {})
    return p


def detect_describe(img, orb=None, cap=2048, pattern=None):
    """orb_ref.detect_describe, remembered per image"""
    p = params_of(orb)
    img = np.ascontiguousarray(img, np.uint8)
    key = (hashlib.sha1(img.tobytes()).hexdigest(), img.shape, tuple(sorted(p.items())), cap,
           None if pattern is None else np.asarray(pattern, np.int8).tobytes())
    if key not in _detected:
        _detected[key] = O.detect_describe(img, p, cap, pattern)
    kp, desc = _detected[key]
    return kp.copy(), desc.copy()


def front_end(prev_img, cur_img, prev_kp=None, ratio=0.65, min_matches=110, cap=2048, orb=None, ransac=None, pattern=None):
    """Steps 1-5 for one pair, as tracking_ref.front_end.  prev_kp: the KEYPOINT records the previous frame kept, or None."""
    p = params_of(orb)
    n_prev = 0 if prev_kp is None else len(prev_kp)
    use = prev_kp is not None and n_prev >= 1 and n_prev >= min_matches
    if use:
        kq, dq = O.describe(np.ascontiguousarray(prev_img, np.uint8), np.asarray(prev_kp, O.KEYPOINT)[:cap], p, pattern)
    else:
        kq, dq = detect_describe(prev_img, orb, cap, pattern)
    kt, dt = detect_describe(cur_img, orb, cap, pattern)
    sym, _, _ = M.match(dq, dt, ratio)
    _, good, rinfo = R.ransac(sym, xy(kq), xy(kt), **(ransac or {}))
    kept_prev, kept_cur = kq[good["query_idx"]], kt[good["train_idx"]]
    info = dict(status=0, used_provided=int(use), n_kp_prev=len(kq), n_kp_cur=len(kt), n_symmetric=len(sym), n_matches=len(good),
                best_hypothesis=int(rinfo["best_hypothesis"]), hypotheses_run=int(rinfo["hypotheses_run"]))
    return dict(used_provided=int(use), kp_prev=kq, desc_prev=dq, kp_cur=kt, desc_cur=dt, sym=sym, good=good, ransac=rinfo,
                kept_prev=kept_prev, kept_cur=kept_cur, info=info)


_walked = {}


def sequence(frames, **kw):
    """The live loop over frames[0], frames[1], ...: pair k is (k, k + 1) and takes what frame k kept as the current frame of
    pair k - 1 (kept_cur -> prev_kp).  Returns one front_end dict per pair; remembered per (frames, settings)."""
    key = (hashlib.sha1(b"".join(np.ascontiguousarray(f, np.uint8).tobytes() for f in frames)).hexdigest(), repr(sorted(kw.items())))
    if key not in _walked:
        out, prev = [], None
        for k in range(len(frames) - 1):
            r = front_end(frames[k], frames[k + 1], prev, **kw)
            out.append(r)
            prev = r["kept_cur"]
        _walked[key] = out
    return _walked[key]
