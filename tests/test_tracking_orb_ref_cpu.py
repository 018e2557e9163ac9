"""The inputs of tests/test_gpu_tracking_orb_batch.py are worth testing, shown without a device: the CPU restatement of the ORB front
end (tests/tracking_orb_ref.py) gives the counts the GPU tests assert — both paths of `usekeypoints` mixed in one walk, key points on
every layer, a size whose upper layers have no band — and the binding's record of the ORB chain has the pinned layout and defaults."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tracking_orb_ref as TO

ARITH_INDEPENDENT = True   # the front end has no arithmetic set


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def counts(r):
    return tuple(r["info"][k] for k in ("n_kp_prev", "n_kp_cur", "n_symmetric", "n_matches"))


@pytest.mark.parametrize("w,h,seed,distance,want,layers", [(256, 240, 31, None, (471, 464, 270, 269), 8), (256, 240, 31, 0.05, (471, 464, 270, 237), 8),
                                                           (160, 96, 5, None, (72, 69, 43, 43), 3), (160, 96, 5, 0.05, (72, 69, 43, 36), 3)])
def test_pair_counts(synth, w, h, seed, distance, want, layers):
    ref, tgt = synth.render_pair(w, h, *TO.INTR[(w, h)], seed=seed)[:2]
    r = TO.front_end(ref, tgt, ransac=dict(distance=distance) if distance else None)
    assert counts(r) == want and r["used_provided"] == 0
    assert np.count_nonzero(np.bincount(r["kept_prev"]["octave"], minlength=8)) == layers


@pytest.mark.parametrize("seed,min_matches,n_matches,used", [(3, 110, [262, 163, 108, 379], [0, 1, 1, 0]), (3, 60, [262, 163, 108, 95], [0, 1, 1, 1]),
                                                             (17, 110, [235, 168, 136, 96], [0, 1, 1, 1])])
def test_sequence_counts_and_paths(synth, seed, min_matches, n_matches, used):
    frames = synth.render_sequence(256, 240, *TO.INTR[(256, 240)], 5, seed=seed)[0]
    walk = TO.sequence(frames, min_matches=min_matches)
    assert [r["info"]["n_matches"] for r in walk] == n_matches
    assert [r["used_provided"] for r in walk] == used
    for r in walk:   # a provided record passes through: every field but the direction is the one the detection before wrote
        assert len(r["kept_prev"]) == len(r["kept_cur"]) == r["info"]["n_matches"]


def test_a_frame_without_a_band_has_no_key_points(synth):
    ref, tgt = synth.render_pair(97, 61, *TO.INTR[(97, 61)], seed=11)[:2]
    r = TO.front_end(ref, tgt)
    assert counts(r) == (0, 0, 0, 0)


def test_params_record(capi):
    assert C.sizeof(capi.TrackingOrbParams) == 56
    p = capi.default_tracking_orb_params()
    assert [getattr(p.orb, k) for k, _ in capi.OrbParams._fields_] == [500, 8, 31, 20, 0]
    d = capi.default_ransac_params()
    assert [getattr(p.ransac, k) for k, _ in capi.RansacParams._fields_] == [getattr(d, k) for k, _ in capi.RansacParams._fields_]
    assert (p.ransac.distance, p.ransac.confidence, p.ransac.max_hypotheses, p.ransac.seed) == (3.0, 0.99, 1000, 0)
    assert p.ratio == np.float32(0.65) and p.min_matches == 110
    q = capi.default_tracking_orb_params(orb=dict(n_features=300), ransac=dict(distance=0.05), min_matches=60)
    assert (q.orb.n_features, q.orb.n_levels, q.ransac.distance, q.min_matches) == (300, 8, 0.05, 60)
    with pytest.raises(AttributeError):
        capi.default_tracking_orb_params(orb=dict(hessian_threshold=1.0))
    assert {"uwt_default_tracking_orb_params", "uwt_tracking_orb_batch_async", "uwt_tracking_orb_batch"} <= set(capi.SYMBOLS)
