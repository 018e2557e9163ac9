"""The CPU restatement of the front end of System::Tracking (tests/tracking_ref.py) on the inputs of tests/test_gpu_tracking_batch.py:
what those tests rely on — which pairs take the provided path, how many matches survive, where RANSAC has to iterate — is pinned
here without a GPU, together with the layout of the records the call exchanges."""
import ctypes as C
import importlib

import numpy as np
import pytest

import surf_cases as K
import surf_ref as S
import tracking_ref as TR

ARITH_INDEPENDENT = True   # the front end has no arithmetic set
W, H = 256, 240


@pytest.fixture(scope="module")
def pair31(synth):
    ref, tgt, _, _, _ = synth.render_pair(W, H, *TR.INTR[(W, H)], seed=31)
    return ref, tgt


def seq(synth, seed):
    return synth.render_sequence(W, H, *TR.INTR[(W, H)], 5, seed=seed)[0]


def test_struct_sizes_match_the_header():
    capi = importlib.import_module("uw-slam_amd.capi")
    assert C.sizeof(capi.TrackingParams) == 56
    assert capi.TRACKING_INFO.itemsize == 32
    assert C.sizeof(capi.TrackingIO) == 9 * C.sizeof(C.c_void_p)
    assert capi.STATS.itemsize == C.sizeof(capi.Stats) == 16
    for name in ("uwt_default_tracking_params", "uwt_tracking_batch_async", "uwt_tracking_batch", "uwt_match_descriptors_device_async"):
        assert name in capi.SYMBOLS


@pytest.mark.parametrize("distance,inliers,run,best", [(None, 174, 1, 0), (0.05, 144, 23, 22), (0.02, 98, 453, None)])
def test_seed31_pair(pair31, distance, inliers, run, best):
    r = TR.front_end(*pair31, ransac=dict(distance=distance) if distance else None)
    i = r["info"]
    assert (i["n_kp_prev"], i["n_kp_cur"], i["n_symmetric"], i["used_provided"]) == (239, 229, 174, 0)
    assert (i["n_matches"], i["hypotheses_run"]) == (inliers, run)
    if best is not None:
        assert i["best_hypothesis"] == best
    if distance == 0.02:
        assert i["n_matches"] < 110   # the next pair of a loop would detect again


def test_seed3_sequence_takes_the_provided_path(synth):
    rs = TR.sequence(seq(synth, 3), min_matches=110)
    assert [r["info"]["used_provided"] for r in rs] == [0, 1, 1, 1]
    assert [r["info"]["n_matches"] for r in rs] == [149, 131, 120, 119]
    assert [r["info"]["n_kp_prev"] for r in rs[1:]] == [149, 131, 120]


def test_seed17_sequence_mixes_the_paths(synth):
    fr = seq(synth, 17)
    rs = TR.sequence(fr, min_matches=90)
    assert [r["info"]["used_provided"] for r in rs] == [0, 1, 0, 0]
    assert [r["info"]["n_matches"] for r in rs] == [92, 83, 89, 86]
    assert rs[1]["info"]["n_kp_prev"] == 92
    assert [r["info"]["used_provided"] for r in TR.sequence(fr, min_matches=110)] == [0, 0, 0, 0]


@pytest.mark.parametrize("w,h,seed,kps,inliers", [(160, 96, 5, (59, 59), 49), (97, 61, 11, (19, 18), 14)])
def test_small_sizes(synth, w, h, seed, kps, inliers):
    a, b, _, _, _ = synth.render_pair(w, h, *TR.INTR[(w, h)], seed=seed)
    i = TR.front_end(a, b)["info"]
    assert (i["n_kp_prev"], i["n_kp_cur"]) == kps and i["n_matches"] == inliers


def test_flat_frames_have_no_match(pair31):
    for a, b in ((pair31[0], K.flat(W, H)), (K.flat(W, H), pair31[1])):
        i = TR.front_end(a, b)["info"]
        assert min(i["n_kp_prev"], i["n_kp_cur"]) == 0
        assert (i["n_symmetric"], i["n_matches"], i["hypotheses_run"], i["best_hypothesis"]) == (0, 0, 0, -1)


def test_describing_the_kept_records_gives_the_kept_rows(synth, pair31):
    """the hand-over rests on it: a frame described at the records it kept as a current frame has, bit for bit, the rows its
    detection had there"""
    cases = [(pair31[1], TR.front_end(*pair31))]
    for seed in (3, 17):
        fr = seq(synth, seed)
        cases.append((fr[1], TR.front_end(fr[0], fr[1])))
    for img, r in cases:
        kq, dq = S.describe(img, r["kept_cur"])
        assert len(kq) >= 8
        assert K.same_keypoints(kq, r["kept_cur"]) is None
        assert K.same_descriptors(dq, r["desc_cur"][r["good"]["train_idx"]]) is None
