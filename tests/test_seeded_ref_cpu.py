"""The specification the seeded GPU tests are measured against (tests/seeded_ref.py, tests/seeded_cases.py), pinned on the CPU:
the written-out loop is the oracle's own where both exist, the cases tell a seeded call from an unseeded one and the two hand-offs
apart, the motion model's restatement agrees with plain matrix arithmetic, and the ABI carries the new symbols."""
import ctypes
import importlib
import itertools
import os
import re

import numpy as np
import pytest

import seeded_cases as SC
import seeded_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (96, 64, (78.0, 78.0, 47.5, 31.5))
NEW_SYMBOLS = ("uwt_default_seed_options", "uwt_estimate_pose_batch_seeded", "uwt_track_batch_seeded_async",
               "uwt_track_features_batch_seeded_async", "uwt_estimate_pose_features_batch_seeded",
               "uwt_track_candidates_batch_seeded_async", "uwt_estimate_pose_candidates_batch_seeded",
               "uwt_tracking_batch_seeded_async", "uwt_tracking_orb_batch_seeded_async", "uwt_predict_seeds_device_async",
               "uwt_tracking_batch_seeded", "uwt_tracking_orb_batch_seeded", "uwt_predict_seeds")
EARLY = dict(max_iters=50, early_exit=1)


def same_run(a, b):
    """status, pose, and every trace row's n_valid, error and pose, bit for bit"""
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[2]) == len(b[2]) and all(
        x["n_valid"] == y["n_valid"] and np.float32(x["error"]).tobytes() == np.float32(y["error"]).tobytes() and
        np.array_equal(x["pose"], y["pose"]) for x, y in zip(a[2], b[2]))


# ---- 1. the identity start under the reference's hand-off is the oracle's own loop ---------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["none", "depth"])
@pytest.mark.parametrize("early_exit", [0, 1])
def test_identity_start_equals_the_oracle(O, synth, arith, early_exit, depth):
    """96 x 64 x 3 levels: weights 0 / 1 / 2 x sampler 0 / 1 (Tukey over the bilinear sampler included: the oracle has it), dense and
    over candidate tables"""
    w, h, intr = SIZE
    ref, tgt, dep = synth.render_pair(w, h, *intr, seed=9100, with_depth=True, max_t=0.015, max_deg=0.8)[:3]
    for weights, sampler in itertools.product((0, 1, 2), (0, 1)):
        p = O.default_params(w, h, *intr, n_levels=3, first_level=2, last_level=0, has_depth=int(depth), weights=weights, sampler=sampler,
                             early_exit=early_exit, max_iters=50 if early_exit else 4)
        d = dep if depth else None
        assert same_run(SR.align(O, p, ref, tgt, d), O.align_pair(p, ref, tgt, d, want_trace=True)), (weights, sampler)
        imgs = O.pyramid(ref, 3)
        deps = O.pyramid(dep, 3) if depth else None
        tables = {}
        for l in range(3):
            L = O.level_intrinsics(p, l)
            tables[l] = O.candidate_points(O.gradient_mag(*O.scharr3(imgs[l])), deps[l] if depth else None, 20.0, grid=(L.w, L.h))[0]
        assert same_run(SR.align(O, p, ref, tgt, d, tables=tables), O.align_pair_points(p, ref, tgt, tables, ref_depth=d, want_trace=True)), \
            ("tables", weights, sampler)


def test_empty_table_and_bad_seed(O, synth):
    w, h, intr = SIZE
    ref, tgt, dep = synth.render_pair(w, h, *intr, seed=9100, with_depth=True)[:3]
    p = O.default_params(w, h, *intr, n_levels=3, first_level=0, last_level=0)
    seed = SC.seeds(O, 1)[0]
    st, pose, tr = SR.align(O, p, ref, tgt, None, seed=seed, tables={0: np.zeros((0, 4), np.float32)})
    assert st == SR.ERR_NO_VALID_POINTS and pose.tobytes() == seed.tobytes() and tr == []   # the seed stands where the identity stood
    for bad in SC.bad_seeds():
        st, pose, tr = SR.align(O, p, ref, tgt, None, seed=bad)
        assert st == SR.ERR_INVALID_ARG and pose.tobytes() == SR.IDENTITY.tobytes() and tr == []
        assert not np.isfinite(bad).all() and np.isfinite(bad).sum() == 6


# ---- 2. the cases discriminate ------------------------------------------------------------------------------------------------------
def test_cases_discriminate(O, synth, arith):
    seeds = SC.seeds(O)
    assert seeds.shape == (SC.N_SEEDS, 7) and np.isfinite(seeds).all()
    heavy, leave = False, {}
    for k in range(SC.N_SEEDS):
        scene = k % SC.N_SCENES
        for over in (EARLY, dict(max_iters=4, early_exit=0)):
            unseeded = SC.expect(O, synth, arith, scene, None, False, **over)
            ref = SC.expect(O, synth, arith, scene, seeds[k], False, **over)
            keep = SC.expect(O, synth, arith, scene, seeds[k], True, **over)
            assert unseeded[0] == ref[0] == keep[0] == 0, (k, over)                      # every good seed ends with status 0
            assert ref[1].tobytes() != unseeded[1].tobytes(), (k, over)                  # the seed shows in the result
            assert keep[1].tobytes() != ref[1].tobytes(), (k, over)                      # and so does the hand-off
        ev = SR.level_evaluations(SC.expect(O, synth, arith, scene, seeds[k], False, **EARLY)[2])
        leave[k] = ev
        heavy = heavy or max(ev.values()) > 4
    print("evaluations per level", leave)
    assert heavy                                              # a level needs more than first_poll + 1 = 4 evaluations
    assert SR.level_evaluations(SC.expect(O, synth, arith, 1, seeds[1], False, **EARLY)[2])[0] > 4   # pair 1, level 0: the rerun's case
    assert SR.level_evaluations(SC.expect(O, synth, arith, 5, seeds[11], True, **EARLY)[2])[0] > 4    # pair 11 under keep: the same
    assert any(leave[a][l] != leave[b][l] for a in range(5) for b in range(5) for l in (0, 1, 2))   # two pairs of a batch leave a level apart
    # the odd size
    for k in range(3):
        assert SC.expect(O, synth, arith, k, seeds[k], False, size=SC.ODD, **EARLY)[0] == 0


# ---- 3. the motion model ---------------------------------------------------------------------------------------------------------------
def matrix(pose):
    x, y, z, w = np.asarray(pose[:4], np.float64)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = pose[4:]
    return T


@pytest.mark.one_arith
def test_predict_seeds_agrees_with_matrices(O):
    """to 1e-5 absolute on poses with |t| <= 1: a sanity bound, about 100 x the f32 epsilon over a handful of operations on values
    <= 1; the bit-level contract is the restatement itself"""
    rng = np.random.default_rng(11)
    n = 200
    tw = rng.uniform(-1, 1, (2 * n, 6)) * [0.5, 0.5, 0.5, 0.8, 0.8, 0.8]
    poses = np.stack([O.se3_exp(t.astype(np.float32)) for t in tw])
    assert np.abs(poses[:, 4:]).max() <= 1.0
    prev, cur = poses[:n], poses[n:]
    got = SR.predict_seeds(O, prev, cur)
    for i in range(n):
        want = matrix(cur[i]) @ np.linalg.inv(matrix(prev[i])) @ matrix(cur[i])
        assert np.abs(matrix(got[i]) - want).max() <= 1e-5, i
    assert np.array_equal(SR.predict_seeds(O, prev[:3], prev[:3]), np.stack([O.se3_mul(O.se3_mul(p, SR.se3_inverse(p)), p) for p in prev[:3]]))
    bad = cur.copy()
    bad[5, 0] = np.nan
    out = SR.predict_seeds(O, prev, bad)
    assert np.isnan(out[5]).all() and np.array_equal(np.delete(out, 5, 0), np.delete(got, 5, 0))
    assert out[5].view(np.uint32).tolist() == [0x7fc00000] * 7


# ---- 4. the ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.one_arith
def test_abi_carries_the_seeded_symbols():
    importlib.import_module("uw-slam_amd").build_native()
    capi = importlib.import_module("uw-slam_amd.capi")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uwt_[a-z0-9_]+)\s*\(", src))
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    assert ctypes.sizeof(capi.SeedOptions) == 32
    assert re.search(r"#define UWT_ABI_VERSION 4\b", src) and lib.uwt_abi_version() == 4
    o = capi.SeedOptions(handoff=1)
    o.reserved[3] = 9
    assert lib.uwt_default_seed_options(ctypes.byref(o)) == 0 and bytes(o) == bytes(32)
    assert lib.uwt_default_seed_options(None) == 1
    # the mirrors carry them too
    T = importlib.import_module("uw-slam_amd.tracker")
    assert all(hasattr(T.Tracker, m) for m in ("EstimatePoseSeeded", "PredictSeeds"))
    hpp = open(os.path.join(ROOT, "include", "uw_tracker.hpp")).read()
    assert all(m in hpp for m in ("EstimatePoseSeeded", "PredictSeeds", "uwt_estimate_pose_features_batch_seeded",
                                  "uwt_estimate_pose_candidates_batch_seeded", "uwt_tracking_batch_seeded"))
