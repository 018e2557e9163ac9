"""The typed forms of k_residual read a pixel's rays — pixel_ray of its column and of its row — from tables their block fills in LDS
and walk byte offsets into them instead of float coordinates (residual_core, fill_ray_tables).  The plain forms (uwt_tuning::typed_loads
= 0) keep the float walk and compute the rays per pixel.  Same floats, same pixels in the same order: every case compares poses and
stats bit for bit three ways — the default against the same context under typed_loads = 0, both against the oracle, and each pair of a
3-pair batch against the same pair alone.  Tuning chained = 0, coarse_batch_px = 0 throughout: every level runs k_residual.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DISTINCT = 3


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def _bits(poses, stats, i):
    s = stats[i]
    return (poses[i].view(np.uint32).tobytes(), int(s["status"]), int(s["iterations"]), int(s["n_valid"]),
            np.float32(s["error"]).view(np.uint32).item())


def _three_ways(capi, O, synth, w, h, intr, nl, depth, slices_per_pair=0, seed=7300):
    """slices_per_pair: target_blocks follows the number of pairs of a call so that a level is cut into (at most) that many blocks per
    pair whatever the call's size — blocks of several steps, the same slicing alone and in the batch; 0 = the default slicing."""
    over = dict(n_levels=nl, first_level=nl - 1, last_level=0, max_iters=4, early_exit=0, has_depth=1 if depth else 0)
    pairs = []
    for s in range(DISTINCT):
        ref, tgt, dep, _, _ = synth.render_pair(w, h, *intr, seed=seed + w + s, with_depth=depth, max_t=0.012, max_deg=0.6)
        pairs.append((ref, tgt, dep if depth else None))
    po = O.default_params(w, h, *intr, **over)
    want = [O.align_pair(po, r, t, d, want_trace=True) for r, t, d in pairs]
    assert all(st == 0 for st, _, _ in want)
    ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=2 * DISTINCT, max_pairs=DISTINCT, **over),
                       tuning=dict(chained=0, coarse_batch_px=0))
    ctx.upload_frames(0, np.stack([f for p in pairs for f in p[:2]]), np.stack([p[2] for p in pairs for _ in (0, 1)]) if depth else None)
    ctx.build_pyramids(0, 2 * DISTINCT)
    ctx.apply_gradient(0, 2 * DISTINCT)
    got = {}
    for typed in (1, 0):
        for refs in ([0, 2, 4], [0], [2], [4]):
            ctx.set_tuning(typed_loads=typed, target_blocks=slices_per_pair * len(refs))
            ref = np.asarray(refs)
            poses, stats = ctx.estimate_pose_batch(ref, ref + 1, raise_on_pair_failure=True)
            got[(typed, len(refs) > 1)] = got.get((typed, len(refs) > 1), []) + [_bits(poses, stats, i) for i in range(len(refs))]
    ctx.close()
    for i in range(DISTINCT):
        st, pose_cpu, tr = want[i]
        for typed in (1, 0):
            alone, batch = got[(typed, False)][i], got[(typed, True)][i]
            assert alone[0] == pose_cpu.view(np.uint32).tobytes(), (typed, i, alone, pose_cpu)
            # uwt_stats against the oracle: status, evaluations, and the last evaluation's valid count and error (Σ r² / n in f32)
            want_stats = (st, len(tr), tr[-1]["n_valid"], np.float32(tr[-1]["error"]).view(np.uint32).item())
            print("typed", typed, "pair", i, "stats", alone[1:], "oracle", want_stats)
            assert alone[1:] == want_stats, (typed, i, alone[1:], want_stats)
            assert batch == alone, (typed, i)
        assert got[(1, False)][i] == got[(0, False)][i], i
    return got


def test_tiny_levels_with_depth_holes(capi, O, synth):
    """64 x 48, 4 levels, depth with holes.  The 8 x 6 level has 12 groups for a block's 256 lanes: the inactive lanes walk rows far
    past the level — 127 rows past its 6 — and read their rays inside the block's tables all the same."""
    _three_ways(capi, O, synth, 64, 48, (52.5, 52.5, 31.5, 23.5), 4, True)


def test_slices_that_begin_mid_row(capi, O, synth):
    """160 x 96, 4 levels, level 0 cut into 5 slices of 768 groups per pair (target_blocks = 5 per pair: 3840 groups, 3 per thread):
    slices begin at pixel 3072 k, column 32 k mod 160 — mid-row — and a block takes three steps (both bodies of the loop and the odd
    tail), wrapping on some and not on others (step: 6 rows + 64 columns)."""
    _three_ways(capi, O, synth, 160, 96, (131.25, 131.25, 79.5, 47.5), 4, True, slices_per_pair=5)


@pytest.mark.one_arith
def test_pitched_ragged_rows(capi, O, synth):
    """150 x 94, 2 levels: rows of 150 points in a pitch of 152, 75 in 76 — the walk wraps at the pitch, the row's last group is
    masked by the integer column (x < gw, x < gw & ~3)."""
    _three_ways(capi, O, synth, 150, 94, (123.0, 123.0, 74.5, 46.5), 2, True, slices_per_pair=3)


@pytest.mark.one_arith
def test_pitch_above_one_step(capi, O, synth):
    """1280 x 32, 2 levels: a step of 1024 pixels is less than a row of level 0, so the row step is 0 and a step wraps or does not;
    10 slices of four steps per pair."""
    _three_ways(capi, O, synth, 1280, 32, (1050.0, 1050.0, 639.5, 15.5), 2, True, slices_per_pair=10)


@pytest.mark.one_arith
def test_other_focal_lengths_off_centre_no_depth(capi, O, synth):
    """160 x 96 with fx != fy and an off-centre principal point, no depth plane (z = 1): X0 and Y0 come from different intrinsics, so
    a swapped or shifted table shows; two slices of eight steps per pair."""
    _three_ways(capi, O, synth, 160, 96, (131.25, 128.5, 71.25, 52.75), 4, False, slices_per_pair=2)
