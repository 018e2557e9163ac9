"""The inputs of the seeded-call tests (tests/test_seeded_ref_cpu.py, tests/test_gpu_seeded.py) and the cache of their expectations.
A helper of the tests, not a test.

Scenes: synth.render_pair(160, 96, *INTR, seed=9100 + i, with_depth=True, max_t=0.015, max_deg=0.8); scene i's reference is slot 2i,
its target slot 2i + 1.  Level 0 is 15 360 px (above kCoarseMaxPixels = 6144: the chained and the batch launches), levels 1 and 2 are
3840 / 960 px (k_coarse / k_coarse_w4 / k_coarse_weighted).  One odd size, 101 x 67.
Seeds: oracle.se3_exp(twist), twists drawn from a fixed default_rng in +-[0.01]^3 x +-[0.004]^3 (translation, rotation); seed k goes
with pair k of a call, pair k is scene k % N_SCENES."""
import numpy as np

import seeded_ref as SR

W, H, INTR = 160, 96, (130.0, 130.0, 79.5, 47.5)
ODD = (101, 67, (82.0, 82.0, 50.0, 33.0))
LEVELS = dict(n_levels=3, first_level=2, last_level=0)
N_SCENES = 6
N_SEEDS = 20
TWIST_SCALE = np.array([0.01, 0.01, 0.01, 0.004, 0.004, 0.004])
SEED_RNG = 20261

_scenes = {}
_expect = {}


def scenes(synth, size=(W, H, INTR)):
    """N_SCENES rendered (ref, tgt, depth) triples of one size, made once"""
    w, h, intr = size
    if (w, h) not in _scenes:
        _scenes[(w, h)] = [synth.render_pair(w, h, *intr, seed=9100 + i, with_depth=True, max_t=0.015, max_deg=0.8)[:3]
                           for i in range(N_SCENES)]
    return _scenes[(w, h)]


def seeds(O, n=N_SEEDS):
    """the first n seeds, [n, 7] float32 (the same rows whatever n)"""
    tw = np.random.default_rng(SEED_RNG).uniform(-1.0, 1.0, (N_SEEDS, 6)) * TWIST_SCALE
    return np.stack([O.se3_exp(t.astype(np.float32)) for t in tw[:n]])


def bad_seeds():
    """one non-finite entry each: NaN and +inf, in q and in t"""
    rows = []
    for at, v in ((1, np.nan), (3, np.inf), (5, np.nan), (6, np.inf)):
        s = np.array([0.001, -0.002, 0.0005, 1.0, 0.003, -0.001, 0.002], np.float32)
        s[at] = v
        rows.append(s)
    return np.stack(rows)


def pair_slots(n):
    """the slot lists of an n-pair call: pair k is scene k % N_SCENES"""
    k = np.arange(n) % N_SCENES
    return (2 * k).astype(np.int32), (2 * k + 1).astype(np.int32)


def oracle_params(O, size=(W, H, INTR), depth=True, **over):
    w, h, intr = size
    kw = dict(LEVELS)
    kw.update(over)
    return O.default_params(w, h, *intr, has_depth=1 if depth else 0, **kw)


def expect(O, synth, arith, scene, seed, keep=False, size=(W, H, INTR), depth=True, tables=None, tables_key=None, **over):
    """seeded_ref.align on one scene from one seed (None: the identity), computed once per (arithmetic set, size, params, scene, seed,
    hand-off, tables) and shared, never changed: (status, pose, trace)"""
    key = (arith, size[:2], depth, tuple(sorted(over.items())), scene, None if seed is None else np.asarray(seed, np.float32).tobytes(),
           bool(keep), tables_key)
    if key not in _expect:
        ref, tgt, dep = scenes(synth, size)[scene]
        p = oracle_params(O, size, depth, **over)
        _expect[key] = SR.align(O, p, ref, tgt, dep if depth else None, seed=seed, keep=keep, tables=tables)
    return _expect[key]
