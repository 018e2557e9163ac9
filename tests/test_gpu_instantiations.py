"""Every combination of run-time facts by which the dispatchers (uwt_launch_residual / _general / _flow / _points / _metric.hip) pick
an instantiation of the kernels that form Jw and the sums, driven through the public ABI at the smallest shapes at which the selection
still happens, and compared with the oracle (reference mode) or tests/metric_ref.py (metric mode) through tests/seeded_ref.py's loop —
bit for bit, as everywhere else in the suite.  profiles/r29/README.md says which instantiations no test launched before this file
existed; tests/golden/kernel_coverage.txt says for every kernel of the library which file compares it.

The selectors (one table each below): arithmetic set (the `arith` fixture), depth plane, f32 / f64 sums, unit factors, fx == fy,
rows that are whole groups of four or not (48 x 36: 48 / 24 / 12 wide; 46 x 35: 46 / 23 / 11 wide), typed / streamed plane loads
(uwt_tuning::typed_loads, stream_bytes), the dump forms, sampler and weights, the Jacobian mode, the pair count on both sides of
k_iterate's threshold (1, 3 | 4) and the number of coarse levels one launch takes (0, 1, 2).

An expectation is computed once per (arith, Jacobian mode, size, intrinsics, factors, depth, weights, sampler, schedule, scene) and
shared by every tuning and launch form that must reproduce it.  One place has a bar instead of equal bits, the suite's
own: the sums of ONE evaluation through the per-stage entry: the entry returns them in f64 and the oracle has no such output, so they
are held to the f64 sums of the (bit-equal) J rows — 1e-11 of sqrt(A_ii A_jj) for f64 sums (tests/test_gpu_metric.py: n * 2^-53 of exact
products), 2e-6 for f32 sums (tests/test_gpu_parity.py) — with n_valid and the integer sum of r^2 exact."""
import importlib

import numpy as np
import pytest

import metric_ref as MR
import seeded_ref as SR
import table_f32_ref as TF

pytestmark = pytest.mark.gpu

REFERENCE, METRIC = 0, 1
SIZES = {"48x36": (48, 36), "46x35": (46, 35)}                  # whole groups of four on every level / ragged rows on every level
INTRINSICS = {"square": lambda w, h: (40.0, 40.0, w / 2 - 0.5, h / 2 - 0.5),
              "nonsquare": lambda w, h: (41.5, 39.25, w / 2 - 0.3, h / 2 + 0.2)}
FACTORS = {"unit": (1.0, 1.0), "nonunit": (0.5, 1.25)}
N_SCENES = 4                                                    # pair k of a call is scene k: slots 2k, 2k + 1
SCHEDULES = {"two_coarse": dict(n_levels=3, first_level=2, last_level=0, max_iters=3, early_exit=0),   # k_coarse takes levels 2 and 1
             "one_coarse": dict(n_levels=3, first_level=1, last_level=0, max_iters=3, early_exit=0)}   # ... level 1 alone
POSE = np.array([0.012, -0.007, 0.005, 0.004, -0.003, 0.006], np.float32)   # a twist: the per-pixel tests' pose is its exponential
NO_STREAM = 1 << 40

_scenes, _want, _terms = {}, {}, {}


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def scenes(synth, size, intr):
    """N_SCENES rendered (ref, tgt, depth) triples of one geometry, made once"""
    key = (size, intr)
    if key not in _scenes:
        w, h = SIZES[size]
        _scenes[key] = [synth.render_pair(w, h, *INTRINSICS[intr](w, h), seed=4100 + 7 * i + w, max_t=0.02, max_deg=1.5, with_depth=True,
                                          z=1.2)[:3] for i in range(N_SCENES)]
    return _scenes[key]


def params_over(factors, depth, weights=0, sampler=0, schedule="two_coarse", **more):
    zf, af = FACTORS[factors]
    return dict(SCHEDULES[schedule], has_depth=int(depth), z_factor=zf, angle_factor=af, weights=weights, sampler=sampler, **more)


def make_ctx(capi, synth, size, intr, max_pairs=N_SCENES, **over):
    w, h = SIZES[size]
    ctx = capi.Context(capi.default_params(w, h, *INTRINSICS[intr](w, h), max_frames=2 * N_SCENES, max_pairs=max_pairs, **over))
    sc = scenes(synth, size, intr)
    ctx.upload_frames(0, np.stack([f for r, t, _ in sc for f in (r, t)]),
                      np.stack([d for _, _, d in sc for _ in (0, 1)]) if over.get("has_depth") else None)
    ctx.build_pyramids(0, 2 * N_SCENES)
    ctx.apply_gradient(0, 2 * N_SCENES)
    t = ctx.get_tuning()
    ctx.default_tuning = {f: getattr(t, f) for f, _ in t._fields_ if f != "reserved"}
    return ctx


def set_form(ctx, jacobian, tuning):
    """the context's defaults with `tuning` over them, and the Jacobian mode"""
    ctx.set_tuning(**dict(ctx.default_tuning, **tuning))
    ctx.set_jacobian(jacobian)


def oracle_of(O, jacobian):
    return MR.MetricOracle(O) if jacobian == METRIC else O


def want(O, synth, arith, jacobian, size, intr, scene, **over):
    """(pose bytes, status, evaluations, n_valid, error bits) of one scene's alignment by the restatement, computed once"""
    key = (arith, jacobian, size, intr, scene, tuple(sorted(over.items())))
    if key not in _want:
        w, h = SIZES[size]
        ref, tgt, dep = scenes(synth, size, intr)[scene]
        st, pose, tr = SR.align(oracle_of(O, jacobian), O.default_params(w, h, *INTRINSICS[intr](w, h), **over), ref, tgt,
                                dep if over["has_depth"] else None)
        _want[key] = (np.asarray(pose, np.float32).tobytes(),) + SR.stats_of(st, tr)
    return _want[key]


def bits(poses, stats):
    return [(np.ascontiguousarray(poses[i], np.float32).tobytes(), int(s["status"]), int(s["iterations"]), int(s["n_valid"]),
             int(np.float32(s["error"]).view(np.uint32))) for i, s in enumerate(stats)]


def check_forms(capi, O, synth, arith, size, intr, forms, jacobians=(REFERENCE, METRIC), **over):
    """one context of these parameters through every (name, pairs, tuning) of `forms` in both Jacobian modes: every pair's pose bytes
    and stats are the restatement's"""
    ctx = make_ctx(capi, synth, size, intr, **over)
    for jacobian in jacobians:
        wants = [want(O, synth, arith, jacobian, size, intr, k, **over) for k in range(N_SCENES)]
        assert all(w[2] > 0 and w[3] > 0 for w in wants)                              # evaluations ran on valid points
        for name, n, tuning in forms:
            set_form(ctx, jacobian, tuning)
            slots = np.arange(n, dtype=np.int32)
            got = bits(*ctx.estimate_pose_batch(2 * slots, 2 * slots + 1))
            case = (size, intr, over, "metric" if jacobian else "reference", name)
            assert got == wants[:n], (case, [g[1:] for g in got], [w[1:] for w in wants[:n]])
    ctx.close()


# ---- 1. one evaluation through the per-stage entries: k_residual's dump forms and the sums of the accumulating forms ---------------------
def level_terms(O, synth, arith, jacobian, size, intr, factors, depth, sampler=0):
    """per level: (J, r, idx) of scene 0 at se3_exp(POSE) by the restatement, computed once"""
    key = (arith, jacobian, size, intr, factors, depth, sampler)
    if key not in _terms:
        w, h = SIZES[size]
        zf, af = FACTORS[factors]
        ref, tgt, dep = scenes(synth, size, intr)[0]
        p = O.default_params(w, h, *INTRINSICS[intr](w, h), **params_over(factors, depth))
        a_pyr, b_pyr = O.pyramid(ref, 3), O.pyramid(tgt, 3)
        d_pyr = O.pyramid(dep, 3) if depth else [None] * 3
        pose = O.se3_exp(POSE)
        out = []
        for lvl in range(3):
            L = O.level_intrinsics(p, lvl)
            gx, gy = O.scharr3(a_pyr[lvl])
            pts = O.dense_points(d_pyr[lvl], L.w, L.h, lvl)
            J, r, idx = oracle_of(O, jacobian).residual_jacobian_ex(a_pyr[lvl], b_pyr[lvl], gx, gy, pts, O.warp(pts, pose, L), L, zf, af, sampler)
            assert len(idx) > L.w * L.h // 3
            out.append((J, r, idx, L.w * L.h))
        _terms[key] = out
    return _terms[key]


def check_terms(out, J, r, idx, n, case):
    valid = np.zeros(n, np.uint8)
    valid[idx] = 1
    assert np.array_equal(out["valid"], valid), case
    assert np.array_equal(out["r"][idx].view(np.uint32), np.asarray(r, np.float32).view(np.uint32)), case
    bad = np.argwhere(out["J"][idx].view(np.uint32) != J.view(np.uint32))
    assert len(bad) == 0, (case, len(bad), bad[:4])


def check_sums(acc, J, r, idx, bar, case):
    Jd = J.astype(np.float64)
    A_ref = Jd.T @ Jd
    scale = np.sqrt(np.outer(np.diag(A_ref), np.diag(A_ref)))
    mag = np.abs(Jd).T @ np.abs(r.astype(np.float64))
    assert acc["n_valid"] == len(idx) and acc["sum_r2"] == int((r.astype(np.int64) ** 2).sum()), case
    assert (np.abs(acc["A"] - A_ref) <= bar * scale).all(), (case, float((np.abs(acc["A"] - A_ref) / scale).max()))
    assert (np.abs(acc["jtr"] - Jd.T @ r.astype(np.float64)) <= bar * mag + 1e-30).all(), case


@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
@pytest.mark.parametrize("size", list(SIZES))
def test_identity_evaluation(capi, O, synth, arith, size, depth):
    """uwt_residual_jacobian on levels 0..2: valid, r and J of the dump form and the sums of the accumulating form, for fx == fy or
    not x unit factors or not x f64 / f32 sums x typed loads on / off x both Jacobian modes (k_residual<.., SAMPLER 0, WEIGHTS 0, ..>)"""
    pose = O.se3_exp(POSE)
    for intr in INTRINSICS:
        for factors in FACTORS:
            for acc64 in (1, 0):
                ctx = make_ctx(capi, synth, size, intr, max_pairs=1, **params_over(factors, depth, accumulate_f64=acc64))
                for jacobian in (REFERENCE, METRIC):
                    terms = level_terms(O, synth, arith, jacobian, size, intr, factors, depth)
                    for typed in ((1, 0) if acc64 and (factors == "unit" or jacobian == METRIC) else (1,)):
                        set_form(ctx, jacobian, dict(typed_loads=typed))
                        for lvl, (J, r, idx, n) in enumerate(terms):
                            case = (size, depth, intr, factors, acc64, jacobian, typed, lvl)
                            check_terms(ctx.residual_jacobian(0, 1, lvl, pose), J, r, idx, n, case)
                            check_sums(ctx.residual_jacobian(0, 1, lvl, pose, dump=False), J, r, idx, 1e-11 if acc64 else 2e-6, case)
                ctx.close()


GENERAL_MODES = {"tukey": (1, 0), "huber": (2, 0), "bilinear": (0, 1), "bilinear_huber": (2, 1)}   # name: (weights, sampler)


@pytest.mark.parametrize("mode", list(GENERAL_MODES))
@pytest.mark.parametrize("size", list(SIZES))
def test_general_evaluation(capi, O, synth, arith, size, mode):
    """uwt_residual_jacobian_weighted (the dump forms of the weighted / bilinear sums and the scale pass in front of them): valid, r,
    J and the weights on levels 0..2, depth or not x unit factors or not x both Jacobian modes, fx != fy"""
    weights, sampler = GENERAL_MODES[mode]
    pose = O.se3_exp(POSE)
    wfun = {0: None, 1: O.tukey_weights, 2: O.huber_weights}[weights]
    for depth in (False, True):
        for factors in FACTORS:
            ctx = make_ctx(capi, synth, size, "nonsquare", max_pairs=1, **params_over(factors, depth, weights, sampler))
            for jacobian in (REFERENCE, METRIC):
                set_form(ctx, jacobian, {})
                for lvl, (J, r, idx, n) in enumerate(level_terms(O, synth, arith, jacobian, size, "nonsquare", factors, depth, sampler)):
                    case = (size, mode, depth, factors, jacobian, lvl)
                    out = ctx.residual_jacobian_weighted(0, 1, lvl, pose)
                    check_terms(out, J, r, idx, n, case)
                    assert out["n_valid"] == len(idx), case
                    if wfun:
                        assert np.array_equal(out["w"][idx].view(np.uint32), wfun(r).view(np.uint32)), case
            ctx.close()


# ---- 2. alignments under identity weights: k_iterate, k_coarse, k_coarse_w4, the accumulating k_residual and its streamed twins ------------
def residual_forms(n):
    """the per-evaluation launches of an n-pair batch: typed or plain plane loads, streamed or not"""
    return [("typed", n, dict(chained=0, coarse_batch_px=0, stream_bytes=NO_STREAM)),
            ("typed, streamed", n, dict(chained=0, coarse_batch_px=0, stream_bytes=0)),
            ("plain", n, dict(chained=0, coarse_batch_px=0, typed_loads=0, stream_bytes=NO_STREAM)),
            ("plain, streamed", n, dict(chained=0, coarse_batch_px=0, typed_loads=0, stream_bytes=0))]


IDENTITY_FORMS = ([("chained, %d" % n, n, dict(chained=1)) for n in (1, 3, 4)] +                         # k_coarse, then k_iterate on level 0
                  [("chained, no coarse launch, %d" % n, n, dict(chained=1, coarse=0)) for n in (1, 3, 4)] +   # k_iterate on every level
                  [("one block per pair and level", 4, dict(chained=0))] +                              # k_coarse_w4 (metric: k_coarse<.., 14, 3, 0>)
                  residual_forms(4))


@pytest.mark.parametrize("depth", [False, True], ids=["nodepth", "depth"])
@pytest.mark.parametrize("intr", list(INTRINSICS))
@pytest.mark.parametrize("size", list(SIZES))
def test_identity_alignments(capi, O, synth, arith, size, intr, depth):
    """3 levels x 3 evaluations of 1, 3 and 4 pairs in the chained flow with and without the coarse launch, the batch's one-block coarse
    levels and its per-evaluation launches under every plane-load switch: unit factors or not, both Jacobian modes"""
    for factors in FACTORS:
        check_forms(capi, O, synth, arith, size, intr, IDENTITY_FORMS, **params_over(factors, depth))


@pytest.mark.parametrize("size", list(SIZES))
def test_one_coarse_level(capi, O, synth, arith, size):
    """a schedule that begins on level 1: the chained flow's coarse launch takes one level instead of two"""
    forms = [("chained, %d" % n, n, dict(chained=1)) for n in (1, 4)] + [("one block per pair and level", 4, dict(chained=0))]
    for intr, factors, depth in (("square", "unit", True), ("nonsquare", "nonunit", False)):
        check_forms(capi, O, synth, arith, size, intr, forms, **params_over(factors, depth, schedule="one_coarse"))


# ---- 3. alignments on the general path: k_resid_hist_v, k_hist_iterate, k_coarse_weighted, the weighted k_residual / k_residual_w4 ---------
GENERAL_FORMS = ([("chained, 1", 1, dict(chained=1)), ("chained, 4", 4, dict(chained=1)),                # robust: k_coarse_weighted + k_hist_iterate
                  ("chained, no coarse launch, 2", 2, dict(chained=1, coarse_weighted=0)),
                  ("one block per pair and level", 4, dict(chained=0)),                                   # k_coarse_weighted on every level
                  ("launches", 4, dict(chained=0, coarse_weighted=0, stream_bytes=NO_STREAM)),            # k_resid_hist_v + weighted k_residual
                  ("launches, streamed", 4, dict(chained=0, coarse_weighted=0, stream_bytes=0))])


@pytest.mark.parametrize("mode", list(GENERAL_MODES))
@pytest.mark.parametrize("intr", list(INTRINSICS))
@pytest.mark.parametrize("size", list(SIZES))
def test_general_alignments(capi, O, synth, arith, size, intr, mode):
    """Tukey, Huber, the bilinear sampler and Huber over it: the chained robust flow, the one-block weighted coarse levels and the
    per-evaluation launches with and without streamed planes; depth or not, unit factors or not, both Jacobian modes"""
    weights, sampler = GENERAL_MODES[mode]
    for depth, factors in ((False, "unit"), (True, "unit"), (False, "nonunit"), (True, "nonunit")):
        check_forms(capi, O, synth, arith, size, intr, GENERAL_FORMS, **params_over(factors, depth, weights, sampler))


# ---- 4. point tables under f32 sums: k_table_eval<.., float> --------------------------------------------------------------------------------
@pytest.mark.parametrize("factors", list(FACTORS))
@pytest.mark.parametrize("size", list(SIZES))
def test_table_alignments_f32_sums(capi, O, synth, arith, size, factors):
    """uwt_estimate_pose_points over every grid point of every level as a table (1728 / 1610 rows on level 0: two blocks of 1024, the
    second partly filled), both Jacobian modes, f64 and f32 sums.  The oracle sums in f64 only; under accumulate_f64 = 0 the kernel's
    f32 part is each thread's chain of fused multiply-adds over its four rows, which tests/table_f32_ref.py restates together with the
    f64 order behind it: pose bytes and stats are the restatement's in both forms, and the two forms' poses differ"""
    w, h = SIZES[size]
    intr = "nonsquare"
    ref, tgt, dep = scenes(synth, size, intr)[0]
    p = O.default_params(w, h, *INTRINSICS[intr](w, h), **params_over(factors, True))   # (the oracle has no accumulate_f64)
    tables = {lvl: O.dense_points(d, O.level_intrinsics(p, lvl).w, O.level_intrinsics(p, lvl).h, lvl) for lvl, d in enumerate(O.pyramid(dep, 3))}
    wants = {}
    for acc64 in (1, 0):
        ctx = make_ctx(capi, synth, size, intr, max_pairs=1, **params_over(factors, True, accumulate_f64=acc64))
        for jacobian in (REFERENCE, METRIC):
            oracle = oracle_of(O, jacobian)
            st, pose_w, tr = SR.align(oracle if acc64 else TF.F32TableOracle(oracle), p, ref, tgt, dep, tables=tables)
            wants[acc64, jacobian] = (np.asarray(pose_w, np.float32).tobytes(),) + SR.stats_of(st, tr)
            assert wants[acc64, jacobian][1:3] == (0, 9) and wants[acc64, jacobian][3] > w * h // 3
            set_form(ctx, jacobian, {})
            pose, s = ctx.estimate_pose_points(0, 1, tables)
            got = bits([pose], [s])[0]
            assert got == wants[acc64, jacobian], ((size, factors, acc64, jacobian), got[1:], wants[acc64, jacobian][1:])
        ctx.close()
    assert all(wants[0, j][0] != wants[1, j][0] for j in (REFERENCE, METRIC))
