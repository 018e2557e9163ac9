"""The robust scale stage in every device form, on the designed residual histograms of tests/scale_cases.py (tests/test_scale_cpu.py
shows that each case reaches its target and that the set tells the rule from its near misses):

  k_resid_hist_v + the dump form     uwt_residual_jacobian_weighted: inv_mad read directly, every r and w, the sums
  k_coarse_weighted                  level 1 of a dense alignment (3072 px): its own LDS histogram, wave_scale in place, the weight table
  k_hist_iterate + the weighted pass level 0 of a dense alignment, and both levels with uwt_tuning::coarse_weighted = 0
  k_table_hist                       uwt_estimate_pose_points and uwt_estimate_pose_candidates_batch_opt: one replica, per-pair tickets

The scale and the weights are held to the plain restatement tests/scale_ref.py, sums and poses to the oracle, bit for bit."""
import importlib
from fractions import Fraction

import numpy as np
import pytest

import metric_ref as MR
import scale_cases as S
import scale_ref as R
import seeded_ref as SR

pytestmark = pytest.mark.gpu
F = np.float32
MODES = {"tukey": (S.TUKEY, 0), "huber": (S.HUBER, 0), "huber_bilinear": (S.HUBER, 1)}
NO_VALID = SR.ERR_NO_VALID_POINTS


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


_frames = {}
_want = {}


def frames(case):
    if case.id not in _frames:
        _frames[case.id] = case.frames()
    return _frames[case.id]


def make_ctx(capi, size, kind, sampler, depth, n_pairs, tuning=None, **over):
    w, h, intr, nl = S.SIZES[size]
    kw = dict(n_levels=nl, first_level=nl - 1, last_level=0, max_iters=2, early_exit=0, weights=kind, sampler=sampler,
              has_depth=int(depth), max_frames=2 * n_pairs, max_pairs=n_pairs)
    kw.update(over)
    return capi.Context(capi.default_params(w, h, *intr, **kw), tuning=tuning)


def load(ctx, cases, first_pair=0):
    fr = [frames(c) for c in cases]
    gray = np.stack([f for i1, i2, _ in fr for f in (i1, i2)])
    dep = np.stack([d for _, _, d in fr for _ in (0, 1)]) if cases[0].has_depth else None
    ctx.upload_frames(2 * first_pair, gray, dep)
    ctx.build_pyramids(2 * first_pair, 2 * len(cases))
    ctx.apply_gradient(2 * first_pair, 2 * len(cases))


def result_bits(poses, stats):
    """one tuple per pair: (pose bytes, status, evaluations, n_valid, error bits); a failed pair: its status alone"""
    out = []
    for i, s in enumerate(stats):
        if s["status"]:
            out.append((int(s["status"]),))
        else:
            out.append((np.ascontiguousarray(poses[i], F).tobytes(), 0, int(s["iterations"]), int(s["n_valid"]),
                        int(F(s["error"]).view(np.uint32))))
    return out


def want_bits(result):
    st, pose, tr = result
    return (int(st),) if st else (np.asarray(pose, F).tobytes(),) + SR.stats_of(st, tr)


def oracle_align(O, arith, case, sampler=0, **over):
    key = (arith, case.id, sampler, tuple(sorted(over.items())))
    if key not in _want:
        i1, i2, dep = frames(case)
        p = S.oracle_params(O, case, sampler=sampler, early_exit=0, **over)
        _want[key] = want_bits(O.align_pair(p, i1, i2, dep, want_trace=True))
    return _want[key]


# ---------------------------------------------------------------- the per-stage entry: dense scale pass + dump form

def stage_reference(O, arith, case, lvl, sampler):
    key = ("stage", arith, case.id, lvl, sampler)
    if key not in _want:
        J, r, idx, ng = S.evaluate(O, case, lvl, sampler, frames(case))
        med, dmed, mad, inv_mad, n = R.scale(r, case.kind)
        W = R.weights(case.kind, r, inv_mad)
        A, b = O.normal_equations(J, r, W, 50.0)
        err = O.error(r, W)[0] if n else 0.0
        vals, first, counts = np.unique(r, return_index=True, return_counts=True)      # the error numerator, exactly
        num = sum((int(c) * Fraction(float(R.weighted_terms(v, W[i], 50.0)[1])) for v, i, c in zip(vals, first, counts)), Fraction(0))
        _want[key] = (J, r, idx, ng, inv_mad, W, A, b, (err, num))
    return _want[key]


def check_stage(ctx, O, arith, case, lvl, sampler):
    J, r, idx, ng, inv_mad, W, A, b, err = stage_reference(O, arith, case, lvl, sampler)
    out = ctx.residual_jacobian_weighted(0, 1, lvl, S.IDENTITY)
    what = (case.id, lvl, sampler)
    assert F(out["inv_mad"]).tobytes() == inv_mad.tobytes(), (what, out["inv_mad"], inv_mad)     # the one place dmed is read directly
    valid = np.zeros(ng, np.uint8)
    valid[idx] = 1
    assert np.array_equal(out["valid"], valid) and out["n_valid"] == len(r), what
    assert np.array_equal(out["r"][idx].view(np.uint32), r.view(np.uint32)), what
    assert np.array_equal(out["J"][idx].view(np.uint32), J.view(np.uint32)), what
    assert np.array_equal(out["w"][idx].view(np.uint32), W.view(np.uint32)), what
    assert np.array_equal(out["A"].astype(F), A) and np.array_equal((-out["jtr"]).astype(F), b), what
    err, num = err
    if len(r):
        assert F(np.float64(F(1.0 / len(r))) * out["err_num"]) == F(err), what
        assert abs(Fraction(out["err_num"]) - num) <= len(r) * Fraction(2) ** -53 * num, what      # an f64 sum of exact products
    else:
        assert out["err_num"] == 0 and not out["A"].any() and not out["jtr"].any(), what


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("family", S.FAMILIES)
def test_per_stage_entry_every_case(capi, O, arith, family, mode):
    """inv_mad, valid, every r, J and w, A, J^T r, the error numerator and n_valid of both levels of every case of the family (its
    constant-depth and 126x94 twins included), Tukey and Huber over the nearest sampler and Huber over the bilinear one"""
    kind, sampler = MODES[mode]
    cases = [c for c in S.CASES if c.family == family and c.kind == kind]
    assert cases
    ctxs = {}
    for c in cases:
        key = (c.size, c.has_depth)
        if key not in ctxs:
            ctxs[key] = make_ctx(capi, c.size, kind, sampler, c.has_depth, 1)
        load(ctxs[key], [c])
        for lvl in range(S.SIZES[c.size][3]):
            check_stage(ctxs[key], O, arith, c, lvl, sampler)
    for ctx in ctxs.values():
        ctx.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_per_stage_entry_weight_sweep(capi, O, arith, mode):
    """one 64x48 frame per deviation 0..255, each holding every residual of [-255, 255]: every (residual value, scale) pair at
    median 0 through robust_weight — the Huber quotient k / ax up to ax = 255, the Tukey polynomial and its cut-off"""
    kind, sampler = MODES[mode]
    ctx = make_ctx(capi, "sweep", kind, sampler, False, 1)
    for c in S.sweep_cases(kind):
        load(ctx, [c])
        check_stage(ctx, O, arith, c, 0, sampler)
    ctx.close()


# ---------------------------------------------------------------- dense alignments

GROUPS = {"%s-%s-%s" % (S.KIND_NAME[k], size, "depth" if d else "nodepth"): [c for c in S.CASES if (c.kind, c.size, c.has_depth) == (k, size, d)]
          for k in (S.TUKEY, S.HUBER) for size, d in (("main", False), ("main", True), ("twin", False))}
TUNINGS = {"default": None, "no_coarse_weighted": dict(coarse_weighted=0)}


@pytest.mark.parametrize("tuning", list(TUNINGS))
@pytest.mark.parametrize("group", list(GROUPS))
def test_dense_alignment_matches_oracle(capi, O, arith, group, tuning):
    """uwt_estimate_pose_batch, fixed schedules of 1 and 2 iterations, levels 1 -> 0 (k_coarse_weighted with the weight table, then
    k_hist_iterate + the weighted pass; both chained with coarse_weighted = 0) and level 0 alone: poses, status, evaluations, n_valid
    and error bits of every case alone and of all cases as one batch in two orders (per-pair bins and ticket words; the pairs without
    a valid pixel fail with the oracle's status beside live ones)."""
    cases = GROUPS[group]
    n = len(cases)
    assert n
    ctx = make_ctx(capi, cases[0].size, cases[0].kind, 0, cases[0].has_depth, n, tuning=TUNINGS[tuning])
    load(ctx, cases)
    order = np.random.default_rng(n).permutation(n)
    for first_level in (1, 0):
        for max_iters in (1, 2):
            over = dict(first_level=first_level, last_level=0, max_iters=max_iters)
            ctx.update_params(**over)
            want = [oracle_align(O, arith, c, **over) for c in cases]
            got = result_bits(*ctx.estimate_pose_batch(2 * np.arange(n), 2 * np.arange(n) + 1))
            bad = [(cases[i].id, got[i][1:], want[i][1:]) for i in range(n) if got[i] != want[i]]
            assert not bad, (over, len(bad), bad[:5])
            got = result_bits(*ctx.estimate_pose_batch(2 * order, 2 * order + 1))
            assert got == [want[i] for i in order], over
            for i in range(n):
                assert result_bits(*ctx.estimate_pose_batch([2 * i], [2 * i + 1])) == [want[i]], (over, cases[i].id)
    if any(c.n == 0 for c in cases):
        assert any(w == (NO_VALID,) for w in want)
    ctx.close()


def test_dense_alignment_huber_bilinear_weight_sweep(capi, O, arith):
    """Huber over the bilinear sampler samples at integer positions at the identity, so one evaluation of the alignment loop sees the
    designed residuals: the 256 sweep frames as one batch and alone give the oracle's bits — the hand-written quotient of
    robust_weight<true> (refined reciprocal + two corrections) against the IEEE k / ax for every (residual, deviation) pair at
    median 0 — and so do the nearest forms of both kinds."""
    for mode, (kind, sampler) in MODES.items():
        cases = S.sweep_cases(kind)
        n = len(cases)
        ctx = make_ctx(capi, "sweep", kind, sampler, False, n, max_iters=1)
        load(ctx, cases)
        want = [oracle_align(O, arith, c, sampler=sampler, max_iters=1) for c in cases]
        assert all(w[1] == 0 for w in want)
        got = result_bits(*ctx.estimate_pose_batch(2 * np.arange(n), 2 * np.arange(n) + 1))
        bad = [(cases[i].id, got[i][1:], want[i][1:]) for i in range(n) if got[i] != want[i]]
        assert not bad, (mode, len(bad), bad[:5])
        for i in range(0, n, 15):
            assert result_bits(*ctx.estimate_pose_batch([2 * i], [2 * i + 1])) == [want[i]], (mode, i)
        ctx.close()


def test_dense_alignment_huber_bilinear_cases(capi, O, arith):
    """one evaluation per level-0 alignment under Huber / bilinear for every Huber case without depth (deviations above 255 are in
    the depth group, below): the chained bilinear scale pass on the designed histograms"""
    for group in ("huber-main-nodepth", "huber-main-depth", "huber-twin-nodepth"):
        cases = GROUPS[group]
        n = len(cases)
        ctx = make_ctx(capi, cases[0].size, S.HUBER, 1, cases[0].has_depth, n, first_level=0, max_iters=1)
        load(ctx, cases)
        want = [oracle_align(O, arith, c, sampler=1, first_level=0, last_level=0, max_iters=1) for c in cases]
        got = result_bits(*ctx.estimate_pose_batch(2 * np.arange(n), 2 * np.arange(n) + 1))
        bad = [(cases[i].id, got[i][1:], want[i][1:]) for i in range(n) if got[i] != want[i]]
        assert not bad, (group, len(bad), bad[:5])
        ctx.close()


# ---------------------------------------------------------------- tables

TABLE_ROWS = [1, 2, 3, 1023, 1024, 1025, 2049]        # the slice boundaries of kFeatPtsPerBlock = 1024: tickets over 1, 2 and 3 blocks
TABLE_CASES = ["lane_dmed-tukey-dmed127", "lane_dmed-tukey-dmed128", "saturation-tukey-fallback", "saturation-tukey-all200",
               "lane_dmed-huber-dmed247", "lane_dmed-huber-dmed248", "lane_med-huber-med-8", "lane_med-huber-med-7",
               "one_sided-huber-med-200_dmed55_spread"]


def table_rows(case, count, seed, lvl=0):
    """`count` distinct counted pixels of a level of the case as table rows (x, y, 1, 1)"""
    w, h = (v >> lvl for v in S.SIZES[case.size][:2])
    pix = np.random.default_rng(seed).permutation((w - 1) * (h - 1))[:count]
    t = np.ones((count, 4), F)
    t[:, 0] = 1 + pix % (w - 1)
    t[:, 1] = 1 + pix // (w - 1)
    return t


@pytest.mark.parametrize("mode", list(MODES))
def test_tables_estimate_pose_points(capi, O, arith, mode):
    """uwt_estimate_pose_points under the context's weights, both samplers, on tables the test writes: rows naming pixels of a designed
    frame (their residuals are the map's), 1 .. 2049 rows, against oracle.align_pair_points; with 1023 rows and more the table's own
    scale is the case's target (asserted through the restatement)"""
    kind, sampler = MODES[mode]
    by_id = {c.id: c for c in S.CASES}
    cases = [by_id[i] for i in TABLE_CASES if by_id[i].kind == kind]
    ctx = make_ctx(capi, "main", kind, sampler, False, 1, n_levels=2, first_level=0, last_level=0, max_iters=2)
    for c in cases:
        load(ctx, [c])
        i1, i2, _ = frames(c)
        p = S.oracle_params(O, c, sampler=sampler, first_level=0, last_level=0, max_iters=2, early_exit=0)
        for rows in TABLE_ROWS:
            t = table_rows(c, rows, rows)
            if rows >= 1023:
                q = S.level_map(c, 0)[t[:, 1].astype(int), t[:, 0].astype(int)]
                assert R.scale(q.astype(F), kind)[:2] == tuple(c.target), (c.id, rows)
            want = want_bits(O.align_pair_points(p, i1, i2, {0: t}, want_trace=True))
            pose, st = ctx.estimate_pose_points(0, 1, {0: t})
            assert result_bits([pose], [st]) == [want], (c.id, rows, st, want[1:])
    ctx.close()


def candidate_pair(O, box, seed):
    """(I1, I2, candidate rows, q of the rows): a flat reference with a box of two-band noise, so that Tracker::ObtainCandidatePoints
    picks pixels of the box; the map — 40 % at 0, 30 % at +200, 30 % at -136: median 0, deviation 136 = lane 17, k = 0 — is then placed
    on those pixels (a dark pixel takes 0 or +200, a bright one 0 or -136)."""
    w, h = S.SIZES["main"][:2]
    rng = np.random.default_rng(seed)
    i1 = np.full((h, w), 128, np.int32)
    y0, y1, x0, x1 = box
    dark = rng.random((y1 - y0, x1 - x0)) < 0.5
    i1[y0:y1, x0:x1] = np.where(dark, rng.integers(20, 56, dark.shape), rng.integers(200, 236, dark.shape))
    i1 = i1.astype(np.uint8)
    pts, n = O.candidate_points(O.gradient_mag(*O.scharr3(i1)), None, 20.0)
    i2 = i1.astype(np.int32)
    px, py = pts[:, 0].astype(int), pts[:, 1].astype(int)
    at = i1[py, px].astype(np.int32)
    step = rng.random(n) < 0.6
    q = np.where(step, np.where(at < 128, 200, np.where(at > 128, -136, 0)), 0)
    i2[py, px] += q
    assert i2.min() >= 0 and i2.max() <= 255
    return i1, i2.astype(np.uint8), pts, q


def test_tables_candidates_batch(capi, O, arith):
    """uwt_estimate_pose_candidates_batch_opt on three pairs whose candidate sets take 1, 2 and 3 slices (hist_flush_scale<1> expects a
    different ticket count per pair): against the oracle and against the per-pair path, Tukey and Huber, both samplers"""
    boxes = [(30, 54, 40, 70), (10, 46, 20, 64), (8, 54, 10, 62)]           # 831, 1747 and 2586 candidates
    pairs = [candidate_pair(O, b, 40 + i) for i, b in enumerate(boxes)]
    slices = [(len(p[2]) + 1023) // 1024 for p in pairs]
    assert slices == [1, 2, 3], [len(p[2]) for p in pairs]
    w, h, intr, _ = S.SIZES["main"]
    over = dict(n_levels=2, first_level=0, last_level=0, max_iters=2, early_exit=0)
    gray = np.stack([f for p in pairs for f in p[:2]])
    for mode, (kind, sampler) in MODES.items():
        for i1, i2, pts, q in pairs:
            counted = (pts[:, 0] > 0) & (pts[:, 1] > 0)
            assert R.scale(q[counted].astype(F), kind)[:2] == (0, 136)
        po = O.default_params(w, h, *intr, weights=kind, sampler=sampler, **over)
        want = [want_bits(O.align_pair_points(po, i1, i2, {0: pts}, want_trace=True)) for i1, i2, pts, q in pairs]
        assert all(x[1] == 0 for x in want)
        ctx = capi.Context(capi.default_params(w, h, *intr, max_frames=6, max_pairs=3, weights=kind, sampler=sampler, **over))
        ctx.upload_frames(0, gray)
        ctx.build_pyramids(0, 6)
        ctx.apply_gradient(0, 6)
        for order in ([0, 1, 2], [2, 0, 1], [1]):
            ref = 2 * np.array(order)
            got = result_bits(*ctx.estimate_pose_candidates_batch(ref, ref + 1, weights=kind, sampler=sampler))
            assert got == [want[i] for i in order], (mode, order)
        for i in range(3):
            tab, n = ctx.obtain_candidate_points(2 * i, 0)
            assert n == len(pairs[i][2])
            pose, st = ctx.estimate_pose_points(2 * i, 2 * i + 1, {0: tab})
            assert result_bits([pose], [st]) == [want[i]], (mode, i)
        ctx.close()


# ---------------------------------------------------------------- histograms left clean

def test_histograms_and_tickets_are_left_clean(capi, O, arith):
    """a call of one case, then a call of a different case on the same context: the second gives the bytes it gives on a fresh context
    (the last block leaves the bins and the ticket word all-zero) — after a live pair, after a pair without a valid pixel, after the
    saturation fallback, in the per-stage entry, the dense alignment (both coarse forms), and the table entry"""
    by_id = {c.id: c for c in S.CASES}
    second = by_id["ties-huber-n1000"]
    firsts = [by_id[i] for i in ("ties-huber-n0", "ties-huber-n1", "lane_dmed-huber-dmed510", "one_sided-huber-med200_dmed100")]
    tables = {0: table_rows(second, 1500, 7), 1: table_rows(second, 700, 8, lvl=1)}

    def calls(ctx):
        out = [ctx.residual_jacobian_weighted(2, 3, lvl, S.IDENTITY) for lvl in (1, 0)]
        a = [(o["inv_mad"], o["w"].tobytes(), o["A"].tobytes(), o["jtr"].tobytes(), o["err_num"], o["n_valid"]) for o in out]
        b = result_bits(*ctx.estimate_pose_batch([2], [3]))
        pose, st = ctx.estimate_pose_points(2, 3, tables)
        return a, b, result_bits([pose], [st])

    for tuning in TUNINGS.values():
        fresh = make_ctx(capi, "main", S.HUBER, 0, True, 2, tuning=tuning)
        load(fresh, [second], first_pair=1)
        want = calls(fresh)
        fresh.close()
        assert want[1] == [oracle_align(O, arith, second, first_level=1, last_level=0, max_iters=2)]
        for first in firsts:
            ctx = make_ctx(capi, "main", S.HUBER, 0, True, 2, tuning=tuning)
            load(ctx, [first, second])
            ctx.residual_jacobian_weighted(0, 1, 0, S.IDENTITY)
            ctx.residual_jacobian_weighted(0, 1, 1, S.IDENTITY)
            ctx.estimate_pose_batch([0], [1])
            ctx.estimate_pose_batch([0, 2], [1, 3])
            ctx.estimate_pose_points(0, 1, tables)
            assert calls(ctx) == want, first.id
            ctx.close()


# ---------------------------------------------------------------- the metric Jacobian keeps the scale's bits

def test_metric_jacobian_keeps_the_scale(capi, O, arith):
    """lane-walk cases under UWT_JACOBIAN_METRIC (that mode has no k_coarse_weighted: both levels take the chained form): inv_mad and
    every weight as in the reference mode, J the metric one, and the alignment against the restated loop over the metric oracle"""
    by_id = {c.id: c for c in S.CASES}
    M = MR.MetricOracle(O)
    for cid in ("lane_dmed-tukey-dmed199", "lane_dmed-huber-dmed200", "lane_dmed-huber-dmed504"):
        c = by_id[cid]
        ctx = make_ctx(capi, "main", c.kind, 0, c.has_depth, 1)
        load(ctx, [c])
        ctx.set_jacobian("metric")
        i1, i2, dep = frames(c)
        p = S.oracle_params(O, c, early_exit=0, max_iters=2)
        for lvl in (1, 0):
            J, r, idx, ng, inv_mad, W, A, b, err = stage_reference(O, arith, c, lvl, 0)
            out = ctx.residual_jacobian_weighted(0, 1, lvl, S.IDENTITY)
            assert F(out["inv_mad"]).tobytes() == inv_mad.tobytes() and out["n_valid"] == len(r)
            assert np.array_equal(out["w"][idx].view(np.uint32), W.view(np.uint32))
            assert np.array_equal(out["r"][idx].view(np.uint32), r.view(np.uint32))
            L = O.level_intrinsics(p, lvl)
            a_img, b_img = O.pyramid(i1, 2)[lvl], O.pyramid(i2, 2)[lvl]
            pts = O.dense_points(O.pyramid(dep, 2)[lvl] if dep is not None else None, L.w, L.h, lvl)
            Jm = M.residual_jacobian_ex(a_img, b_img, *O.scharr3(a_img), pts, O.warp(pts, S.IDENTITY, L), L, p.z_factor, p.angle_factor, 0)[0]
            assert np.array_equal(out["J"][idx].view(np.uint32), Jm.view(np.uint32)) and not np.array_equal(Jm, J)
        want = want_bits(SR.align(M, p, i1, i2, dep, keep=False))
        assert want[1] == 0
        assert result_bits(*ctx.estimate_pose_batch([0], [1])) == [want], cid
        ctx.close()
