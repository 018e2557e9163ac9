"""The warp and validity stage of the kernels (warp_ray / warp_point, pixel_warp_raw, pixel_sanitize, pixel_gather_index, jw_terms,
pixel_jacobian in uwt_kernels.h, and the table kernels' twins) on the designed cases of tests/validity_cases.py, through every form that
contains the stage, in both arithmetic sets, bit for bit against the oracle (tests/metric_ref.py over it for the metric mode,
tests/seeded_ref.py's loop for the alignments).  tests/test_validity_cpu.py shows, without a GPU, which classes each case reaches and that
each of fourteen plausible mistakes in the stage changes the expectation of a named case.

One place has a bar instead of equal bits, the suite's own (tests/test_gpu_instantiations.py): the f64 sums the per-stage entry returns
with dump = 0 have no oracle output and are held to the f64 sums of the (bit-equal) rows within 1e-11 of sqrt(A_ii A_jj) — n 2^-53 of
exact products is 2e-13 at these sizes — with n_valid and the integer sum of r^2 exact.  NaN payloads of uwt_warp are not compared
(tools/exp/stage_fuzz.py has the same exemption), nor those of a pose that is NaN in the oracle too: a NaN must be a NaN.

The range cases (test_range_cases) sit at the ends of the domain include/uwt.h states for the dense warp's division: bit equality just
inside each bound, the library's refusal just outside it; profiles/r30/README.md has what the device returns beyond."""
import importlib

import numpy as np
import pytest

import cloud_ref as CR
import metric_ref as MR
import seeded_ref as SR
import validity_cases as VC
import validity_ref as VR
import warp_image_ref as WR

pytestmark = pytest.mark.gpu

REFERENCE, METRIC = 0, 1
OK, INVALID_ARG, NO_VALID_POINTS = 0, 1, 2
FACTORS = {"unit": (1.0, 1.0), "nonunit": (0.5, 1.25)}
NO_STREAM = 1 << 40
N_PAIRS = 4


def geometry(case):
    return (case.size, case.intr, case.depth, case.depth_scale)


def geometry_id(g):
    return "%s-%s-%s%s" % (g[0], g[1], g[2] or "nodepth", "" if g[3] == VC.DEPTH_SCALE else "-ds%g" % g[3])


def geometries(cases):
    out = []
    for c in cases:
        if geometry(c) not in out:
            out.append(geometry(c))
    return out


def cases_of(g, cases):
    return [c for c in cases if geometry(c) == g]


DENSE_NORMAL = [c for c in VC.NORMAL if c.table is None]                          # (the single-row size 48 x 4 included, in every form)
DENSE_RANGE = [c for c in VC.RANGE if c.table is None]


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("uw-slam_amd.capi")
    m.lib()
    return m


def make_ctx(capi, case, planes=True):
    """a context of the case's geometry with its frame pair in slots 2k, 2k + 1 of N_PAIRS pairs"""
    w, h = VC.SIZES[case.size]
    ctx = capi.Context(capi.default_params(w, h, *VC.INTRINSICS[case.intr], max_frames=2 * N_PAIRS, max_pairs=2 * N_PAIRS, **VC.params_over(case)))
    if planes:
        ref, tgt, dep = VC.frames_of(case)
        ctx.upload_frames(0, np.stack([ref, tgt] * N_PAIRS), np.stack([dep] * (2 * N_PAIRS)) if dep is not None else None)
        ctx.build_pyramids(0, 2 * N_PAIRS)
        ctx.apply_gradient(0, 2 * N_PAIRS)
    t = ctx.get_tuning()
    ctx.default_tuning = {f: getattr(t, f) for f, _ in t._fields_ if f != "reserved"}
    return ctx


def set_form(ctx, jacobian, tuning):
    ctx.set_tuning(**dict(ctx.default_tuning, **tuning))
    ctx.set_jacobian(jacobian)


_want = {}


def expected(O, case, lvl, factors="unit", sampler=0, jacobian=REFERENCE):
    """(J, r, idx, rows) of one level of a case by the oracle, made once per arithmetic set"""
    key = (MR.current_arith(O), case.name, lvl, factors, sampler, jacobian)
    if key not in _want:
        L, i1, i2, gx, gy, pts = VC.level_inputs(O, case, lvl)
        zf, af = FACTORS[factors]
        J, r, idx = MR.MetricOracle(O, jacobian == METRIC).residual_jacobian_ex(i1, i2, gx, gy, pts, O.warp(pts, case.pose, L), L, zf, af, sampler)
        _want[key] = (J, r, idx, pts.shape[0])
    return _want[key]


def terms_differ(out, J, r, idx, n):
    """None, or what differs between a dump of the per-stage entry and the expectation"""
    valid = np.zeros(n, np.uint8)
    valid[idx] = 1
    if not np.array_equal(out["valid"], valid):
        bad = np.nonzero(out["valid"] != valid)[0]
        return "valid: %d rows, first %s (device %s)" % (len(bad), bad[:4].tolist(), out["valid"][bad[:4]].tolist())
    if out["n_valid"] != len(idx):
        return "n_valid %d against %d" % (out["n_valid"], len(idx))
    if not VR.same_bits(out["r"][idx], r):
        return "r: %d rows" % np.count_nonzero(out["r"][idx].view(np.uint32) != np.asarray(r, np.float32).view(np.uint32))
    bad = np.argwhere(out["J"][idx].view(np.uint32) != J.view(np.uint32))
    if len(bad):
        i, k = bad[0]
        return "J: %d entries, first row %d column %d: device %r, want %r" % (len(bad), idx[i], k, out["J"][idx[i], k], J[i, k])
    return None


def sums_differ(acc, J, r, idx, bar=1e-11):
    Jd = J.astype(np.float64)
    with np.errstate(all="ignore"):
        A_ref = Jd.T @ Jd
        scale = np.sqrt(np.outer(np.diag(A_ref), np.diag(A_ref)))
        mag = np.abs(Jd).T @ np.abs(r.astype(np.float64))
        if acc["n_valid"] != len(idx) or acc["sum_r2"] != int((r.astype(np.int64) ** 2).sum()):
            return "n_valid %d against %d, sum_r2 %d" % (acc["n_valid"], len(idx), acc["sum_r2"])
        if not (np.abs(acc["A"] - A_ref) <= bar * scale).all():
            return "A"
        if not (np.abs(acc["jtr"] - Jd.T @ r.astype(np.float64)) <= bar * mag + 1e-30).all():
            return "jtr"
    return None


# ---- 1. uwt_warp: k_warp_table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", geometries(VC.NORMAL), ids=geometry_id)
def test_warp_table(capi, O, arith, g):
    """all four output columns of uwt_warp on every level's table of every case, the single-row size and the explicit tables included"""
    cases = cases_of(g, VC.NORMAL)
    ctx = make_ctx(capi, cases[0], planes=False)
    for case in cases:
        for lvl in VC.levels_of(case):
            L, _, _, _, _, pts = VC.level_inputs(O, case, lvl)
            want = O.warp(pts, case.pose, L)
            got = ctx.warp(lvl, pts, case.pose)
            assert VR.same_bits(got, want, nan_equal=True), (case.name, lvl, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
            assert np.array_equal(np.isnan(got), np.isnan(want))
    ctx.close()


# ---- 2. the per-stage entry: k_residual's dump forms and the production instantiation's sums -----------------------------------------------
@pytest.mark.parametrize("g", geometries(DENSE_NORMAL), ids=geometry_id)
def test_per_stage_entry(capi, O, arith, g):
    """uwt_residual_jacobian on every level at every case's pose: valid, r, J, n_valid of the dump form and n_valid, sum_r2, A, J^T r of
    the same call with dump = 0, under typed and plain plane loads x unit factors or not x both Jacobian modes (the geometries supply
    whole and ragged rows, fx == fy and not)"""
    cases = cases_of(g, DENSE_NORMAL)
    ctx = make_ctx(capi, cases[0])
    for factors, (zf, af) in FACTORS.items():
        ctx.update_params(z_factor=zf, angle_factor=af)
        for jacobian in (REFERENCE, METRIC):
            for typed in (1, 0):
                set_form(ctx, jacobian, dict(typed_loads=typed))
                for case in cases:
                    for lvl in range(VC.N_LEVELS):
                        J, r, idx, n = expected(O, case, lvl, factors, 0, jacobian)
                        where = (case.name, lvl, factors, jacobian, typed)
                        assert terms_differ(ctx.residual_jacobian(0, 1, lvl, case.pose), J, r, idx, n) is None, where
                        assert sums_differ(ctx.residual_jacobian(0, 1, lvl, case.pose, dump=False), J, r, idx) is None, where
    ctx.close()


# ---- 3. the weighted entry over the bilinear sampler ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", geometries(DENSE_NORMAL), ids=geometry_id)
def test_weighted_entry_bilinear(capi, O, arith, g):
    """uwt_residual_jacobian_weighted with sampler 1 (identity and Huber weights): the sampler's floorf and its "+ 1" clamp at x2 in
    [iw - 1, iw) and in (0, 1) are classes of the cases; valid, r, J and the weights against the oracle's residual_jacobian_ex"""
    cases = cases_of(g, DENSE_NORMAL)
    ctx = make_ctx(capi, cases[0])
    for weights in (0, 2):
        ctx.update_params(sampler=1, weights=weights)
        for jacobian in (REFERENCE, METRIC):
            set_form(ctx, jacobian, {})
            for case in cases:
                for lvl in range(VC.N_LEVELS):
                    J, r, idx, n = expected(O, case, lvl, "unit", 1, jacobian)
                    out = ctx.residual_jacobian_weighted(0, 1, lvl, case.pose)
                    assert terms_differ(out, J, r, idx, n) is None, (case.name, lvl, weights, jacobian)
                    if weights and len(idx):
                        assert VR.same_bits(out["w"][idx], O.huber_weights(r)), (case.name, lvl, jacobian)
    ctx.close()


# ---- 4. one Gauss-Newton step per level from the designed pose: k_iterate, k_coarse, k_coarse_w4 and the per-evaluation launches -------------
STEP_FORMS = [("chained, 1", 1, dict(chained=1)), ("chained, 4", 4, dict(chained=1)),
              ("chained, no coarse launch, 4", 4, dict(chained=1, coarse=0)),
              ("one block per pair and level", 4, dict(chained=0)),
              ("launches, typed, streamed", 4, dict(chained=0, coarse_batch_px=0, stream_bytes=0)),
              ("launches, plain", 4, dict(chained=0, coarse_batch_px=0, typed_loads=0, stream_bytes=NO_STREAM))]
SCHEDULES = [(0, 0), (1, 1), (2, 2), (2, 0)]   # (first_level, last_level): one step on one level each, and one per level down the pyramid


def want_of(st, pose, tr):
    """(pose bytes, status, iterations, n_valid, error bits) of a pair from tests/seeded_ref.py's (status, pose, trace), as uwt_stats
    defines the fields.  status OK: the last evaluation's.  NO_VALID_POINTS — the loop stopped at an evaluation without a valid point:
    the pose is the one in front of that evaluation (the seed, or what the levels before made of it), `iterations` ("residual
    evaluations over all levels") counts that evaluation too, `n_valid` ("of the last evaluation") is 0, and `error`, which that
    evaluation could not form, is the last one formed — 0 where none was."""
    if st == OK:
        return (np.asarray(pose, np.float32).tobytes(),) + SR.stats_of(st, tr)
    assert st == NO_VALID_POINTS
    return (np.asarray(pose, np.float32).tobytes(), st, len(tr) + 1, 0, int(np.float32(tr[-1]["error"]).view(np.uint32)) if tr else 0)


def step_want(O, case, jacobian, first, last):
    key = (MR.current_arith(O), case.name, "step", jacobian, first, last)
    if key not in _want:
        ref, tgt, dep = VC.frames_of(case)
        p = VC.oracle_params(O, case, first_level=first, last_level=last)
        st, pose, tr = SR.align(MR.MetricOracle(O, jacobian == METRIC), p, ref, tgt, dep, seed=case.pose, keep=True)
        _want[key] = want_of(st, pose, tr)
    return _want[key]


def step_differs(pose, s, want):
    """None, or how a pair's pose and uwt_stats differ from want_of's — compared in full whatever the status: a pair that ran out of
    valid points shows the pose it stopped at and the counts want_of states.  A pose of NaNs — a Jacobian of 2^28 x gradient overflows
    the normal equations in the oracle too — must be a pose of NaNs: payloads apart."""
    got = (int(s["status"]), int(s["iterations"]), int(s["n_valid"]), int(np.float32(s["error"]).view(np.uint32)))
    if got != want[1:]:
        return "stats %s against %s" % (got, want[1:])
    w = np.frombuffer(want[0], np.float32)
    return None if VR.same_bits(pose, w, nan_equal=True) else "pose %s against %s" % (pose, w)


@pytest.mark.parametrize("g", geometries(DENSE_NORMAL), ids=geometry_id)
def test_one_step_from_the_designed_pose(capi, O, arith, g):
    """uwt_estimate_pose_batch_seeded with the case's pose as the seed, max_iters = 1 and handoff keep: pose bytes, status, evaluations,
    n_valid and error bits of 1 and 4 pairs in the chained flow, the one-block coarse kernels and the per-evaluation launches equal
    tests/seeded_ref.py's loop over the oracle.  A level without a valid point: NO_VALID_POINTS, the pose in front of that evaluation
    (the seed on the first level) and the counts want_of states, in every launch form."""
    cases = cases_of(g, DENSE_NORMAL)
    ctx = make_ctx(capi, cases[0])
    for first, last in SCHEDULES:
        ctx.update_params(first_level=first, last_level=last)
        for jacobian in (REFERENCE, METRIC):
            for name, n, tuning in STEP_FORMS:
                set_form(ctx, jacobian, tuning)
                slots = np.arange(n, dtype=np.int32)
                for case in cases:
                    want = step_want(O, case, jacobian, first, last)
                    poses, stats = ctx.estimate_pose_batch_seeded(2 * slots, 2 * slots + 1, np.tile(case.pose, (n, 1)), handoff="keep")
                    for k, s in enumerate(stats):
                        assert step_differs(poses[k], s, want) is None, (case.name, first, last, jacobian, name, k, step_differs(poses[k], s, want))
    ctx.close()


# ---- 5. uwt_estimate_pose_points over the same rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", geometries(DENSE_NORMAL), ids=geometry_id)
def test_point_tables_of_the_same_rows(capi, O, arith, g):
    """every level's grid as an explicit table (sentinel rows and all; the entry starts from the identity, where u = col and v = row
    exactly: column 0 and row 0 sit on the bound), and on the 48 x 36 geometry of intrinsics A the table of fractional reference
    positions: pose bytes and stats equal the loop over the oracle in both Jacobian modes"""
    case = cases_of(g, DENSE_NORMAL)[0]
    ctx = make_ctx(capi, case)
    ref, tgt, dep = VC.frames_of(case)
    jobs = [(2, 0, {lvl: VC.level_inputs(O, case, lvl)[5] for lvl in range(VC.N_LEVELS)})]
    if g == geometry(VC.BY_NAME["table_fraction"]):
        jobs.append((0, 0, {0: VC.BY_NAME["table_fraction"].table}))
    for first, last, tables in jobs:
        ctx.update_params(first_level=first, last_level=last)
        p = VC.oracle_params(O, case, first_level=first, last_level=last)
        for jacobian in (REFERENCE, METRIC):
            want = want_of(*SR.align(MR.MetricOracle(O, jacobian == METRIC), p, ref, tgt, dep, tables=tables))
            set_form(ctx, jacobian, {})
            pose, st = ctx.estimate_pose_points(0, 1, tables)
            assert step_differs(pose, st, want) is None, (g, first, jacobian, step_differs(pose, st, want))
    ctx.close()


# ---- 6. the image warp and the cloud at the flips and the tz cases -------------------------------------------------------------------------
MOVED = [c for c in DENSE_NORMAL if c.name.startswith(("flip_", "tz_"))]


@pytest.mark.parametrize("g", geometries(MOVED), ids=geometry_id)
def test_image_warp_and_cloud(capi, O, arith, g):
    """uwt_warp_image_batch on levels 0 and 2 (rows with z2 == 0 are skipped as not finite, rows behind the camera land where the
    reference puts them) and uwt_point_cloud_batch in world mode, against tests/warp_image_ref.py and tests/cloud_ref.py"""
    cases = cases_of(g, MOVED)
    ctx = make_ctx(capi, cases[0])
    ref, tgt, dep = VC.frames_of(cases[0])
    p = VC.oracle_params(O, cases[0])
    poses = np.stack([c.pose for c in cases])
    for lvl in (0, 2):
        r = ctx.warp_image_batch([0] * len(cases), [1] * len(cases), poses, lvl=lvl)
        assert r["status"] == OK
        for i, case in enumerate(cases):
            L, i1, i2, _, _, _ = VC.level_inputs(O, case, lvl)
            want = WR.dense_reference(O, p, lvl, i1, i2, O.pyramid(dep, VC.N_LEVELS)[lvl] if dep is not None else None, case.pose)
            assert tuple(int(r["quality"][i][k]) for k in WR.QUALITY_FIELDS) == tuple(want["quality"][k] for k in WR.QUALITY_FIELDS), (case.name, lvl)
            for k in ("warped", "valid", "absdiff"):
                assert r[k][i].tobytes() == want[k].tobytes(), (case.name, lvl, k)
    L, i1, _, _, _, pts = VC.level_inputs(O, cases[0], 0)
    for skip in (0, 1):
        want = CR.batch_cloud(O, [(pts, c.pose, i1) for c in cases], L, arith, 1, 1, skip)
        r = ctx.point_cloud_batch([0] * len(cases), poses, capi.default_cloud_params(mode=1, stride=1, skip_invalid=skip))
        assert r["status"] == OK
        assert [tuple(int(x[k]) for k in CR.INFO_FIELDS) for x in r["info"]] == want[1]
        assert r["points"].tobytes() == want[0].tobytes(), skip
    ctx.close()


# ---- 7. the range cases: at and beyond the ends of the dense warp's domain --------------------------------------------------------------------
def entry_report(capi, ctx, O, case):
    """what differs between the device and the oracle through uwt_warp and the per-stage entry, as lines of text"""
    report = []
    for lvl in range(VC.N_LEVELS):
        L, _, _, _, _, pts = VC.level_inputs(O, case, lvl)
        want = O.warp(pts, case.pose, L)
        got = ctx.warp(lvl, pts, case.pose)
        if not VR.same_bits(got, want, nan_equal=True):
            bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
            report.append("level %d uwt_warp: %d of %d rows; row %d: device %s, oracle %s" % (lvl, len(bad), len(pts), bad[0], got[bad[0]], want[bad[0]]))
        for jacobian in (REFERENCE, METRIC):
            set_form(ctx, jacobian, {})
            J, r, idx, n = expected(O, case, lvl, "unit", 0, jacobian)
            d = terms_differ(ctx.residual_jacobian(0, 1, lvl, case.pose), J, r, idx, n)
            if d:
                report.append("level %d entry, Jacobian mode %d: %s" % (lvl, jacobian, d))
    return report


@pytest.mark.parametrize("case", DENSE_RANGE, ids=lambda c: c.name)
def test_range_cases(capi, O, arith, case):
    """Just inside the bounds of include/uwt.h ("the dense warp's division") the device equals the oracle bit for bit through uwt_warp, the
    per-stage entry and a seeded step; just outside, and at the far values, uwt_create refuses the depth_scale and a seeded call
    refuses the pair — that pair alone: its neighbour's bits are what they are without it.  What the per-stage entry, which takes its
    pose as given, returns out there is printed next to the oracle's (profiles/r30/README.md), not asserted."""
    refusal = VC.refusal(case)
    if refusal == "create":
        with pytest.raises(capi.UwtError) as e:
            make_ctx(capi, case, planes=False)
        assert e.value.status == INVALID_ARG
        return
    ctx = make_ctx(capi, case)
    report = entry_report(capi, ctx, O, case)
    print("RANGE %s %s (%s): %s" % (case.range_tag, arith, refusal or "inside", "equal" if not report else "; ".join(report)))
    near = VC.BY_NAME["half_px_pos"].pose
    want_near = step_want(O, VC.BY_NAME["half_px_pos"], REFERENCE, 2, 0) if geometry(case) == geometry(VC.BY_NAME["half_px_pos"]) else None
    set_form(ctx, REFERENCE, {})
    for n, tuning in ((2, dict(chained=1)), (4, dict(chained=1)), (4, dict(chained=0))):
        set_form(ctx, REFERENCE, tuning)
        slots = np.arange(n, dtype=np.int32)
        seeds = np.tile(near, (n, 1))
        seeds[0] = case.pose
        poses, stats = ctx.estimate_pose_batch_seeded(2 * slots, 2 * slots + 1, seeds, handoff="keep")
        if refusal == "seed":
            s0 = stats[0]
            assert (poses[0].tobytes(), s0["status"], s0["iterations"], s0["n_valid"], s0["error"]) == (SR.IDENTITY.tobytes(), INVALID_ARG, 0, 0, 0), (case.name, n, tuning)
        else:
            assert not report, report
            assert step_differs(poses[0], stats[0], step_want(O, case, REFERENCE, 2, 0)) is None, (case.name, n, tuning)
        if want_near is not None:
            assert all(step_differs(poses[k], stats[k], want_near) is None for k in range(1, n)), (case.name, n, tuning)
    ctx.close()
