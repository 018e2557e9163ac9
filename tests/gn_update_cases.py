"""The inputs of the Gauss-Newton update tests (tests/test_gn_update_cpu.py shows on the CPU that they can tell a wrong kernel from a
right one, tests/test_gpu_gn_update.py feeds them to uwt_gn_update_records): records for the fold, matrices for the solve, twists for
the exponential.  Everything is generated from fixed seeds; nothing here depends on the arithmetic set."""
import numpy as np

import gn_update_ref as R

FOLD_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 150, 160]
NAN_WORD = 0x7ff80000   # both words of a record past `count`: a NaN in every f64 slot, huge in every integer one


def fold_slot_values(rng, count):
    """`count` values of one slot: (count - 1) // 2 pairs +v, -v with |v| in [2^8, 2^60) at shuffled places — whatever order adds them, the
    sum that comes out is the rounding the order left behind, about 2^7 — and one or two values in [1, 2^8) that do not cancel."""
    n_pairs = (count - 1) // 2
    vals = []
    for _ in range(n_pairs):
        v = np.ldexp(1.0 + rng.random(), int(rng.integers(8, 60)))
        vals += [v, -v]
    for _ in range(count - 2 * n_pairs):
        vals.append(np.ldexp(1.0 + rng.random(), int(rng.integers(0, 8))) * (1.0 if rng.random() < 0.5 else -1.0))
    return [vals[i] for i in rng.permutation(count)]


def fold_records(count, seed=0, hostile=0):
    """count x 64 words.  Slots 0..26 and 29 by fold_slot_values; small counts.  hostile 1 / 2: word 55 of every record all ones, words
    60..63 random, the sum of r^2 past 2^53, the valid counts summing into (2^31, 2^32) (1) or past 2^32 (2)."""
    rng = np.random.default_rng(1000 * count + seed)
    cols = [fold_slot_values(rng, count) for _ in range(R.N_SUMS + 1)]
    total_n = {0: None, 1: 3 << 30, 2: (1 << 32) + 12345}[hostile]
    recs = np.zeros((count, R.REC_WORDS), np.uint32)
    r2s = [((1 << 53) + (1 << 52)) // count + 2 * int(rng.integers(0, 1 << 20)) for _ in range(count)]
    r2s[0] += 1 - sum(r2s) % 2   # an odd total past 2^53: no double holds it
    for q in range(count):
        if hostile:
            n = total_n // count + (total_n % count if q == 0 else 0)
            recs[q] = R.make_record([c[q] for c in cols[:R.N_SUMS]], n, r2s[q], cols[R.N_SUMS][q], 0xffffffff, rng.integers(0, 1 << 32, 4))
        else:
            recs[q] = R.make_record([c[q] for c in cols[:R.N_SUMS]], int(rng.integers(1, 1000)), int(rng.integers(0, 1 << 40)), cols[R.N_SUMS][q])
    return recs


def pad_records(recs, stride, fill=NAN_WORD):
    """count x 64 -> stride x 64, the records past the count filled with `fill`"""
    out = np.full((stride, R.REC_WORDS), fill, np.uint32)
    out[:len(recs)] = recs
    return out


# ---------------------------------------------------------------- one system (A, jtr) as records

SPLIT9 = [1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128, 1 / 256, 1 / 256]   # dyadic: v * w adds back to v exactly, in any order


def system_records(A, jtr, n_valid=100, sum_r2=123456, err_num=0.0, split=False):
    """The records of one evaluation whose fold is exactly (A's upper triangle, jtr): one record, or nine whose parts add exactly"""
    sums = R.upper_triangle(np.asarray(A, np.float64)) + [np.float64(v) for v in jtr]
    if not split:
        return R.make_record(sums, n_valid, sum_r2, err_num).reshape(1, -1)
    recs = np.zeros((9, R.REC_WORDS), np.uint32)
    for q, w in enumerate(SPLIT9):
        r2 = {2: sum_r2 // 2, 7: sum_r2 - sum_r2 // 2}.get(q, 0)
        recs[q] = R.make_record([s * w for s in sums], n_valid if q == 4 else 0, r2, err_num * w)
    return recs


# ---------------------------------------------------------------- matrices for the solve

def rank_deficient(i):
    """Symmetric, exact small integers, rank i, leading i x i block diag(4, 2, 8, 1, 16)[:i]: [[B, BC], [C'B, C'BC]] with C in {0, +-1}.
    Every multiplier of the elimination is 0 or +-1 and every pivot a power of two, so f32 eliminates exactly: the first tiny pivot is
    column i's, an exact zero."""
    B = np.diag([4.0, 2.0, 8.0, 1.0, 16.0][:i])
    rng = np.random.default_rng(40 + i)
    Cm = rng.integers(-1, 2, (i, 6 - i)).astype(np.float64)
    A = np.zeros((6, 6))
    A[:i, :i] = B
    A[:i, i:] = B @ Cm
    A[i:, :i] = (B @ Cm).T
    A[i:, i:] = Cm.T @ B @ Cm
    return A.astype(np.float32)


TIES = np.array([[-2, -2, -1, -2, 1, 1], [-2, 1, 1, 1, -1, 2], [-1, 1, -2, 1, 2, 1], [-2, 1, 1, 2, -2, 2], [1, -1, 2, -2, -2, -2],
                 [1, 2, 1, 2, -2, -1]], np.float32)     # two or three rows share the largest magnitude in every column 0..4
SWAPS = np.array([[-1, 1, -1, 2, -1, 1], [1, 2, -2, 1, -2, -2], [-1, -2, -1, 2, -2, 1], [2, 1, 2, 1, 2, -1], [-1, -2, -2, 2, 2, 1],
                  [1, -2, 1, -1, 1, 2]], np.float32)    # the pivot row is never the diagonal's in columns 0..4
EPS10 = R.F32_EPS10


def threshold_matrix(pos, below):
    """identity with 10 * FLT_EPSILON (below: the float under it) on the diagonal at `pos`"""
    A = np.eye(6, dtype=np.float32)
    A[pos, pos] = np.nextafter(EPS10, np.float32(0)) if below else EPS10
    return A


def jtj_like(seed):
    """J'J of 60 rows whose translation columns are 1000 x the rotation columns': the translation block 10^6 x the rotation block"""
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 1, (60, 6)) * np.array([1e3, 1e3, 1e3, 1, 1, 1])
    r = rng.normal(0, 5, 60)
    return (J.T @ J).astype(np.float32), (J.T @ r).astype(np.float32)


def solve_cases():
    """name -> (A f32 6x6, jtr f32[6], singular_at or None)"""
    rng = np.random.default_rng(7)
    rhs = lambda: rng.integers(-9, 10, 6).astype(np.float32)
    cases = {}
    for i in range(6):
        cases["rank_%d" % i] = (rank_deficient(i), rhs(), i)
    cases["ties"] = (TIES, rhs(), None)
    cases["swaps"] = (SWAPS, rhs(), None)
    for pos in (2, 5):
        cases["threshold_at_%d" % pos] = (threshold_matrix(pos, False), rhs(), None)
        cases["threshold_below_%d" % pos] = (threshold_matrix(pos, True), rhs(), pos)
    for s in (0, 1):
        A, b = jtj_like(90 + s)
        cases["jtj_%d" % s] = (A, b, None)
    return cases


# ---------------------------------------------------------------- twists for the exponential

def theta_of(om):
    om = np.asarray(om, np.float32)
    return np.sqrt(np.float32(om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])


def theta_targets():
    f = np.float32
    out = [f(0.0), f(1e-7)]
    for c in (f(1e-5), f(0.5), f(1.0)):
        out += [np.nextafter(c, f(0)), c, np.nextafter(c, f(2))]
    return out + [f(0.3), f(3.0), f(np.pi), f(2 * np.pi), f(10.0), f(1e4)]


def general_omega(theta, rng):
    """a rotation vector off the axes whose theta, as sqrtf of the f32 sum of squares gives it, is exactly `theta`"""
    if theta == 0:
        return np.zeros(3, np.float32)
    if theta == np.float32(1e4):
        return np.array([3600.0, -4800.0, 8000.0], np.float32)   # 0.36, 0.48, 0.8: every square and partial sum an exact float, |om| = 1e4
    d = rng.normal(0, 1, 3)
    d /= np.linalg.norm(d)
    om = (np.float64(theta) * d).astype(np.float32)
    j = int(np.argmax(np.abs(om)))
    for _ in range(4096):   # theta is monotone in |om[j]| and moves by at most one ulp per ulp of om[j]
        t = theta_of(om)
        if t == theta:
            return om
        om[j] = np.nextafter(om[j], np.float32(np.sign(om[j]) * (np.inf if t < theta else 0.0)))
    raise AssertionError("no rotation vector with theta %r" % theta)


UPSILONS = [(0.0, 0.0, 0.0), (1e-3, -2e-3, 5e-4), (1.0, -2.0, 3.0), (1e3, -1e3, 500.0)]
# prior poses: the identity, a quaternion whose squared norm is exactly 1 in f32, and one (unit to rounding) where it is not
UNIT_POSES = [(0, 0, 0, 1, 0, 0, 0), (0.5, -0.5, 0.5, 0.5, 1.0, -2.0, 0.25)]
OFF_UNIT_POSE = tuple(np.concatenate([(np.array([0.3, -0.2, 0.1, 0.9]) / np.linalg.norm([0.3, -0.2, 0.1, 0.9])).astype(np.float32),
                                      np.array([0.1, 0.2, -0.3], np.float32)]))
PRIOR_POSES = UNIT_POSES + [OFF_UNIT_POSE]


def exp_cases():
    """[(name, xi f32[6], prior pose)]: every theta target on each axis and along two general directions, translations and prior poses
    taken in turn"""
    rng = np.random.default_rng(11)
    out = []
    n = 0
    for ti, theta in enumerate(theta_targets()):
        for kind in range(5):
            if kind < 3:
                om = np.zeros(3, np.float32)
                om[kind] = theta if (ti + kind) % 2 == 0 else -theta
            else:
                om = general_omega(theta, rng)
            assert theta_of(om) == theta, (theta, om)
            xi = np.concatenate([np.array(UPSILONS[n % 4], np.float32), om])
            out.append(("theta_%d_%s" % (ti, "xyzgh"[kind]), xi, np.array(PRIOR_POSES[n % 3], np.float32)))
            n += 1
    return out
