"""The restatement of the descriptor-matching contract (tests/match_ref.py) checked on its own, without the library: against a
plain-Python triple loop on tiny sets, against an f64 evaluation of the same distances on the generator's cases, and against the
constructed cases' outputs written out by hand (tests/match_cases.py)."""
import importlib
import struct

import numpy as np
import pytest

import match_cases
import match_ref as R

ARITH_INDEPENDENT = True   # matching has no arithmetic set


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("uw-slam_amd.synth")


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def loop_knn2(A, B):
    """the contract as loops over Python floats rounded to f32 after every operation"""
    out = []
    for a in A:
        d0 = d1 = None
        j0 = j1 = -1
        for j, b in enumerate(B):
            if A.dtype == np.uint8:
                d = float(sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b)))
            else:
                s = 0.0
                for x, y in zip(a, b):
                    e = f32(float(x) - float(y))
                    s = f32(s + f32(e * e))
                d = float(np.sqrt(np.float32(s)))
            if d0 is None or d < d0:
                d1, j1, d0, j0 = d0, j0, d, j
            elif d1 is None or d < d1:
                d1, j1 = d, j
        out.append((j0, j1, d0 or 0.0, d1 or 0.0))
    return np.array(out, R.KNN2) if out else np.zeros(0, R.KNN2)


def loop_match(A, B, ratio):
    fwd, bwd = loop_knn2(A, B), loop_knn2(B, A)
    def keeps(r):
        if r["idx1"] < 0:
            return False
        with np.errstate(divide="ignore", invalid="ignore"):
            return not (np.float32(r["d0"]) / np.float32(r["d1"]) > np.float32(ratio))
    out = []
    for i, r in enumerate(fwd):   # the reference's symmetryTest loops (src/Tracker.cpp:74-102) over the surviving rows
        for j, q in enumerate(bwd):
            if keeps(r) and keeps(q) and r["idx0"] == j and q["idx0"] == i:
                out.append((i, j, r["d0"]))
                break
    return np.array(out, R.MATCH), fwd


@pytest.mark.parametrize("n,m,dim,kind", [(7, 9, 8, "l2"), (12, 5, 4, "l2"), (1, 2, 4, "l2"), (2, 1, 4, "l2"), (0, 3, 4, "l2"), (3, 0, 4, "l2"),
                                          (9, 11, 4, "hamming"), (6, 6, 8, "hamming")])
def test_restatement_equals_the_plain_loops(synth, n, m, dim, kind):
    A, B, _, _ = synth.descriptor_pair(3 + n, n, m, dim, kind, noise=0.2)
    if kind == "hamming" and n and m:   # few bits: many ties
        A &= 3
        B &= 3
    want, want_fwd = loop_match(A, B, 0.8)
    got, fwd, _ = R.match(A, B, 0.8)
    assert fwd.tobytes() == want_fwd.tobytes()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n,m,dim", [(1500, 1400, 64), (500, 500, 128), (2000, 2000, 64)])
def test_f32_order_decides_nothing_on_the_generator_cases(synth, n, m, dim):
    """rows whose best index, second index or survival differ from an f64 evaluation: at most 0.5 % of the query rows"""
    A, B, _, _ = synth.descriptor_pair(7, n, m, dim, "l2")
    m32, f, b = R.match(A, B, 0.65)
    m64, f6, b6 = R.match(A, B, 0.65, f64=True)
    differ = (f["idx0"] != f6["idx0"]) | (f["idx1"] != f6["idx1"]) | (R.survives(f, 0.65) != R.survives(f6, 0.65))
    share = differ.sum() / n
    sf, sb = int(R.survives(f, 0.65).sum()), int(R.survives(b, 0.65).sum())
    print("%d x %d x %d: forward survivors %d, backward %d, symmetric %d; rows differing from f64: %.4f %%"
          % (n, m, dim, sf, sb, len(m32), 100 * share))
    assert share <= 0.005
    # every stage keeps and drops rows
    assert 0 < len(m32) < min(sf, sb) and sf < n and sb < m


def test_hamming_generator_case_exercises_the_tie_rule(synth):
    A, B, _, _ = synth.descriptor_pair(7, 500, 480, 32, "hamming")
    mt, f, _ = R.match(A, B, 0.65)
    ties = int((f["d0"] == f["d1"]).sum())
    print("Hamming 500 x 480 x 32 B: symmetric %d, rows with d0 == d1: %d" % (len(mt), ties))
    assert ties > 0 and 0 < len(mt) < 500
    assert np.all(f["idx0"][f["d0"] == f["d1"]] < f["idx1"][f["d0"] == f["d1"]])   # lowest index first


@pytest.mark.parametrize("case", match_cases.CASES, ids=[c[0] for c in match_cases.CASES])
def test_constructed_cases_give_the_outputs_written_by_hand(case):
    _, A, B, ratio, want_fwd, want = case
    got, fwd, _ = R.match(A, B, ratio)
    assert fwd.tobytes() == np.array(want_fwd, R.KNN2).tobytes(), fwd
    assert got.tobytes() == np.array(want, R.MATCH).tobytes(), got
    loops, _ = loop_match(A, B, ratio)
    assert loops.tobytes() == got.tobytes()
