"""Constructed descriptor sets for the matching tests, each with the outputs the contract of include/uwt.h gives, written out by
hand: (name, A, B, ratio, forward 2-NN records (idx0, idx1, d0, d1), matches (query_idx, train_idx, distance)).  A helper module of
tests/test_match_ref_cpu.py and tests/test_gpu_match.py (not a test, not a conftest)."""
import numpy as np


def _f(rows):
    return np.array(rows, np.float32).reshape(len(rows), -1)


def _axis(xs, dim=4):
    """points on the first axis of a dim-dimensional space"""
    a = np.zeros((len(xs), dim), np.float32)
    a[:, 0] = xs
    return a


CASES = [
    # duplicate train rows: ties at the best (rows 0, 1 at distance 1) and at the second (rows 2, 3 at distance 5); lowest index wins.
    # Backward: every train row has A0 and A1 at a ratio above 0.65 or points at A0; only (0, 0) is symmetric and survives:
    # B0 -> A0 at 1, A1 at 49: 1 / 49 survives and points back.  Forward row 0: 1 / 1 = 1 > 0.65: dropped.  No match.
    ("duplicate_train_rows", _axis([0, 50]), _axis([1, 1, 5, 5]), 0.65,
     [(0, 1, 1.0, 1.0), (2, 3, 45.0, 45.0)], []),
    # a query row equal to two train rows: d0 = d1 = 0, 0 / 0 is NaN, the row survives; B0 -> A0 at 0, A1 at 10: survives, points back.
    # A1 = (10, 0): B2 = (10, 4) at 4, B0 at 10 (tie with B1: lowest): 0.4 survives; B2 -> A1 at 4, A0 at sqrt(116): survives, back.
    ("query_equals_two_train_rows", _f([[0, 0, 0, 0], [10, 0, 0, 0]]), _f([[0, 0, 0, 0], [0, 0, 0, 0], [10, 4, 0, 0]]), 0.65,
     [(0, 1, 0.0, 0.0), (2, 0, 4.0, 10.0)], [(0, 0, 0.0), (1, 2, 4.0)]),
    # d0 / d1 exactly on the ratio: 1 / 2 = 0.5 is not > 0.5, the row survives.  A1 = 100: B1 at 98, B0 at 99: dropped.
    # B0 = 1 -> A0 at 1, A1 at 99: survives, points back.
    ("exactly_on_the_ratio", _axis([0, 100]), _axis([1, 2]), 0.5,
     [(0, 1, 1.0, 2.0), (1, 0, 98.0, 99.0)], [(0, 0, 1.0)]),
    # the same sets a hair below: 0.5 > 0.49999997 and row 0 goes too
    ("just_below_the_ratio", _axis([0, 100]), _axis([1, 2]), float(np.nextafter(np.float32(0.5), np.float32(0))),
     [(0, 1, 1.0, 2.0), (1, 0, 98.0, 99.0)], []),
    # all descriptors identical: every distance 0, every row's neighbours are rows 0 and 1, every row survives (NaN); every forward
    # row points at B0, which points back at A0 alone
    ("all_identical", np.full((5, 8), 0.25, np.float32), np.full((4, 8), 0.25, np.float32), 0.65,
     [(0, 1, 0.0, 0.0)] * 5, [(0, 0, 0.0)]),
    # asymmetric: A1 = 3 -> B0 = 1 (2 against 97), but B0 -> A0 = 0 (1 against 2: 0.5 survives); the symmetry test drops row 1.
    # B1 = 100 -> A1 at 97, A0 at 100: 0.97 dropped.
    ("asymmetric_pair", _axis([0, 3]), _axis([1, 100]), 0.65,
     [(0, 1, 1.0, 100.0), (0, 1, 2.0, 97.0)], [(0, 0, 1.0)]),
    # one train row: idx0 / d0 are reported, there is no second neighbour, nothing survives
    ("single_train_row", _axis([0, 3, 7]), _axis([4]), 0.65,
     [(0, -1, 4.0, 0.0), (0, -1, 1.0, 0.0), (0, -1, 3.0, 0.0)], []),
    # Hamming, duplicate train rows: A0 = 00 00 00 00; B0 = B1 = 01 00 00 00 (1 bit), B2 = ff 0f 00 00 (12 bits).  1 / 1 dropped.
    # A1 = ff ff 00 00: B2 at 4 bits, B0 at 15 (tie with B1): 4 / 15 survives; B2 -> A1 at 4, A0 at 12: survives, points back.
    ("hamming_duplicates", np.array([[0, 0, 0, 0], [255, 255, 0, 0]], np.uint8),
     np.array([[1, 0, 0, 0], [1, 0, 0, 0], [255, 15, 0, 0]], np.uint8), 0.65,
     [(0, 1, 1.0, 1.0), (2, 0, 4.0, 15.0)], [(1, 2, 4.0)]),
]
