"""Plain restatement of the sums k_table_eval forms under accumulate_f64 = 0 (uw-slam_amd/csrc/uwt_kernels.h: k_table_eval,
accumulate(float ..), block_reduce_store_at), for tests/test_gpu_instantiations.py.  A helper of the tests, not a test.

The f32 part of those sums is small and fixed: a block takes 1024 table rows, thread t of block b the rows b * 1024 + r * 256 + t,
r = 0..3, and adds each VALID row's 27 products to its own 27 accumulators with one fused multiply-add each, in f32, from +0.
Everything behind that is f64, in an order this file writes out: a block's 256 values of one sum are added in 8 segments of 32 (thread
8 v + s of a reduction pass starts its segment s at column (8 v + s) & 31 and wraps; v the sum's place in the pass of 14), the 8
segment sums in segment order; the blocks' records fold as gn_update_ref.fold_values does; A and b come out of the 27 sums as in
gn_update_ref.update.  So the f32 form has a restatement as exact as the f64 form's, and is compared bit for bit."""
import numpy as np

import gn_update_ref as GN

ROWS_PER_BLOCK, BLOCK, PASS = 1024, 256, 14
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: a * b + c rounded ONCE.  The product of two f32 is exact in f64; t = RN64(p + c) and the exact
    error e of that addition (TwoSum) say on which side of t the exact value lies.  RN32(t) is RN32(exact) unless t sits exactly half
    way between two f32 and e != 0: then the exact value's neighbour on e's side is the result."""
    a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    t = p + c64
    bb = t - p
    e = (p - (t - bb)) + (c64 - bb)
    f = t.astype(np.float32)
    d = f.astype(np.float64) - t
    other = np.nextafter(f, np.where(d > 0, -np.inf, np.inf).astype(np.float32))
    tie = (d != 0) & (np.abs(other.astype(np.float64) - t) == np.abs(d)) & (e != 0)
    return np.where(tie, np.where(e > 0, np.maximum(f, other), np.minimum(f, other)), f).astype(np.float32)


def thread_sums(J, r, idx, n_rows):
    """[blocks, 256, 27] float32: every thread's accumulators behind its (up to) four rows.  J, r: the valid rows' Jacobian rows and
    residuals; idx: their row numbers in the table of n_rows rows."""
    blocks = max(1, -(-n_rows // ROWS_PER_BLOCK))
    Jt = np.zeros((blocks * ROWS_PER_BLOCK, 6), np.float32)
    rt = np.zeros(blocks * ROWS_PER_BLOCK, np.float32)
    ok = np.zeros(blocks * ROWS_PER_BLOCK, bool)
    Jt[idx], rt[idx], ok[idx] = J, r, True
    Jt, rt, ok = (x.reshape((blocks, ROWS_PER_BLOCK // BLOCK, BLOCK) + x.shape[1:]) for x in (Jt, rt, ok))
    acc = np.zeros((blocks, BLOCK, 27), np.float32)
    for step in range(ROWS_PER_BLOCK // BLOCK):
        Js, rs, oks = Jt[:, step], rt[:, step], ok[:, step]
        for s, (i, j) in enumerate(PAIRS):
            acc[:, :, s] = np.where(oks, fma32(Js[:, :, i], Js[:, :, j], acc[:, :, s]), acc[:, :, s])
        for i in range(6):
            acc[:, :, 21 + i] = np.where(oks, fma32(Js[:, :, i], rs, acc[:, :, 21 + i]), acc[:, :, 21 + i])
    return acc


def block_sum(values, s):
    """one block's f64 value of sum s (0..26) from its 256 threads' f32 values, in block_reduce_store_at's order"""
    v = s % PASS
    total = None
    for seg in range(8):
        start = (8 * v + seg) & 31
        part = np.float64(0.0)
        for j in range(32):
            part = part + np.float64(values[seg * 32 + ((j + start) & 31)])
        total = part if total is None else total + part
    return total


def sums(J, r, idx, n_rows):
    """the 27 f64 sums of one evaluation of one table, as the update reads them"""
    acc = thread_sums(J, r, idx, n_rows)
    return [GN.fold_values([block_sum(acc[b, :, s], s) for b in range(acc.shape[0])]) for s in range(27)]


def normal_equations(J, r, idx, n_rows, gain):
    """(A [6, 6], b [6]) float32 from those sums, as gn_update_ref.update forms them under identity weights"""
    S = sums(J, r, idx, n_rows)
    b = np.array([np.float32(-(np.float64(np.float32(gain)) * S[21 + i])) for i in range(6)], np.float32)
    return GN.symmetric_from_sums(S), b


class F32TableOracle:
    """An oracle (oracle.oracle or metric_ref.MetricOracle) whose normal_equations are k_table_eval's under accumulate_f64 = 0, for
    seeded_ref.align over tables under identity weights: it remembers the row numbers of the evaluation's valid rows"""

    def __init__(self, base):
        self._base = base

    def __getattr__(self, name):
        return getattr(self._base, name)

    def residual_jacobian_ex(self, img1, img2, gx, gy, pts, *rest):
        J, r, idx = self._base.residual_jacobian_ex(img1, img2, gx, gy, pts, *rest)
        self._idx, self._n_rows = np.asarray(idx), len(pts)
        return J, r, idx

    def normal_equations(self, J, r, W, gain):
        assert W is None and len(J) == len(self._idx)
        return normal_equations(J, r, self._idx, self._n_rows, gain)
