"""Plain restatement of the scalar tail of one Gauss-Newton iteration (uw-slam_amd/csrc/uwt_kernels.h: update_compute /
tail_fold_wave -> update_solve_wave), for the tests of uwt_gn_update_records.  Python loops over numpy scalars, nothing vectorised:
every addition is written where the kernels do it.

A record (kRecWords = 64 words, block_reduce_store_at): 32 eight-byte slots.
  slots 0..26   f64: the 21 upper-triangle sums of J^T J (row-major), then the 6 of J^T r
  slot 27       valid points: u32 in the LOW word (word 54); the high word (55) is not part of it
  slot 28       sum of r^2: a 64-bit integer (words 56-57)
  slot 29       f64: the error numerator of the general kind's records (words 58-59)
  slots 30, 31  not sums (words 60, 61 carry clock probes): read by the fold's lanes 30 / 31 and ignored
The fold: part p = records p, p + 8, p + 16, ... in increasing order, each part from +0.0 / 0; then parts 0..7 in part order, part 0's sum
first.  Integer slots alike in 64-bit two's complement; the valid count goes through uint32 once at the end, then through int.
"""
import numpy as np

REC_WORDS = 64
N_SUMS = 27
STATE_DTYPE = np.dtype([("pose", "<f4", (7,)), ("last_error", "<f4"), ("error", "<f4"), ("level_done", "<i4"), ("status", "<i4"),
                        ("iters", "<i4"), ("n_valid", "<i4")])
F32_EPS10 = np.float32(1.1920929e-07) * np.float32(10)   # the pivot threshold of cv's LU: FLT_EPSILON * 10, an f32 product


def make_record(sums, n_valid=0, sum_r2=0, err_num=0.0, word55=0, tail_words=(0, 0, 0, 0)):
    """64 uint32 words from 27 f64 sums, the two integer counts, the error numerator, word 55 and words 60..63"""
    rec = np.zeros(REC_WORDS, np.uint32)
    f = rec.view(np.float64)
    for i in range(N_SUMS):
        f[i] = np.float64(sums[i])
    rec[54] = np.uint32(int(n_valid) & 0xffffffff)
    rec[55] = np.uint32(int(word55) & 0xffffffff)
    rec.view(np.uint64)[28] = np.uint64(int(sum_r2) & 0xffffffffffffffff)
    f[29] = np.float64(err_num)
    for i in range(4):
        rec[60 + i] = np.uint32(int(tail_words[i]) & 0xffffffff)
    return rec


def state(pose=(0, 0, 0, 1, 0, 0, 0), last_error=50000.0, error=0.0, level_done=0, status=0, iters=0, n_valid=0):
    s = np.zeros((), STATE_DTYPE)
    s["pose"] = np.asarray(pose, np.float32)
    s["last_error"], s["error"] = np.float32(last_error), np.float32(error)
    s["level_done"], s["status"], s["iters"], s["n_valid"] = level_done, status, iters, n_valid
    return s


# ---------------------------------------------------------------- the fold

def fold_values(vals, order="parts"):
    """One f64 slot over its records' values.  order: "parts" (the kernels'), "sequential" (record order), "swap12" (parts 1 and 2
    exchanged in the final pass) or "reversed" (the final pass from part 7 down) — the last three exist so that tests can show their
    inputs tell the orders apart.  Up to 8 records every part holds one record and "parts" IS the record order."""
    vals = [np.float64(v) for v in vals]
    if order == "sequential":
        s = np.float64(0.0)
        for v in vals:
            s = s + v
        return s
    parts = []
    for p in range(8):
        cs = np.float64(0.0)
        q = p
        while q < len(vals):
            cs = cs + vals[q]
            q += 8
        parts.append(cs)
    seq = {"swap12": [0, 2, 1, 3, 4, 5, 6, 7], "reversed": list(range(7, -1, -1))}.get(order, list(range(8)))
    s = parts[seq[0]]
    for p in seq[1:]:
        s = s + parts[p]
    return s


def _wrap64(v):
    v &= 0xffffffffffffffff
    return v - (1 << 64) if v >> 63 else v


def fold_ints(vals):
    """An integer slot: 64-bit two's-complement additions in the same order"""
    parts = []
    for p in range(8):
        s = 0
        q = p
        while q < len(vals):
            s = _wrap64(s + _wrap64(int(vals[q])))
            q += 8
        parts.append(s)
    s = parts[0]
    for p in range(1, 8):
        s = _wrap64(s + parts[p])
    return s


def fold(records, count, general, order="parts"):
    """records: (>= count) x 64 words.  Returns (sums[27] f64, err_num f64, n as the kernels' int, sum_r2 as their long long)."""
    recs = np.ascontiguousarray(records, np.uint32).reshape(-1, REC_WORDS)[:count]
    f = recs.view(np.float64)      # count x 32
    u = recs.view(np.uint64)
    sums = [fold_values([f[q, i] for q in range(count)], order) for i in range(N_SUMS)]
    err_num = fold_values([f[q, 29] for q in range(count)], order) if general else np.float64(0.0)
    n64 = fold_ints([int(u[q, 27]) & 0xffffffff for q in range(count)])    # the low word only
    n = n64 & 0xffffffff                                                    # (uint32_t)
    n = n - (1 << 32) if n >> 31 else n                                     # (int)
    sr2 = fold_ints([int(u[q, 28]) for q in range(count)])
    return sums, err_num, n, sr2


# ---------------------------------------------------------------- the solve, spelled out (what the oracle's LU does, column by column)

def symmetric_from_sums(sums):
    """A = (float) of the 21 upper-triangle sums, mirrored"""
    A = np.zeros((6, 6), np.float32)
    q = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = np.float32(sums[q])
            A[j, i] = A[i, j]
            q += 1
    return A


def upper_triangle(A):
    return [np.float64(A[i][j]) for i in range(6) for j in range(i, 6)]


def lu_trace(A):
    """The elimination of cv::hal::LU32f on A alone, f32: per column (chosen row, rows that attain the column's largest magnitude, pivot).
    Stops behind the column whose pivot is below the threshold.  Returns (trace, singular_at or None)."""
    A = np.array(A, np.float32).reshape(6, 6).copy()
    trace = []
    for i in range(6):
        k = i
        for j in range(i + 1, 6):
            if abs(A[j, i]) > abs(A[k, i]):
                k = j
        ties = sum(1 for j in range(i, 6) if abs(A[j, i]) == abs(A[k, i]))
        trace.append((k, ties, A[k, i]))
        if abs(A[k, i]) < F32_EPS10:
            return trace, i
        if k != i:
            A[[i, k], i:] = A[[k, i], i:]
        d = np.float32(-1.0) / A[i, i]
        for j in range(i + 1, 6):
            alpha = A[j, i] * d
            for q in range(i + 1, 6):
                A[j, q] = A[j, q] + alpha * A[i, q]
    return trace, None


def solve(O, A, b, arith):
    """deltaMat = A.inv() * b under the arithmetic set: cv::solve's LU on b (opencv), or the inverse formed and multiplied in f64 (legacy)"""
    if arith == "legacy":
        X, _ = O.inv6(A)
        d = np.zeros(6, np.float32)
        for i in range(6):
            s = np.float64(0.0)
            for j in range(6):
                s = s + np.float64(X[i, j]) * np.float64(b[j])
            d[i] = np.float32(s)
        return d
    return O.solve6(A, b)[0]


# ---------------------------------------------------------------- update_solve_wave, line by line

def update(O, st, records, count, k, max_iters, early_exit, epsilon, gain, general, arith, block_form=False, order="parts"):
    """The pair's next state and whether it took a step.  block_form: k_gn_update returns a finished pair unchanged."""
    st = st.copy()
    if block_form and (st["level_done"] or st["status"]):
        return st, False
    sums, err_num, n, sr2 = fold(records, count, general, order)
    epsilon, gain = np.float32(epsilon), np.float32(gain)
    st["iters"] = st["iters"] + 1
    st["n_valid"] = n
    step = True
    with np.errstate(all="ignore"):
        if n == 0:
            st["status"] = 2
            st["level_done"] = 1
            step = False
        else:
            inv_n = np.float32(np.float64(1.0) / np.float64(n))
            if general:
                error = np.float32(np.float64(inv_n) * err_num)
            else:
                error = np.float32(np.float64(inv_n) * np.float64(sr2))
            st["error"] = error
            last = np.float32(st["last_error"])
            if early_exit and (error >= last or k == max_iters - 1 or np.abs(np.float32(error - last)) < epsilon):
                st["level_done"] = 1
                step = False
            else:
                st["last_error"] = error
        if step:
            b = np.zeros(6, np.float32)
            for i in range(6):
                b[i] = np.float32(-sums[21 + i]) if general else np.float32(-(np.float64(gain) * sums[21 + i]))
            A = symmetric_from_sums(sums)
            delta = solve(O, A, b, arith)
            d = O.se3_exp(delta)
            st["pose"] = O.se3_mul(np.array(st["pose"], np.float32), d)
    return st, step
