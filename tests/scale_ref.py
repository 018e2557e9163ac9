"""The robust scale stage restated plainly: Python loops over numpy scalars, nothing shared with oracle/uwt_oracle.c or the kernels.

The contract (uw-slam_amd/csrc/uwt_kernels.h "Scale from the signed residual histogram alone", include/uwt.h uwt_weights):
  median  Tracker::MedianMat, src/Tracker.cpp:1571-1594: the values rounded (cvRound, half to even); under the reference Tukey
          saturated to [0, 255] first (:1572-1573), under Huber kept signed; the smallest value whose cumulative count
          exceeds (float)(n / 2)  (:1575-1591: "bin > m" on a float m of an integer division);
  MAD     Tracker::MedianAbsoluteDeviation, :1607-1619: the same median of |q - med| over the signed values, which the u8
          conversion of :1613 clamps at 255 (Tukey); the Huber extension clamps at 510; times 1.4826f;
  weights Tracker::TukeyFunctionWeights, :1626-1654 (MAD 0 -> 1, :1634-1637; b = 4.6851); Huber k = 1.345 (extension);
  sums    the weighted residual (r * gain) * w of :559-561 and the error term r * (r * w) of :499-502.
No valid pixel: the reference would divide by zero further on; the project's rule is MAD = 1 and no median (None)."""
import numpy as np

F = np.float32
D = np.float64
TUKEY, HUBER = 1, 2
C_MAD = F(1.4826)
TUKEY_B = F(4.6851)
HUBER_K = F(1.345)
DEV_CLAMP = {TUKEY: 255, HUBER: 510}


def first_exceeding(counts, n):
    """The smallest value of {value: count} whose cumulative count exceeds float32(n // 2); None if none does."""
    m = F(n // 2)
    cum = 0
    for v in sorted(counts):
        cum += counts[v]
        if F(cum) > m:
            return v
    return None


def counted(values, lo, hi, counts=None):
    """{value clamped to [lo, hi]: count}"""
    out = {}
    for i, v in enumerate(values):
        v = min(max(int(v), lo), hi)
        out[v] = out.get(v, 0) + (1 if counts is None else int(counts[i]))
    return out


def scale(r, kind):
    """(med, dmed, mad, inv_mad, n) of the residuals r under TUKEY or HUBER."""
    q = np.sort(np.rint(np.asarray(r, F).reshape(-1))).astype(np.int64)
    n = int(q.size)
    if n == 0:
        return None, None, F(1), F(1), 0
    vals, cnts = np.unique(q, return_counts=True)       # the sorted values, run-length coded
    med = first_exceeding(counted(vals, 0 if kind == TUKEY else -255, 255, cnts), n)
    dmed = first_exceeding(counted([abs(int(v) - med) for v in vals], 0, DEV_CLAMP[kind], cnts), n)
    mad = C_MAD * F(dmed)
    if mad == F(0):
        mad = F(1)
    inv_mad = F(D(1.0) / D(mad))
    return med, dmed, mad, inv_mad, n


def tukey_weight(r, inv_mad):
    b = TUKEY_B
    inv_b2 = F(D(1.0) / D(b * b))
    x = F(r) * F(inv_mad)
    if abs(x) <= b:
        t = F(D(1.0) - D((x * x) * inv_b2))
        return t * t
    return F(0)


def huber_weight(r, inv_mad):
    ax = abs(F(r) * F(inv_mad))
    return F(1) if ax <= HUBER_K else HUBER_K / ax


def weight(kind, r, inv_mad):
    return tukey_weight(r, inv_mad) if kind == TUKEY else huber_weight(r, inv_mad)


def weights(kind, r, inv_mad):
    """weight() of every element; each distinct residual value is evaluated once"""
    r = np.asarray(r, F).reshape(-1)
    memo = {}
    out = np.empty(r.size, F)
    for i, x in enumerate(r):
        k = x.tobytes()
        if k not in memo:
            memo[k] = weight(kind, x, inv_mad)
        out[i] = memo[k]
    return out


def weighted_terms(r, w, gain):
    """((r * gain) * w as f32, f64(r) * f64(r * w)): what a pixel adds to J^T r (times its Jacobian row) and to the error numerator"""
    r, w, gain = F(r), F(w), F(gain)
    return (r * gain) * w, D(r) * D(r * w)
