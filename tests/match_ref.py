"""The restatement, in numpy, of the descriptor-matching contract of include/uwt.h (uwt_knn_match_batch,
uwt_match_descriptors_batch) and nothing else: distances, 2-NN with lowest-index ties, ratio test, symmetry test.  A helper module
of the matching tests and of nothing else (not a test, not a conftest).

    L2        s = 0; for k: d = a[k] - b[k]; s = s + d * d   (f32, in that order, no FMA: numpy's f32 ufuncs round every step)
              dist = sqrt(s) (f32, correctly rounded)
    Hamming   popcount(a ^ b) as a float
"""
import numpy as np

KNN2 = np.dtype([("idx0", "<i4"), ("idx1", "<i4"), ("d0", "<f4"), ("d1", "<f4")])
MATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint16)


def distances(A, B, f64=False):
    """[n, m] distances of every row of A to every row of B; dtype decides the norm (float32: L2, uint8: Hamming).  f64: the L2
    distances evaluated in double (the yardstick the f32 order is compared with), not rounded to float."""
    A, B = np.asarray(A), np.asarray(B)
    n, m = A.shape[0], B.shape[0]
    if A.dtype == np.uint8:
        s = np.zeros((n, m), np.uint16)
        for k in range(A.shape[1]):
            s += _POPCOUNT[A[:, k, None] ^ B[None, :, k]]
        return s.astype(np.float64 if f64 else np.float32)
    t = np.float64 if f64 else np.float32
    A, B = A.astype(t), B.astype(t)
    s = np.zeros((n, m), t)
    for k in range(A.shape[1]):
        d = A[:, k, None] - B[None, :, k]
        s = s + d * d
    return np.sqrt(s)


def knn2_of(D):
    """knnMatch(.., 2) on a distance matrix: per row the nearest and the second nearest column, ties to the lowest index (argmin
    returns the first minimum).  A missing neighbour is idx = -1, d = 0."""
    n, m = D.shape
    out = np.zeros(n, KNN2)
    out["idx0"] = out["idx1"] = -1
    if n == 0 or m == 0:
        return out
    rows = np.arange(n)
    best = np.argmin(D, axis=1)
    out["idx0"], out["d0"] = best, D[rows, best]
    if m >= 2:
        rest = D.astype(np.float64, copy=True)
        rest[rows, best] = np.inf
        second = np.argmin(rest, axis=1)
        out["idx1"], out["d1"] = second, D[rows, second]
    return out


def knn2(A, B, f64=False):
    return knn2_of(distances(A, B, f64))


def survives(knn, ratio):
    """ratioTest: two neighbours and !(d0 / d1 > ratio), an f32 division; 0 / 0 is NaN and survives"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = knn["d0"].astype(np.float32) / knn["d1"].astype(np.float32)
    return (knn["idx1"] >= 0) & ~(q > np.float32(ratio))


def symmetric(fwd, bwd, ratio):
    """symmetryTest as the contract states it: (i, j, d0) for every surviving forward row i with idx0 = j whose backward row j
    survives with idx0 = i, ascending i"""
    sf, sb = survives(fwd, ratio), survives(bwd, ratio)
    out = []
    for i in np.nonzero(sf)[0]:
        j = int(fwd["idx0"][i])
        if sb[j] and bwd["idx0"][j] == i:
            out.append((i, j, fwd["d0"][i]))
    return np.array(out, MATCH)


def match(A, B, ratio=0.65, f64=False):
    """Returns (matches, forward records, backward records)."""
    D = distances(A, B, f64)
    fwd, bwd = knn2_of(D), knn2_of(np.ascontiguousarray(D.T))
    return symmetric(fwd, bwd, ratio), fwd, bwd
