"""Inputs and integer comparers of the ORB tests (tests/test_orb_ref_cpu.py, tests/test_orb_cpu.py, tests/test_gpu_orb.py): a helper
module, not a test.  Everything is deterministic.  The generators are those of tests/surf_cases.py."""
import numpy as np

import orb_ref as O
import surf_cases as K

texture, blob_image, flat = K.texture, K.blob_image, K.flat
same_keypoints = K.same_keypoints   # key points AS INTEGERS: the record is SURF's

# (x, y, sigma, polarity) on a 256 x 240 frame: small blobs near the centre, where every layer of the pyramid still has its
# candidate band; a blob of sigma b is a FAST corner (the centre against its whole ring) on the layers that see it with sigma < 4.5
BLOBS = [(128, 120, 3.0, 1), (100, 112, 4.0, -1), (156, 126, 3.5, 1), (60, 60, 3.0, -1), (196, 180, 3.0, 1), (60, 180, 5.0, 1),
         (200, 60, 6.0, -1), (128, 64, 8.0, 1), (128, 176, 10.0, -1), (90, 130, 2.5, 1)]


def orb_blob_image():
    return blob_image(256, 240, blobs=BLOBS)


def mirrored_texture(w, h, seed):
    """a texture beside its mirror image: every corner of layer 0 has a twin with the same H"""
    t = texture(w // 2, h, seed)
    return np.ascontiguousarray(np.concatenate([t, t[:, ::-1]], axis=1))


def squares(w=160, h=96):
    """bright axis-aligned squares on a dark field, well inside the default candidate band"""
    img = np.full((h, w), 20, np.uint8)
    boxes = [(40, 36, 60, 56), (90, 38, 120, 60)]   # x0, y0, x1, y1 (inclusive)
    for x0, y0, x1, y1 in boxes:
        img[y0:y1 + 1, x0:x1 + 1] = 220
    return img, boxes


def frame_of(name, w, h):
    if name == "blobs":
        return orb_blob_image()
    if name[0] == "m":
        return mirrored_texture(w, h, int(name[1:]))
    return texture(w, h, int(name[1:]))


def second_pattern():
    """another valid table: the default one turned by a quarter and mirrored"""
    p = O.default_pattern().astype(np.int64)
    return np.stack([-p[:, 1], -p[:, 0], -p[:, 3], -p[:, 2]], 1).astype(np.int8)


def same_descriptors(got, want):
    """descriptors compared as bytes; a description of the first difference or None"""
    got, want = np.ascontiguousarray(got, np.uint8), np.ascontiguousarray(want, np.uint8)
    if got.shape != want.shape:
        return "shape: %r against %r" % (got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    if bad.size:
        bits = int(np.unpackbits(got[bad[0]] ^ want[bad[0]]).sum())
        return "descriptor %d of %d: %d bits differ (%d rows differ)" % (bad[0], len(got), bits, bad.size)
    return None


def tie_cutting_features(img, n_levels=8, lo=4, hi=200):
    """the smallest n_features in lo..hi under which every layer that has candidates has more than its quota, and layer 0's quota
    falls between two candidates of equal H (so the (y, x) rule decides which is kept); None if there is none"""
    p = O.default_params()
    per = [O.layer_candidates(O.layer(img, l), p) for l in range(n_levels)]
    H0 = np.sort(per[0][2])[::-1]
    for nf in range(lo, hi):
        q = O.level_quota(nf, n_levels)
        if all(len(per[l][0]) > q[l] for l in range(n_levels) if len(per[l][0])) and 0 < q[0] < len(H0) and H0[q[0] - 1] == H0[q[0]]:
            return nf
    return None
