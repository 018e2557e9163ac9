"""Inputs of the SURF tests (tests/test_surf_ref_cpu.py, tests/test_gpu_surf.py, tests/golden/make_surf_golden.py): a helper module,
not a test.  Everything is deterministic."""
import importlib

import numpy as np

import surf_ref as S

synth = importlib.import_module("uw-slam_amd.synth")

# (x, y, sigma, polarity): isolated Gaussian blobs on a 256 x 240 frame, sigma chosen per octave (a blob of sigma b peaks at filter
# size ~5.5 b: 3 -> octave 0, 6 -> octave 1, 11.5 -> octave 2, 23 -> octave 3), placed where the layer above still has its window
BLOBS = [
    (128, 120, 23.0, 1),
    (58, 58, 11.5, -1), (198, 58, 11.5, 1), (58, 182, 11.5, 1), (198, 182, 11.5, -1),
    (128, 30, 6.0, 1), (128, 210, 6.0, -1), (30, 120, 6.0, -1), (226, 120, 6.0, 1),
    (16, 16, 3.0, 1), (240, 16, 3.0, -1), (16, 224, 3.0, -1), (240, 224, 3.0, 1), (96, 16, 3.0, -1), (160, 224, 3.0, 1),
]
BLOB_OCTAVE = {23.0: 3, 11.5: 2, 6.0: 1, 3.0: 0}


def blob_image(w=256, h=240, blobs=BLOBS, amplitude=100.0, shift=(0, 0)):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.full((h, w), 128.0)
    for x, y, s, pol in blobs:
        f += pol * amplitude * np.exp(-((xs - x - shift[0]) ** 2 + (ys - y - shift[1]) ** 2) / (2.0 * s * s))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def texture(w, h, seed):
    return synth.texture(w, h, seed)


def flat(w, h, value=77):
    return np.full((h, w), value, np.uint8)


def padded_texture(w, h, seed, margin, shift=(0, 0)):
    """a texture window of (w - 2 margin) x (h - 2 margin) on a flat frame, moved by an integer shift: content away from the border"""
    img = np.full((h, w), 128, np.uint8)
    t = synth.texture(w - 2 * margin, h - 2 * margin, seed)
    # fade the window's rim so that the frame holds no step edge
    yy, xx = np.mgrid[0:t.shape[0], 0:t.shape[1]]
    rim = np.minimum(np.minimum(xx, t.shape[1] - 1 - xx), np.minimum(yy, t.shape[0] - 1 - yy)).astype(np.float64)
    a = np.clip(rim / 12.0, 0.0, 1.0)
    t = np.rint(128.0 + a * (t.astype(np.float64) - 128.0)).astype(np.uint8)
    img[margin + shift[1]:margin + shift[1] + t.shape[0], margin + shift[0]:margin + shift[0] + t.shape[1]] = t
    return img


def border_keypoints(w, h):
    """hand-placed key points whose sampling boxes leave the image on every side, and one far outside"""
    rows = [(1.5, 2.25, 12.0), (w - 2.0, 3.5, 20.0), (2.75, h - 1.5, 15.0), (w - 1.25, h - 2.5, 30.0), (w / 2.0, 0.0, 45.0),
            (0.0, h / 2.0, 9.0), (w / 2.0 + 0.5, h - 1.0, 60.0), (w - 0.5, h / 2.0, 25.0), (w / 2.0, h / 2.0, 200.0),
            (-40.0, -30.0, 18.0), (w + 300.0, h + 300.0, 10.0)]
    k = np.zeros(len(rows), S.KEYPOINT)
    for i, (x, y, s) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["size"] = x, y, s
        k[i]["response"], k[i]["octave"], k[i]["laplacian"] = 1000.0 + i, i % 4, (-1, 0, 1)[i % 3]
    return k


def same_keypoints(got, want):
    """key points compared AS INTEGERS (f32 fields as uint32, then octave and laplacian); a description of the first difference or None"""
    got, want = np.ascontiguousarray(got, S.KEYPOINT), np.ascontiguousarray(want, S.KEYPOINT)
    if len(got) != len(want):
        return "count: %d against %d" % (len(got), len(want))
    a, b = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.nonzero((a != b).any(axis=1))[0]
    if bad.size:
        return "key point %d of %d: %r against %r (%d differ)" % (bad[0], len(got), got[bad[0]], want[bad[0]], bad.size)
    return None


def same_descriptors(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "shape: %r against %r" % (got.shape, want.shape)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), 64).any(axis=1))[0]
    if bad.size:
        return "descriptor %d of %d: max |diff| %g (%d rows differ)" % (bad[0], len(got), float(np.abs(got[bad[0]] - want[bad[0]]).max()), bad.size)
    return None
