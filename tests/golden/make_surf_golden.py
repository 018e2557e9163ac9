"""Writes tests/golden/surf_160x96.npz: the restatement's (tests/surf_ref.py) key points and descriptors of one 160 x 96 texture
frame, under the default parameters, upright, and under cap = 16.  tests/test_surf_ref_cpu.py compares the restatement with this
file bit for bit, so that a later edit of the restatement is noticed.  Run from the repository root: python tests/golden/make_surf_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import surf_cases as K   # noqa: E402
import surf_ref as S     # noqa: E402

SEED = 3


def vectors():
    img = K.texture(160, 96, SEED)
    kp, desc = S.detect_describe(img)
    up = dict(S.default_params(), upright=1)
    kp_u, desc_u = S.detect_describe(img, up)
    kp_c, desc_c = S.detect_describe(img, None, 16)
    I = S.integral(img)
    r11, _ = S.response_layer(I, 1, 1)
    return dict(image=img, keypoints=kp, descriptors=desc, keypoints_upright=kp_u, descriptors_upright=desc_u,
                keypoints_cap16=kp_c, descriptors_cap16=desc_c, integral_last_row=I[-1], response_o1_l1=r11)


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "surf_160x96.npz"), **vectors())
    print("wrote surf_160x96.npz")
