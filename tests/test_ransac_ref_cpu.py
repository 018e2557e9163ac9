"""The numpy restatement of the RANSAC contract (tests/ransac_ref.py) against TRUTH, so that the yardstick of tests/test_gpu_ransac.py
is known to be a RANSAC: synthetic two-view scenes with known correspondences (tests/ransac_cases.py), recall of the true inliers
and the number of accepted outliers; then constructed cases with known answers, and the sample generator.

Bounds.  Recall: measured with the committed seeds under distance 3, confidence 0.99, 1000 hypotheses (the lowest of each family
stands beside its bound below); the bound is that minimum less 0.04, rounded down to 0.01 — the margin covers nothing but a change
of numpy's random streams.  Accepted outliers: a uniformly random point lies within 3 px of a given epipolar line with a
probability of about 6 px over the image diagonal (800 px), 0.0075; the bound is three times that expectation plus 5 (the tail of
a Poisson count that small), against 0 .. 10 measured."""
import numpy as np
import pytest

import ransac_cases as K
import ransac_ref as R

ARITH_INDEPENDENT = True

# family: (lowest recall measured, bound)
RECALL = {
    "n200_o30": (0.943, 0.90), "n200_o50": (0.980, 0.94), "n2000_o30": (0.986, 0.94), "n2000_o45": (0.935, 0.89),
    "n4096_o20": (0.969, 0.92), "n8_clean": (1.0, 0.96), "n9_clean": (1.0, 0.96), "n12_clean": (0.917, 0.87),
    "n200_planar": (0.993, 0.95), "n200_xtrans": (0.914, 0.87), "n200_forward": (1.0, 0.96), "n200_still_noisy": (1.0, 0.96),
    "n200_still_exact": (1.0, 0.96),
}


@pytest.mark.parametrize("family", [f[0] for f in K.FAMILIES])
def test_restatement_finds_the_true_inliers(family):
    _, n, share, _, _, _, _ = K.FAMILIES[[f[0] for f in K.FAMILIES].index(family)]
    outlier_bound = 3 * (6.0 / 800.0) * share * n + 5
    for i, (m, k0, k1, truth) in enumerate(K.family_scenes(family)):
        mask, good, info = R.ransac(m, k0, k1)
        mask = mask.astype(bool)
        recall = (mask & truth).sum() / truth.sum()
        accepted = int((mask & ~truth).sum())
        print(family, i, "recall %.3f" % recall, "accepted outliers", accepted, "hypotheses run", int(info["hypotheses_run"]))
        assert recall >= RECALL[family][1], (family, i, recall)
        assert accepted <= outlier_bound, (family, i, accepted, outlier_bound)
        assert info["n_inliers"] == mask.sum() == len(good) and good.tobytes() == m[mask].tobytes()
        assert 0 <= info["best_hypothesis"] < info["hypotheses_run"] <= 1000
        if share <= 0.3 and n >= 200:
            assert info["hypotheses_run"] < 1000   # the adaptive count ends the loop early


@pytest.mark.parametrize("case", K.known_cases(), ids=[c[0] for c in K.known_cases()])
def test_known_answers(case):
    name, m, k0, k1, truth, expect = case
    mask, good, info = R.ransac(m, k0, k1)
    assert info["status"] == 0 and len(good) == mask.sum() == info["n_inliers"]
    if expect == "nothing":
        assert not mask.any() and info["best_hypothesis"] == -1 and not np.any(info["F"]) and info["hypotheses_run"] == 0
    elif expect == "all_at_1":
        assert mask.all() and info["hypotheses_run"] == 1 and info["best_hypothesis"] == 0
    elif expect == "truth_kept":
        assert mask.astype(bool)[truth].all()
        assert (mask.astype(bool) & ~truth).sum() <= 3 * (6.0 / 800.0) * (~truth).sum() + 5
    if name == "x_translation_exact":   # F22 = 0 geometry: found through full pivoting, without a fixed f[8] = 1
        assert info["best_hypothesis"] >= 0 and mask.sum() >= truth.sum()


def test_samples_are_distinct_and_depend_on_seed_h_and_n_alone():
    for n in (8, 200):
        for h in range(2000):
            s = R.sample(3, h, n)
            assert len(set(s)) == 8 and min(s) >= 0 and max(s) < n, (n, h, s)
    assert sorted(R.sample(0, 0, 8)) == list(range(8))
    assert R.sample(1, 5, 200) != R.sample(2, 5, 200) and R.sample(1, 5, 200) != R.sample(1, 6, 200)
    assert R.mix(0) == 0   # (the mixer's other values are pinned by the device comparison)


def test_iteration_count_formula():
    assert R.iterations(0.99, 200, 200, 1000) == 0 and R.iterations(1.0, 200, 150, 1000) == 1000
    assert R.iterations(0.99, 200, 0, 1000) == 1000 and R.iterations(0.99, 200, 8, 1000) == 1000
    assert R.iterations(0.99, 200, 140, 1000) == 78   # log(0.01) / log(1 - 0.7^8) = 77.6
    seq = [R.iterations(0.99, 200, k, 1000) for k in range(8, 201)]
    assert all(a >= b for a, b in zip(seq, seq[1:]))
