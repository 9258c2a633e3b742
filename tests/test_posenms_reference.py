"""Hand-worked cases that pin tests/posenms_reference.py, the gauge of PoseNMS, and a case per mutation switch that
shows the gauge tells the rule from its mutation.  No GPU.

The people are K keypoints with one sigma; a copy shifted by d along x has, against the original and with equal areas,
e_k = d^2 / (2 sigma)^2 / area / 2 for every keypoint, so OKS = exp(-e): ``shift(oks)`` inverts that."""
import numpy as np
import pytest

from tests import posenms_reference as PR
from tests.cocoeval_reference import shift_for_oks

K, SIGMA, AREA = 5, 0.05, 3000.0
SIG = np.full(K, SIGMA)
BASE = np.array([[10.0, 20.0], [40.0, 25.0], [30.0, 60.0], [15.0, 70.0], [55.0, 80.0]])


def shift(oks, area=AREA):
    return shift_for_oks(oks, SIGMA, area)


def image(shifts, scores, areas=None, vis=None):
    kpts = np.stack([BASE + (s, 0.0) for s in shifts]) if len(shifts) else np.zeros((0, K, 2))
    return PR.make_image(kpts, scores, np.full(len(shifts), AREA) if areas is None else areas, vis)


def test_identical_poses_have_oks_one():
    assert PR.pair_oks(BASE, BASE.copy(), AREA, 1.3 * AREA, SIG) == 1.0
    d = shift(0.8)
    assert abs(PR.pair_oks(BASE, BASE + (d, 0.0), AREA, AREA, SIG) - 0.8) < 1e-12
    # the mean of the two areas is the scale: (1 + 3) / 2 = 2 times the area halves e
    assert abs(PR.pair_oks(BASE, BASE + (d, 0.0), AREA, 3 * AREA, SIG) - 0.8 ** 0.5) < 1e-12
    # symmetric in its arguments
    assert PR.pair_oks(BASE, BASE + (d, 0.0), AREA, 3 * AREA, SIG) == PR.pair_oks(BASE + (d, 0.0), BASE, 3 * AREA, AREA,
                                                                                 SIG)


def test_visibility_selects_the_keypoints_and_none_gives_zero():
    moved = BASE.copy()
    moved[0] += (shift(0.5), 0.0)                      # only keypoint 0 differs
    va, vb = np.array([0.9, 0.9, 0.9, 0.1, 0.9]), np.array([0.9, 0.9, 0.3, 0.9, 0.9])
    assert abs(PR.pair_oks(BASE, moved, AREA, AREA, SIG) - (4 + 0.5) / 5) < 1e-12
    assert abs(PR.pair_oks(BASE, moved, AREA, AREA, SIG, va, vb, 0.2) - (3 + 0.5) / 4) < 1e-12     # keypoint 3 is out
    assert abs(PR.pair_oks(BASE, moved, AREA, AREA, SIG, va, vb, 0.3) - (2 + 0.5) / 3) < 1e-12     # 0.3 > 0.3 is not
    assert PR.pair_oks(BASE, moved, AREA, AREA, SIG, va, vb, 0.9) == 0.0                           # n == 0
    with pytest.raises(ValueError):
        PR.nms_image(image([0.0], [0.5]), SIG, vis_thr=0.2)


def test_rescore_by_hand():
    ks = np.array([[0.9, 0.1, 0.5, 0.2, 0.3], [0.1, 0.2, 0.0, 0.15, 0.2], [0.25, 0.25, 0.25, 0.25, 0.25]])
    got = PR.rescore(ks, [0.8, 0.7, 0.5], 0.2)
    assert got[0] == 0.8 * (((0.9 + 0.5) + 0.3) / 3)           # 0.2 > 0.2 is not
    assert got[1] == 0.0                                       # n == 0
    assert got[2] == 0.5 * 0.25
    assert PR.rescore(ks, [0.8, 0.7, 0.5], 0.0)[1] == 0.7 * ((((0.1 + 0.2) + 0.15) + 0.2) / 4)
    assert PR.rescore(np.zeros((0, 5)), np.zeros(0)).shape == (0,)


def test_hard_chain_b_is_suppressed_so_c_survives():
    """a, b, c in a row, each 0.92 from its neighbour, a and c 0.92^4 = 0.716 apart: a suppresses b, and b, being
    dead, does not suppress c."""
    d = shift(0.92)
    im = image([0.0, d, 2 * d], [0.9, 0.8, 0.7])
    assert abs(PR.pair_oks(im["kpts"][0], im["kpts"][2], AREA, AREA, SIG) - 0.92 ** 4) < 1e-12
    r = PR.nms_image(im, SIG, "hard", 0.9)
    assert r["keep"].tolist() == [True, False, True] and r["picks"] == [0, 2]
    assert r["scores"].tobytes() == im["score"].tobytes()
    assert len(r["oks_seen"]) == 2 + 0 + 0                     # (a, b), (a, c); b is dead; c has nobody after it
    # given in another order, the scores still decide: now b is the pivot and takes both neighbours
    r = PR.nms_image(image([0.0, d, 2 * d], [0.7, 0.9, 0.8]), SIG, "hard", 0.9)
    assert r["keep"].tolist() == [False, True, False]
    # at 0.95 nothing is suppressed
    assert PR.nms_image(im, SIG, "hard", 0.95)["keep"].all()
    assert PR.nms_image(image([], []), SIG)["keep"].shape == (0,)


def test_soft_scores_by_hand():
    d = shift(0.95)
    far = 1e4
    im = image([0.0, d, far], [0.9, 0.85, 0.5])
    g = PR.nms_image(im, SIG, "soft_gaussian", 0.9)
    w = np.exp(-0.95 ** 2 / 0.9)                               # 0.3668: b drops below c
    assert g["picks"] == [0, 2, 1] and g["keep"].all()
    assert g["scores"][0] == 0.9 and g["scores"][2] == 0.5 and abs(g["scores"][1] - 0.85 * w) < 1e-12
    assert g["gaps"][0] == (0.9, 0.85, True, 0, 1) and g["gaps"][1][0] == 0.5 and g["gaps"][2][1] is None
    lin = PR.nms_image(im, SIG, "soft_linear", 0.9)
    assert lin["picks"] == [0, 2, 1] and abs(lin["scores"][1] - 0.85 * 0.05) < 1e-12 and lin["scores"][2] == 0.5
    # max_dets = 2: the first two picks are kept; b keeps its current score
    cut = PR.nms_image(im, SIG, "soft_gaussian", 0.9, max_dets=2)
    assert cut["keep"].tolist() == [True, False, True] and abs(cut["scores"][1] - 0.85 * w) < 1e-12
    one = PR.nms_image(im, SIG, "soft_linear", 0.9, max_dets=1)
    assert one["keep"].tolist() == [True, False, False] and abs(one["scores"][1] - 0.85 * 0.05) < 1e-12
    # two rescorings multiply
    im3 = image([0.0, d, d], [0.9, 0.8, 0.1])
    r = PR.nms_image(im3, SIG, "soft_gaussian", 0.9)
    assert r["picks"] == [0, 1, 2] and abs(r["scores"][2] - 0.1 * w * np.exp(-1 / 0.9)) < 1e-12
    # linear: below the threshold nothing changes
    low = PR.nms_image(image([0.0, shift(0.5)], [0.9, 0.8]), SIG, "soft_linear", 0.9)
    assert low["scores"].tolist() == [0.9, 0.8]


def test_run_concatenates_and_counts():
    d = shift(0.95)
    images = [image([0.0, d], [0.9, 0.8]), image([], []), image([0.0], [0.3])]
    r = PR.run(images, SIG, "hard", 0.9)
    assert r["keep"].tolist() == [True, False, True] and r["counts"].tolist() == [1, 0, 1]
    assert r["counts"].dtype == np.int32
    with pytest.raises(ValueError):
        PR.run(images, SIG, "softer")


# ------------------------------------------------------------------------------------------------ the mutations
def test_mutation_unstable_tie():
    d = shift(0.95)
    im = image([0.0, d], [0.7, 0.7])
    for mode in PR.MODES:
        assert PR.nms_image(im, SIG, mode, 0.9, max_dets=1)["keep"].tolist() == [True, False], mode
        assert PR.nms_image(im, SIG, mode, 0.9, max_dets=1, unstable_tie=True)["keep"].tolist() == [False, True], mode


def test_mutation_ge_instead_of_gt():
    im = image([0.0, 0.0], [0.9, 0.8])                          # OKS exactly 1
    assert PR.nms_image(im, SIG, "hard", 1.0)["keep"].tolist() == [True, True]
    assert PR.nms_image(im, SIG, "hard", 1.0, ge_suppress=True)["keep"].tolist() == [True, False]
    assert PR.nms_image(im, SIG, "hard", 0.9)["keep"].tolist() == [True, False]


def test_mutation_pivot_area():
    """The pivot is small (area A), the other large (4 A): the mean 2.5 A gives 0.92, the pivot's own area gives
    0.92^2.5 = 0.81."""
    d = shift(0.92, 2.5 * AREA)
    im = image([0.0, d], [0.9, 0.8], areas=[AREA, 4 * AREA])
    assert PR.nms_image(im, SIG, "hard", 0.9)["keep"].tolist() == [True, False]
    assert PR.nms_image(im, SIG, "hard", 0.9, pivot_area=True)["keep"].tolist() == [True, True]


def test_mutation_linear_below_the_threshold():
    im = image([0.0, shift(0.5)], [0.9, 0.8])
    assert PR.nms_image(im, SIG, "soft_linear", 0.9)["scores"][1] == 0.8
    assert abs(PR.nms_image(im, SIG, "soft_linear", 0.9, linear_below=True)["scores"][1] - 0.4) < 1e-12


def test_random_image_is_seeded_and_straddles_the_threshold():
    a = PR.random_image(np.random.default_rng(3), 17, 40, identical=True, equal_scores=True)
    b = PR.random_image(np.random.default_rng(3), 17, 40, identical=True, equal_scores=True)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert a["kpts"].shape == (40, 17, 2) and a["vis"].shape == (40, 17)
    assert a["kpts"][0].tobytes() == a["kpts"][1].tobytes() and a["area"][0] == a["area"][1]
    assert a["vis"][0].tobytes() == a["vis"][1].tobytes() and a["score"][0] == a["score"][1]
    assert len(set(a["score"][20:23].tolist())) == 1 and len(set(a["score"].tolist())) == 40 - 1 - 2
    assert a["score"].min() > 0.05 and a["score"].max() < 1.0
    seen = PR.nms_image(a, PR.default_sigmas(17), "soft_gaussian", 0.9, max_dets=40)["oks_seen"]
    assert any(v > 0.9 for v in seen) and any(0.3 < v < 0.9 for v in seen) and 1.0 in seen
    assert PR.random_image(np.random.default_rng(3), 1, 0)["kpts"].shape == (0, 1, 2)
