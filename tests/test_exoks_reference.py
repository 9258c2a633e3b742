"""CPU tests of Ex-OKS evaluation: the gauge of tests/exoks_reference.py pinned on hand-computed cases and on the plain
OKS, the conditions its fixtures have to meet for tests/test_exoks_gpu.py (the seeds are chosen here), and what
CocoKeypointEval(ex_oks=True) does without a device: argument errors, the JSON helpers, the command line's parser."""
import json

import numpy as np
import pytest

from tests import cocoeval_reference as CR
from tests import exoks_reference as XR

K = 17
SIG = np.full(K, 0.05)
AREA = 5000.0
WINDOW = (100.0, 100.0, 200.0, 200.0)


def _person(inside=True, seed=0):
    """17 annotated keypoints, all inside WINDOW (its inner [120, 180]^2) or all outside it (to its right)."""
    rng = np.random.default_rng(seed)
    kp = np.zeros((K, 3))
    kp[:, 0] = rng.uniform(120, 180, K) + (0.0 if inside else 200.0)
    kp[:, 1] = rng.uniform(120, 180, K)
    kp[:, 2] = 2
    return kp, (100.0, 100.0, 100.0, 100.0)


def _image(kp, box, dets, presence, scores=None):
    D = len(dets)
    im = CR.make_image([kp], [box], [AREA], None, dets, scores or [0.9] * D, [AREA] * D)
    return dict(im, gt_window=np.array([WINDOW]), dt_presence=np.asarray(presence, dtype=np.float64).reshape(D, K))


def _exoks(im, tau=0.5, info=None):
    return XR.compute_exoks(im["dt_kpts"], im["dt_presence"], im["gt_kpts"], im["gt_bbox"], im["gt_area"],
                            im["gt_window"], SIG, tau, info)


# ------------------------------------------------------------------------------------------------ anchors
def test_all_outside_and_all_reported_absent_is_a_perfect_score():
    """Every keypoint outside the window, every presence 0: each term is 1 wherever the detection put them, so
    ExOKS = 1 exactly and every stat of the "all" and "medium" ranges is 1."""
    kp, box = _person(inside=False)
    im = _image(kp, box, [kp[:, :2] + 777.0], np.zeros((1, K)))
    info = {}
    assert _exoks(im, info=info)[0, 0] == 1.0 and info["absent"] == K and info["both"] == 0
    s = XR.evaluate([im], SIG)
    for name in ("AP", "AP50", "AP75", "APm", "AR", "ARm"):
        assert abs(s[name] - 1.0) < 1e-12, (name, s[name])
    # plain OKS sees a detection 777 px off: nothing
    assert CR.evaluate([im], SIG)["AP"] == 0.0


def test_an_inside_keypoint_reported_absent_contributes_nothing():
    """A detection exactly on the ground truth: K terms of 1.  Reporting m of them absent leaves (K - m) / K."""
    kp, box = _person()
    for m in (1, 5, K):
        p = np.ones(K)
        p[:m] = 0.2
        info = {}
        got = _exoks(_image(kp, box, [kp[:, :2]], p), info=info)[0, 0]
        assert got == (K - m) / K and info["missed"] == m and info["both"] == K - m
    # AP: 5 of 17 missed gives ExOKS 12 / 17 = 0.7059: matched at 0.5 .. 0.7, five thresholds of ten
    p = np.ones(K)
    p[:5] = 0.0
    s = XR.evaluate([_image(kp, box, [kp[:, :2]], p)], SIG)
    assert abs(s["AP"] - 0.5) < 1e-12 and abs(s["AP50"] - 1.0) < 1e-12 and s["AP75"] == 0.0


def test_a_false_positive_is_charged_by_its_depth():
    """Every keypoint outside the window, every one predicted present at depth b inside it, b chosen with
    shift_for_oks so that exp(-b^2 / (2 sigma)^2 / area / 2) is a wanted value."""
    kp, box = _person(inside=False)
    for want in (0.62, 0.92, 0.999):
        b = CR.shift_for_oks(want, 0.05, AREA)
        assert 0 < b < 50
        # depth b from the left edge, from the bottom edge, and in a corner (the nearer border counts)
        for x, y in ((100.0 + b, 150.0), (150.0, 200.0 - b), (100.0 + b, 100.0 + b + 3.0)):
            det = np.tile([x, y], (K, 1))
            info = {}
            got = _exoks(_image(kp, box, [det], np.ones(K)), info=info)[0, 0]
            assert abs(got - want) < 1e-12 and info["false_positive"] == K, (want, x, y, got)
    # one keypoint: the others reported absent, each worth 1
    b = CR.shift_for_oks(0.5, 0.05, AREA)
    p = np.zeros(K)
    p[4] = 0.9
    det = np.tile([200.0 - b, 150.0], (K, 1))
    assert abs(_exoks(_image(kp, box, [det], p))[0, 0] - (K - 1 + 0.5) / K) < 1e-12


def test_a_prediction_outside_the_window_for_an_outside_keypoint_costs_nothing():
    kp, box = _person(inside=False)
    for x, y in ((50.0, 150.0), (150.0, 250.0), (100.0, 150.0), (200.0, 150.0), (150.0, 100.0), (150.0, 200.0),
                 (-1e6, 1e6)):
        det = np.tile([x, y], (K, 1))
        assert _exoks(_image(kp, box, [det], np.ones(K)))[0, 0] == 1.0, (x, y)     # b = 0: exp(-0) = 1 exactly


def test_presence_equal_to_the_threshold_counts_as_present():
    kp, box = _person()
    below = np.nextafter(0.5, 0.0)
    assert _exoks(_image(kp, box, [kp[:, :2]], np.full(K, 0.5)))[0, 0] == 1.0
    assert _exoks(_image(kp, box, [kp[:, :2]], np.full(K, below)))[0, 0] == 0.0
    assert _exoks(_image(kp, box, [kp[:, :2]], np.full(K, below)), tau=below)[0, 0] == 1.0
    # and the window is half open: a keypoint on x0 / y0 is inside, one on x1 / y1 is outside
    for x, y, inside in ((100.0, 150.0, True), (150.0, 100.0, True), (200.0, 150.0, False), (150.0, 200.0, False)):
        edge = kp.copy()
        edge[:, 0], edge[:, 1] = x, y
        info = {}
        _exoks(_image(edge, box, [edge[:, :2]], np.zeros(K)), info=info)
        assert info["missed" if inside else "absent"] == K, (x, y)


def test_unannotated_keypoints_do_not_count_and_no_visible_keeps_the_grown_box():
    kp, box = _person()
    kp[::2, 2] = 0
    p = np.ones(K)
    p[::2] = 0.0                                    # absent on keypoints that are not annotated: not read
    det = kp[:, :2].copy()
    det[::2] += 500.0
    assert _exoks(_image(kp, box, [det], p))[0, 0] == 1.0
    kp[:, 2] = 0
    im = _image(kp, box, [det, det + 5000.0], np.zeros((2, K)))
    assert np.array_equal(_exoks(im), CR.compute_oks(im["dt_kpts"], im["gt_kpts"], im["gt_bbox"], im["gt_area"], SIG))


# ------------------------------------------------------------------------------------------------ against the plain gauge
@pytest.mark.parametrize("k", [1, 17, 133])
def test_all_inside_and_all_present_is_the_plain_oks_bit_for_bit(k):
    images = XR.ragged_images(k, all_inside=True)
    sig = CR.default_sigmas(k)
    seen = 0
    for im in images:
        info = {}
        got = XR.compute_exoks(im["dt_kpts"], im["dt_presence"], im["gt_kpts"], im["gt_bbox"], im["gt_area"],
                               im["gt_window"], sig, info=info)
        want = CR.compute_oks(im["dt_kpts"], im["gt_kpts"], im["gt_bbox"], im["gt_area"], sig)
        assert np.array_equal(got, want)
        assert info["missed"] == info["absent"] == info["false_positive"] == 0
        seen += got.size
    assert seen == sum(d * g for d, g in XR.RAGGED)
    # the same keypoints as the batch with real windows: only windows and presence differ
    for a, b in zip(images, XR.ragged_images(k)):
        assert a["dt_kpts"].tobytes() == b["dt_kpts"].tobytes() and a["gt_kpts"].tobytes() == b["gt_kpts"].tobytes()


def test_the_restated_matching_is_cocoeval_references():
    """exoks_reference.evaluate_image on the plain OKS gives cocoeval_reference.evaluate_image's result, and the
    chained evaluation its stats: the restated walk is the original."""
    images = XR.ragged_images(17)
    sig = CR.default_sigmas(17)
    for rng in CR.AREA_RANGES:
        for im in images:
            want = CR.evaluate_image(im, sig, rng)
            got = XR.evaluate_image(im, sig, rng, similarity=XR.plain_similarity)
            assert got["npig"] == want["npig"]
            for key in ("dt_index", "dt_score", "dt_matched", "dt_ignore", "gt_ignore", "gt_matched", "oks"):
                assert np.array_equal(got[key], want[key]), key
    want, got = CR.evaluate(images, sig), XR.evaluate(images, sig, similarity=XR.plain_similarity)
    assert all(got[k] == want[k] for k in CR.STATS) and np.array_equal(got["precision"], want["precision"])


# ------------------------------------------------------------------------------------------------ fixture conditions
def _check_candidates(results, images):
    from tests.test_cocoeval_gpu import check_fixture
    check_fixture(results, images)


@pytest.mark.parametrize("k", [1, 17, 133])
def test_ragged_fixture_conditions(k):
    """What tests/test_exoks_gpu.py asks of the ragged batch, on the gauge: the four cases occur (K = 17, 133: in every
    image that has both detections and ground truths; K = 1: over the batch, since its (1, 1) image is a single term
    and its twin image shares one window), every exponent is below 29, where both exp implementations state 1 ulp;
    K = 17, the batch whose flags are compared: no candidate Ex-OKS within 1e-9 of a threshold or of another value of
    its row, twins apart, with every detection kept and with the cut to 20."""
    images = XR.ragged_images(k)
    sig = CR.default_sigmas(k)
    total = dict.fromkeys(XR.CASES, 0)
    e_max = 0.0
    for im, (D, G) in zip(images, XR.RAGGED):
        assert im["gt_window"].shape == (G, 4) and im["dt_presence"].shape == (D, k)
        assert np.all(im["gt_window"][:, 2:] > im["gt_window"][:, :2])
        assert np.array_equal(im["dt_presence"], im["dt_presence"].astype(np.float32).astype(np.float64))
        if not (D and G):
            continue
        info = {}
        XR.compute_exoks(im["dt_kpts"], im["dt_presence"], im["gt_kpts"], im["gt_bbox"], im["gt_area"],
                         im["gt_window"], sig, info=info)
        if k > 1:
            assert all(info[c] > 0 for c in XR.CASES), ((D, G), info)
        for c in XR.CASES:
            total[c] += info[c]
        e_max = max(e_max, info["e_max"])
    print(f"K = {k}: cases {total}, largest e {e_max:.2f}")
    assert all(total[c] > 0 for c in XR.CASES) and e_max < 29.0
    # every kind of presence value is in there
    p = np.concatenate([im["dt_presence"].reshape(-1) for im in images])
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    assert all((p == v).any() for v in (0.0, below, 0.5, 1.0)) and ((p > 0.5) & (p < 1.0)).any()
    if k == 17:
        for max_dets in (64, 20):
            want = XR.evaluate(images, sig, max_dets=max_dets)
            _check_candidates(want["per_image"][0], images)
        twin = want["per_image"][0][4]
        assert twin["oks"][:, 0].tobytes() == twin["oks"][:, 1].tobytes() and twin["gt_matched"][:, 1].any()
        # what tests/test_exoks_gpu.py compares Ex-OKS with: the plain mode and another threshold, same condition
        plain, low = CR.evaluate(images, sig), XR.evaluate(images, sig, tau=0.25)
        _check_candidates(plain["per_image"][0], images)
        _check_candidates(low["per_image"][0], images)
        assert any(abs(want[s] - plain[s]) > 1e-3 for s in CR.STATS)           # the mode matters on this batch
        assert any(abs(want[s] - low[s]) > 1e-3 for s in CR.STATS)             # and so does the threshold


def test_batch64_fixture_conditions():
    images = XR.batch64()
    want = XR.evaluate(images, CR.COCO17_SIGMAS)
    _check_candidates(want["per_image"][0], images)
    assert any(r["dt_index"].size == 20 and im["dt_score"].size > 20 for r, im in zip(want["per_image"][0], images))
    assert all(want["info"][c] > 0 for c in XR.CASES) and want["info"]["e_max"] < 29.0
    assert 0.05 < want["AP"] < 0.95 and want["APm"] > -1 and want["APl"] > -1       # a batch that says something
    twin = want["per_image"][0][3]
    assert twin["oks"][:, 0].tobytes() == twin["oks"][:, 1].tobytes()


# ------------------------------------------------------------------------------------------------ the module, no device
def _evaluator(**kw):
    from probpose_pytorch_amd import CocoKeypointEval
    return CocoKeypointEval(SIG, **kw)


def test_constructor_and_window_errors():
    from probpose_pytorch_amd import CocoKeypointEval
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="presence_threshold"):
            CocoKeypointEval(SIG, ex_oks=True, presence_threshold=bad)
    for ok in (0.0, 0.5, 1.0):
        assert CocoKeypointEval(SIG, ex_oks=True, presence_threshold=ok).presence_threshold == ok
    assert _evaluator().ex_oks is False and _evaluator().presence_threshold == 0.5
    kp, box = _person()
    good = dict(image_id=1, keypoints=kp[None], bboxes=[box], areas=[AREA])
    for ex in (True, False):            # without Ex-OKS windows are checked all the same
        ev = _evaluator(ex_oks=ex)
        for bad in ([0.0, 0.0, 10.0], [[0.0, 0.0, 10.0, 10.0]] * 2, [0.0, 0.0, np.nan, 10.0],
                    [0.0, 0.0, np.inf, 10.0], [5.0, 0.0, 5.0, 10.0], [0.0, 7.0, 10.0, 6.0]):
            with pytest.raises(ValueError, match="windows"):
                ev.add_ground_truth(**good, windows=bad)
        assert not ev._gts
        ev.add_ground_truth(**good, windows=WINDOW)                        # [4] goes to every instance
        ev.add_ground_truth(2, np.stack([kp, kp]), [box, box], [AREA, AREA], windows=[WINDOW, (0, 0, 1, 1)])
        assert ev._window_array(2).tolist() == [list(WINDOW), list(WINDOW), [0, 0, 1, 1]]
    ev = _evaluator(ex_oks=True)
    with pytest.raises(ValueError, match="windows"):
        ev.add_ground_truth(**good)
    ev.add_ground_truth(3, np.zeros((0, K, 3)), np.zeros((0, 4)), np.zeros(0))      # G = 0 needs none
    _evaluator().add_ground_truth(**good)                                            # nor does the plain mode


def test_presence_errors():
    det = dict(image_ids=[1, 1], keypoints=np.zeros((2, K, 2)), scores=np.array([0.5, 0.4]),
               areas=np.array([1.0, 2.0]))
    good = np.full((2, K), 0.5)
    for ex in (True, False):
        ev = _evaluator(ex_oks=ex)
        for bad in (np.zeros((2, K + 1)), np.zeros((3, K)), np.zeros(K)):
            with pytest.raises(ValueError, match="presence"):
                ev.add_detections(**det, presence=bad)
        for value in (np.nan, np.inf, -0.01, 1.01):
            bad = good.copy()
            bad[1, 3] = value
            with pytest.raises(ValueError, match="presence"):
                ev.add_detections(**det, presence=bad)
        assert not ev._dets
        ev.add_detections(**det, presence=good)
        ev.add_detections(**det, presence=np.array([[0.0] * K, [1.0] * K], dtype=np.float32))
        assert len(ev._dets) == len(ev._presence) == 2 and ev._presence[1].dtype == np.float64
    with pytest.raises(ValueError, match="presence"):
        _evaluator(ex_oks=True).add_detections(**det)
    ev = _evaluator()
    ev.add_detections(**det)
    assert ev._presence == [None]
    ev.reset()
    assert not ev._presence and not ev._windows


def _coco_files(tmp_path, images, size=True, presence_key=True):
    sizes = [(640 + i, 480) for i in range(len(images))] if size else None
    return XR.coco_files(tmp_path, images, sizes, presence_key)


def test_the_command_lines_fixture_meets_the_conditions():
    """The ragged batch under the windows a COCO file can express, (0, 0, width, height): the four cases occur, every
    exponent is below 29 and no candidate sits on a threshold or on another value of its row."""
    images = XR.ragged_images(17)
    images = XR.with_image_windows(images, XR.image_sizes(images))
    want = XR.evaluate(images, CR.COCO17_SIGMAS)
    _check_candidates(want["per_image"][0], images)
    assert all(want["info"][c] > 0 for c in XR.CASES) and want["info"]["e_max"] < 29.0
    assert want["AP"] > 0.05


def test_json_windows_and_presence(tmp_path):
    from probpose_pytorch_amd import CocoKeypointEval
    images = XR.ragged_images(17)[2:5]                  # (1, 1), (20, 7), (33, 2)
    want_p = np.concatenate([im["dt_presence"] for im in images])
    for presence_key in (True, False):
        gt, res, gpath, rpath = _coco_files(tmp_path, images, presence_key=presence_key)
        for source, results in ((gpath, rpath), (gt, res)):
            ev = CocoKeypointEval.from_coco_json(source, CR.COCO17_SIGMAS, ex_oks=True, presence_threshold=0.4)
            assert ev.ex_oks and ev.presence_threshold == 0.4
            ev.add_results_json(results)
            win = ev._window_array(3)
            assert win.tolist() == [[0, 0, 640, 480]] + [[0, 0, 641, 480]] * 7 + [[0, 0, 642, 480]] * 2
            (pos, dkp, sc, dar), = ev._dets
            assert ev._presence[0].tobytes() == want_p.tobytes()
            assert dkp.tobytes() == np.concatenate([im["dt_kpts"] for im in images]).tobytes()
    # the plain mode reads neither
    ev = CocoKeypointEval.from_coco_json(gt, CR.COCO17_SIGMAS)
    ev.add_results_json(res)
    assert ev._presence == [None] and ev._window_array(3).shape == (0, 4)
    # an image without width / height has no window; the plain mode does not ask for one
    gt, res, gpath, rpath = _coco_files(tmp_path, images, size=False)
    with pytest.raises(ValueError, match="width"):
        CocoKeypointEval.from_coco_json(gpath, CR.COCO17_SIGMAS, ex_oks=True)
    CocoKeypointEval.from_coco_json(gpath, CR.COCO17_SIGMAS)
    gt["images"][1]["width"] = 100
    with pytest.raises(ValueError, match="width"):
        CocoKeypointEval.from_coco_json(gt, CR.COCO17_SIGMAS, ex_oks=True)
    ev = CocoKeypointEval.from_coco_json(_coco_files(tmp_path, images)[0], CR.COCO17_SIGMAS, ex_oks=True)
    with pytest.raises(ValueError, match="presence"):
        ev.add_results_json([dict(image_id=10, category_id=1, keypoints=[0.0] * 51, score=0.5, presence=[0.5] * 3)])
    with pytest.raises(ValueError, match="presence"):       # a COCO visibility of 2 is no probability
        ev.add_results_json([dict(image_id=10, category_id=1, keypoints=[0.0, 0.0, 2.0] * 17, score=0.5)])


def test_command_line_parsing():
    from probpose_pytorch_amd import cocoeval
    a = cocoeval._parser().parse_args(["gt.json", "res.json"])
    assert (a.ground_truth, a.results, a.sigmas, a.category_id, a.max_dets, a.ex_oks, a.presence_thr) == \
        ("gt.json", "res.json", "coco17", 1, 20, False, 0.5)
    a = cocoeval._parser().parse_args(["g", "r", "--sigmas", "0.05", "--category-id", "3", "--max-dets", "7",
                                       "--ex-oks", "--presence-thr", "0.3"])
    assert (a.sigmas, a.category_id, a.max_dets, a.ex_oks, a.presence_thr) == ("0.05", 3, 7, True, 0.3)
    with pytest.raises(SystemExit):
        cocoeval._parser().parse_args(["only_one.json"])
    assert np.array_equal(cocoeval._cli_sigmas("coco17", {}, 1), CR.COCO17_SIGMAS)
    data = dict(annotations=[dict(category_id=2, keypoints=[0.0] * 9), dict(category_id=1, keypoints=[0.0] * 15)])
    assert cocoeval._cli_sigmas("0.07", data, 1).tolist() == [0.07] * 5
    data["categories"] = [dict(id=1, keypoints=["a", "b"])]
    assert cocoeval._cli_sigmas("0.07", data, 1).tolist() == [0.07] * 2
    for spec, d in (("coco", data), ("0.07", {})):
        with pytest.raises(ValueError, match="--sigmas"):
            cocoeval._cli_sigmas(spec, d, 1)


def test_ex_oks_evaluate_has_no_cpu_fallback():
    """Without a device evaluate() raises; with one it scores the detection that sits on the ground truth."""
    import torch
    from probpose_pytorch_amd import _lib
    kp, box = _person()
    ev = _evaluator(ex_oks=True)
    ev.add_ground_truth(1, kp[None], [box], [AREA], windows=WINDOW)
    ev.add_detections([1], kp[None, :, :2], [0.9], [AREA], presence=np.ones((1, K)))
    if torch.cuda.is_available():
        assert abs(ev.evaluate()["AP"] - 1.0) < 1e-12        # precision is tp / (tp + fp + eps): not 1 to the bit
    else:
        with pytest.raises(_lib.HipExtensionError):
            ev.evaluate()
