"""CPU tests of COCO keypoint evaluation: the gauge of tests/cocoeval_reference.py pinned on hand-derived cases and
shown to reject three mutations of the rules, then what CocoKeypointEval does without a device: argument errors, the
JSON round trip, the refusal to evaluate without a GPU, and the C ABI's refusals before any launch."""
import json

import numpy as np
import pytest

from tests import cocoeval_reference as CR

K = 17
SIG = np.full(K, 0.05)
AREA = 5000.0                       # a "medium" person: 32^2 <= 5000 <= 96^2


def _person(x=100.0, y=100.0, side=80.0, v=2, seed=0):
    rng = np.random.default_rng(seed)
    kp = np.zeros((K, 3))
    kp[:, 0] = x + rng.uniform(0, side, K)
    kp[:, 1] = y + rng.uniform(0, side, K)
    kp[:, 2] = v
    return kp, (x, y, side, side)


def _shifted(kp, oks, area=AREA):
    out = kp[:, :2].copy()
    out[:, 0] += CR.shift_for_oks(oks, 0.05, area)
    return out


def _stats(images, **kw):
    return CR.evaluate(images, SIG, **kw)


def test_shift_gives_the_wanted_oks():
    kp, box = _person()
    for want in (0.62, 0.92, 0.5, 0.999):
        got = CR.compute_oks([_shifted(kp, want)], [kp], [box], [AREA], SIG)[0, 0]
        assert abs(got - want) < 1e-12
    # invisible keypoints do not count: moving them changes nothing
    kp2 = kp.copy()
    kp2[::2, 2] = 0
    det = _shifted(kp, 0.8)
    det[::2] += 1000.0
    assert abs(CR.compute_oks([det], [kp2], [box], [AREA], SIG)[0, 0] - 0.8) < 1e-12


def test_perfect_detections():
    """Every ground truth detected exactly: all stats 1 where defined; no medium ground truth -> APm = ARm = -1."""
    images = []
    for i, area in enumerate((200.0 ** 2, 120.0 ** 2, 100.0 ** 2)):       # all large
        kp, box = _person(seed=i)
        images.append(CR.make_image([kp], [box], [area], None, [kp[:, :2]], [0.9 - 0.1 * i], [area]))
    s = _stats(images)
    for name in ("AP", "AP50", "AP75", "APl", "AR", "AR50", "AR75", "ARl"):
        assert abs(s[name] - 1.0) < 1e-12, (name, s[name])
    assert s["APm"] == -1.0 and s["ARm"] == -1.0
    kp, box = _person(seed=9)
    images.append(CR.make_image([kp], [box], [AREA], None, [kp[:, :2]], [0.5], [AREA]))
    s = _stats(images)
    assert all(abs(s[name] - 1.0) < 1e-12 for name in CR.STATS)


def anchor_image():
    """One ground truth, detection A (score 0.9, OKS 0.62) and detection B (score 0.8, OKS 0.92)."""
    kp, box = _person()
    return CR.make_image([kp], [box], [AREA], None, [_shifted(kp, 0.62), _shifted(kp, 0.92)], [0.9, 0.8],
                         [AREA, AREA])


def test_anchor_case():
    """Thresholds 0.5 - 0.6: A takes the ground truth, B is a false positive behind it: precision 1 at every recall.
    0.65 - 0.9: A is a false positive ahead of B: precision 0.5.  0.95: nothing matches.
    AP = (3 * 1 + 6 * 0.5 + 0) / 10 = 0.6, AP50 = 1, AP75 = 0.5, AR = 9 / 10."""
    s = _stats([anchor_image()])
    assert abs(s["AP"] - 0.6) < 1e-12 and abs(s["AP50"] - 1.0) < 1e-12
    assert abs(s["AP75"] - 0.5) < 1e-12 and abs(s["AR"] - 0.9) < 1e-12
    assert abs(s["APm"] - 0.6) < 1e-12 and s["APl"] == -1.0


def test_crowd_is_matched_twice_and_neither_counts():
    kp, box = _person()
    solo, sbox = _person(x=400.0, seed=3)
    im = CR.make_image([kp, solo], [box, sbox], [AREA, AREA], [True, False],
                       [_shifted(kp, 0.88), _shifted(kp, 0.78), solo[:, :2]], [0.9, 0.8, 0.7], [AREA] * 3)
    r = CR.evaluate_image(im, SIG, CR.AREA_RANGES[0])
    assert r["npig"] == 1
    assert r["dt_matched"][0].tolist() == [True, True, True]
    assert r["dt_ignore"][0].tolist() == [True, True, False]
    s = _stats([im])
    assert abs(s["AP50"] - 1.0) < 1e-12 and abs(s["AP75"] - 1.0) < 1e-12 and abs(s["AR"] - 1.0) < 1e-12
    # (above their OKS of 0.88 / 0.78 the two are plain false positives ahead of the hit: precision 1/2 at 0.8 and
    # 0.85, 1/3 at 0.9 and 0.95)
    assert abs(s["AP"] - (6 + 0.5 + 0.5 + 1 / 3 + 1 / 3) / 10) < 1e-12
    # the same ground truth without the crowd flag: the second detection is a false positive
    im2 = dict(im, gt_crowd=np.array([False, False]))
    r2 = CR.evaluate_image(im2, SIG, CR.AREA_RANGES[0])
    assert r2["dt_matched"][0].tolist() == [True, False, True] and not r2["dt_ignore"][0].any()


def test_ground_truth_outside_the_area_range_makes_its_match_ignored():
    kp, box = _person()
    im = CR.make_image([kp], [box], [AREA], None, [kp[:, :2]], [0.9], [AREA])
    large = CR.evaluate_image(im, SIG, CR.AREA_RANGES[2])
    assert large["npig"] == 0 and large["gt_ignore"].tolist() == [True]
    assert large["dt_matched"].all() and large["dt_ignore"].all()
    medium = CR.evaluate_image(im, SIG, CR.AREA_RANGES[1])
    assert medium["npig"] == 1 and medium["dt_matched"].all() and not medium["dt_ignore"].any()


def test_ground_truth_without_visible_keypoints():
    """Scored by the distance to its grown box over all K keypoints, and ignored."""
    kp, box = _person(v=0)
    inside = kp[:, :2].copy()                            # inside the grown box: distance 0 -> OKS 1
    far = inside + 5000.0
    oks = CR.compute_oks([inside, far], [kp], [box], [AREA], SIG)
    assert oks[0, 0] == 1.0 and oks[1, 0] == 0.0
    # one keypoint 10 px right of the grown box's edge, the rest inside: (K - 1 + exp(-e)) / K
    edge = inside.copy()
    edge[3, 0] = box[0] + 2 * box[2] + 10.0
    want = (K - 1 + np.exp(-(10.0 ** 2) / (0.1 ** 2) / (AREA + CR.EPS) / 2)) / K
    assert abs(CR.compute_oks([edge], [kp], [box], [AREA], SIG)[0, 0] - want) < 1e-15
    im = CR.make_image([kp], [box], [AREA], None, [inside], [0.9], [AREA])
    r = CR.evaluate_image(im, SIG, CR.AREA_RANGES[0])
    assert r["npig"] == 0 and r["dt_matched"].all() and r["dt_ignore"].all()
    assert _stats([im])["AP"] == -1.0


def test_unmatched_detection_outside_the_area_range_is_ignored():
    kp, box = _person()
    stray = kp[:, :2] + 3000.0
    im = CR.make_image([kp], [box], [AREA], None, [stray, kp[:, :2]], [0.9, 0.8], [200.0 ** 2, AREA])
    r = CR.evaluate_image(im, SIG, CR.AREA_RANGES[1])
    assert r["dt_matched"][0].tolist() == [False, True] and r["dt_ignore"][0].tolist() == [True, False]
    s = _stats([im])
    assert abs(s["APm"] - 1.0) < 1e-12          # the stray is ignored in "medium" ...
    assert abs(s["AP"] - 0.5) < 1e-12           # ... and a false positive ahead of the hit in "all"


def test_more_than_max_dets_are_cut_by_score():
    kp, box = _person()
    dets = [kp[:, :2] + 3000.0] * 25
    scores = list(np.linspace(0.3, 0.7, 25))
    dets[4] = kp[:, :2]                                  # the hit has one of the lowest scores
    im = CR.make_image([kp], [box], [AREA], None, dets, scores, [AREA] * 25)
    r = CR.evaluate_image(im, SIG, CR.AREA_RANGES[0])
    assert r["dt_index"].tolist() == list(range(24, 4, -1)) and not r["dt_matched"].any()
    assert _stats([im])["AP"] == 0.0
    assert CR.evaluate_image(im, SIG, CR.AREA_RANGES[0], max_dets=21)["dt_matched"][0, 20]


def duplicate_gt_image():
    kp, box = _person()
    return CR.make_image([kp, kp.copy()], [box, box], [AREA, AREA], None, [_shifted(kp, 0.9)], [0.9], [AREA])


def test_identical_ground_truths_the_later_one_is_taken():
    r = CR.evaluate_image(duplicate_gt_image(), SIG, CR.AREA_RANGES[0])
    assert r["oks"][0, 0] == r["oks"][0, 1]
    assert r["gt_matched"][0].tolist() == [False, True]


def equal_score_images():
    """Two images, one ground truth each; every detection has score 0.5.  Image 0: a miss, then the hit.  Image 1: the
    hit, then a miss.  In input order the sorted list is miss, hit, hit, miss."""
    out = []
    for i, hit_first in enumerate((False, True)):
        kp, box = _person(seed=i)
        dets = [kp[:, :2], kp[:, :2] + 3000.0]
        out.append(CR.make_image([kp], [box], [AREA], None, dets if hit_first else dets[::-1], [0.5, 0.5],
                                 [AREA, AREA]))
    return out


def test_equal_scores_keep_input_order():
    ims = equal_score_images()
    r = CR.evaluate_image(ims[0], SIG, CR.AREA_RANGES[0])
    assert r["dt_index"].tolist() == [0, 1] and r["dt_matched"][0].tolist() == [False, True]
    p, rc = CR.accumulate([CR.evaluate_image(im, SIG, CR.AREA_RANGES[0]) for im in ims])
    # tp/fp along miss, hit, hit, miss: precision 0, 1/2, 2/3, 2/4 -> envelope 2/3; recall reaches 1
    assert abs(p[0, 0] - 2 / 3) < 1e-12 and abs(p[0, 100] - 2 / 3) < 1e-12 and rc[0] == 1.0
    # the other image order: hit, miss, miss, hit: precision 1 up to recall 0.5, then 0.5
    p2, _ = CR.accumulate([CR.evaluate_image(im, SIG, CR.AREA_RANGES[0]) for im in ims[::-1]])
    assert abs(p2[0, 50] - 1.0) < 1e-12 and abs(p2[0, 51] - 0.5) < 1e-12


def test_empty_images():
    kp, box = _person()
    no_dets = CR.make_image([kp], [box], [AREA])
    no_gts = CR.make_image(None, None, None, None, [kp[:, :2]], [0.9], [AREA])
    nothing = CR.make_image()
    s = _stats([no_dets])
    assert s["AP"] == 0.0 and s["AR"] == 0.0 and s["APl"] == -1.0
    s = _stats([no_gts, nothing])
    assert all(s[k] == -1.0 for k in CR.STATS)
    hit = CR.make_image([kp], [box], [AREA], None, [kp[:, :2]], [0.5], [AREA])
    s = _stats([no_dets, no_gts, nothing, hit])          # 2 ground truths, one found behind a false positive
    assert abs(s["AR"] - 0.5) < 1e-12
    assert abs(s["AP"] - 0.5 * 51 / 101) < 1e-12         # precision 1/2 at the 51 recall levels up to 0.5, then 0
    assert all(v == -1.0 for k, v in _stats([]).items() if k in CR.STATS)


def early_stop_image():
    """A non-ignored ground truth with OKS 0.7 and a crowd with OKS 0.9: the walk must stop at the crowd once the
    non-ignored one is held, or the detection is swallowed by the crowd and the ground truth is never found."""
    kp, box = _person()
    crowd, cbox = _person(seed=5)
    det = _shifted(kp, 0.7)
    # the crowd's keypoints are the detection's, shifted: OKS(det, crowd) = 0.9
    crowd[:, :2] = det
    crowd[:, 0] -= CR.shift_for_oks(0.9, 0.05, AREA)
    return CR.make_image([kp, crowd], [box, cbox], [AREA, AREA], [False, True], [det], [0.9], [AREA])


def envelope_images():
    """miss, hit, hit over two ground truths: precision 0, 1/2, 2/3 rises, so the envelope lifts the front."""
    out = []
    for i in range(2):
        kp, box = _person(seed=i)
        dets = [kp[:, :2] + 3000.0, kp[:, :2]] if i == 0 else [kp[:, :2]]
        out.append(CR.make_image([kp], [box], [AREA], None, dets, [0.9, 0.8] if i == 0 else [0.7],
                                 [AREA] * len(dets)))
    return out


def tie_images():
    """Two ground truths mirrored about detection 1 (integer coordinates: c - 5 and c + 5 against c, so both OKS are
    the same bits, exp(-0.25) = 0.78), and detection 2 exactly on ground truth 0 (OKS 1 with it, exp(-1) = 0.37 with
    the other).  Later-wins: detection 1 takes ground truth 1 and leaves 0 to detection 2: two hits.  First-wins:
    detection 1 takes ground truth 0 and detection 2 finds nothing."""
    rng = np.random.default_rng(2)
    c = rng.integers(100, 200, (K, 2)).astype(np.float64)
    g0, g1 = np.concatenate([c, np.full((K, 1), 2.0)], axis=1), np.concatenate([c, np.full((K, 1), 2.0)], axis=1)
    g0[:, 0] -= 5.0
    g1[:, 0] += 5.0
    box = (100.0, 100.0, 100.0, 100.0)
    return [CR.make_image([g0, g1], [box, box], [AREA, AREA], None, [c, g0[:, :2]], [0.9, 0.8], [AREA, AREA])]


def test_the_gauge_rejects_three_mutations():
    # first index wins on ties: AP50 drops from 1 to 51 / 101 (one hit, then a false positive: recall stops at 0.5)
    ims = tie_images()
    r = CR.evaluate_image(ims[0], SIG, CR.AREA_RANGES[0])
    assert r["oks"][0, 0] == r["oks"][0, 1] and abs(r["oks"][0, 0] - np.exp(-0.25)) < 1e-12
    assert r["oks"][1, 0] == 1.0 and abs(r["oks"][1, 1] - np.exp(-1.0)) < 1e-12
    good, bad = _stats(ims), _stats(ims, tie_first=True)
    assert abs(good["AP50"] - 1.0) < 1e-12 and abs(good["AR50"] - 1.0) < 1e-12
    assert abs(bad["AP50"] - 51 / 101) < 1e-12 and abs(bad["AR50"] - 0.5) < 1e-12
    # ... and on the bit-identical pair it marks the other ground truth
    im = duplicate_gt_image()
    assert CR.evaluate_image(im, SIG, CR.AREA_RANGES[0], tie_first=True)["gt_matched"][0].tolist() == [True, False]
    # no early stop: the crowd swallows the detection, AP50 and AR50 collapse from 1 to 0
    im = early_stop_image()
    oks = CR.evaluate_image(im, SIG, CR.AREA_RANGES[0])["oks"]
    assert abs(oks[0, 0] - 0.7) < 1e-9 and abs(oks[0, 1] - 0.9) < 1e-9
    good, bad = _stats([im]), _stats([im], early_stop=False)
    assert abs(good["AP50"] - 1.0) < 1e-12 and abs(good["AR50"] - 1.0) < 1e-12
    assert bad["AP50"] == 0.0 and bad["AR50"] == 0.0
    # no envelope: AP50 drops from 2/3 to (0 + 1/2 * 50 + 2/3 * 50) / 101 (recall 0 reads the leading miss)
    ims = envelope_images()
    good, bad = _stats(ims), _stats(ims, envelope=False)
    assert abs(good["AP50"] - 2 / 3) < 1e-12
    assert abs(bad["AP50"] - (0.5 * 50 + (2 / 3) * 50) / 101) < 1e-12


# ------------------------------------------------------------------------------------------------ the module, no device
def _evaluator(**kw):
    from probpose_pytorch_amd import CocoKeypointEval
    return CocoKeypointEval(SIG, **kw)


def test_value_errors_name_the_argument():
    ev = _evaluator()
    kp, box = _person()
    good = dict(image_id=1, keypoints=kp[None], bboxes=[box], areas=[AREA])
    for change, word in ((dict(keypoints=kp[None, :5]), "keypoints"), (dict(keypoints=kp), "keypoints"),
                         (dict(bboxes=[box, box]), "bboxes"), (dict(areas=[AREA, AREA]), "areas"),
                         (dict(iscrowd=[0, 1]), "iscrowd"), (dict(areas=[np.nan]), "areas")):
        with pytest.raises(ValueError, match=word):
            ev.add_ground_truth(**{**good, **change})
    det = dict(image_ids=[1, 1], keypoints=np.zeros((2, K, 2)), scores=np.array([0.5, 0.4]), areas=np.array([1.0, 2.0]))
    for change, word in ((dict(keypoints=np.zeros((2, K + 1, 2))), "keypoints"),
                         (dict(keypoints=np.zeros((2, K, 4))), "keypoints"),
                         (dict(keypoints=np.zeros((3, K, 2))), "keypoints"),
                         (dict(scores=np.array([0.5])), "scores"), (dict(areas=np.zeros((2, 1))), "areas"),
                         (dict(scores=np.array([0.5, np.inf])), "scores"),
                         (dict(scores=np.array([np.nan, 0.1])), "scores"),
                         (dict(image_ids=[[1, 1]]), "image_ids")):
        with pytest.raises(ValueError, match=word):
            ev.add_detections(**{**det, **change})
    ev.add_detections(**{**det, "keypoints": np.zeros((2, K, 3))})        # a third column is accepted
    from probpose_pytorch_amd import CocoKeypointEval
    with pytest.raises(ValueError, match="sigmas"):
        CocoKeypointEval([])
    with pytest.raises(ValueError, match="area_ranges"):
        CocoKeypointEval(SIG, area_ranges=[1.0, 2.0])
    with pytest.raises(ValueError, match="max_dets"):
        CocoKeypointEval(SIG, max_dets=0)


def _coco_files(tmp_path):
    images = [CR.random_image(np.random.default_rng(s), K, G, D) for s, (G, D) in enumerate(((2, 3), (0, 2), (3, 0)))]
    gt = dict(images=[dict(id=10 + i) for i in range(3)], annotations=[], categories=[dict(id=1, name="person")])
    res = []
    for i, im in enumerate(images):
        for g in range(im["gt_kpts"].shape[0]):
            gt["annotations"].append(dict(id=len(gt["annotations"]), image_id=10 + i, category_id=1,
                                          keypoints=im["gt_kpts"][g].reshape(-1).tolist(),
                                          bbox=im["gt_bbox"][g].tolist(), area=float(im["gt_area"][g]),
                                          iscrowd=int(im["gt_crowd"][g])))
        for d in range(im["dt_kpts"].shape[0]):
            k3 = np.concatenate([im["dt_kpts"][d], np.ones((K, 1))], axis=1)
            res.append(dict(image_id=10 + i, category_id=1, keypoints=k3.reshape(-1).tolist(),
                            score=float(im["dt_score"][d])))
    gt["annotations"].append(dict(id=999, image_id=10, category_id=2, keypoints=[0.0] * (3 * K), bbox=[0, 0, 1, 1]))
    res.append(dict(image_id=10, category_id=2, keypoints=[0.0] * (3 * K), score=0.99))
    gpath, rpath = tmp_path / "gt.json", tmp_path / "res.json"
    gpath.write_text(json.dumps(gt))
    rpath.write_text(json.dumps(res))
    return images, gt, res, str(gpath), str(rpath)


def test_json_round_trip(tmp_path):
    from probpose_pytorch_amd import CocoKeypointEval
    images, gt, res, gpath, rpath = _coco_files(tmp_path)
    for source, results in ((gpath, rpath), (gt, res)):
        ev = CocoKeypointEval.from_coco_json(source, SIG)
        ev.add_results_json(results)
        assert list(ev._index) == [10, 11, 12]
        kp, bb, ar, flags, counts = ev._ground_truth_arrays(3)
        assert counts.tolist() == [2, 0, 3]
        assert kp.tobytes() == np.concatenate([im["gt_kpts"] for im in images]).tobytes()
        assert bb.tobytes() == np.concatenate([im["gt_bbox"] for im in images]).tobytes()
        assert ar.tobytes() == np.concatenate([im["gt_area"] for im in images]).tobytes()
        assert (flags & 1).astype(bool).tolist() == np.concatenate([im["gt_crowd"] for im in images]).tolist()
        (pos, dkp, sc, dar), = ev._dets
        assert pos.tolist() == [0, 0, 0, 1, 1]
        assert dkp.tobytes() == np.concatenate([im["dt_kpts"] for im in images]).tobytes()
        assert sc.tobytes() == np.concatenate([im["dt_score"] for im in images]).tobytes()
        ext = images[0]["dt_kpts"][1].max(axis=0) - images[0]["dt_kpts"][1].min(axis=0)
        assert dar[1] == ext[0] * ext[1]                 # no "area" in the result: the keypoints' bounding extent
    with pytest.raises(ValueError, match="keypoints"):
        ev.add_results_json([dict(image_id=10, category_id=1, keypoints=[0.0] * 5, score=0.5)])
    ev.reset()
    assert not ev._index and not ev._dets and not ev._gts


def test_evaluate_refuses_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from probpose_pytorch_amd import _lib
    ev = _evaluator()
    kp, box = _person()
    ev.add_ground_truth(1, kp[None], [box], [AREA])
    ev.add_detections([1], kp[None, :, :2], [0.9], [AREA])
    with pytest.raises(_lib.HipExtensionError):
        ev.evaluate()


def test_c_abi_refusals_without_a_device(built_lib):
    """Null pointers and offsets that are not monotone are refused on the host with a message; nothing is launched
    (there is no device here to launch on)."""
    L = built_lib
    good = np.array([[0, 2, 5], [0, 1, 4], [0, 2, 11]], dtype=np.int64)
    p = 0x1000

    def oks(offs, n_img=2, K=17, tot=(5, 4, 11), null=None):
        args = [p] * 8
        if null is not None:
            args[null] = None
        return L.pp_cocoeval_oks(n_img, K, *tot, offs.ctypes.data if offs is not None else None, *args, None)

    def match(offs, A=3, T=10, tot=(5, 4, 11), null=None):
        args = [p] * 11
        if null is not None:
            args[null] = None
        return L.pp_cocoeval_match(2, A, T, *tot, offs.ctypes.data if offs is not None else None, *args, None)

    for bad, word in ((np.array([[0, 3, 2], [0, 1, 4], [0, 3, 0]], dtype=np.int64), b"not monotone"),
                      (np.array([[0, 2, 5], [0, 4, 1], [0, 8, -1]], dtype=np.int64), b"not monotone"),
                      (np.array([[0, 2, 5], [0, 1, 4], [0, 3, 11]], dtype=np.int64), b"OKS offsets"),
                      (np.array([[1, 2, 5], [0, 1, 4], [0, 1, 10]], dtype=np.int64), b"start at 0")):
        assert oks(bad) != 0 and word in L.pp_last_error(), L.pp_last_error()
        assert match(bad) != 0 and word in L.pp_last_error(), L.pp_last_error()
    assert oks(good, tot=(6, 4, 11)) != 0 and b"offsets end" in L.pp_last_error()
    assert oks(None) != 0 and b"null host offsets" in L.pp_last_error()
    assert oks(good, K=0) != 0 and b"K=0" in L.pp_last_error()
    assert oks(good, n_img=-1) != 0 and b"n_img" in L.pp_last_error()
    for i in range(8):
        assert oks(good, null=i) != 0 and b"null argument" in L.pp_last_error(), i
    for i in range(11):
        assert match(good, null=i) != 0 and b"null argument" in L.pp_last_error(), i
    assert match(good, A=0) != 0 and b"area ranges" in L.pp_last_error()
    assert match(good, T=0) != 0 and b"thresholds" in L.pp_last_error()
    acc = lambda *a, null=None: L.pp_cocoeval_accumulate(*a, *[None if j == null else p for j in range(9)], None)
    for i in range(9):
        assert acc(5, 3, 10, 101, null=i) != 0 and b"null argument" in L.pp_last_error(), i
    assert acc(-1, 3, 10, 101) != 0 and b"Dtot" in L.pp_last_error()
    assert acc(1 << 31, 3, 10, 101) != 0 and b"Dtot" in L.pp_last_error()
    assert acc(5, 3, 10, 0) != 0 and b"R=0" in L.pp_last_error()
    from probpose_pytorch_amd import _lib
    assert (_lib.PP_COCO_GT_CROWD, _lib.PP_COCO_GT_NO_VISIBLE) == (1, 2)
