"""CocoKeypointEval on the GPU against the plain-loop float64 gauge of tests/cocoeval_reference.py.

Bounds (u = 2^-53, the unit roundoff of float64; OKS and every precision / recall value lie in [0, 1]):

OKS.  The kernel and the gauge evaluate e = (dx^2 + dy^2) / (2 sigma)^2 / (area + eps) / 2 with the same operations in
the same order on the same float64 inputs, unfused: e is the same bits on both sides.  What differs, over the n <= K
keypoints that count:
  * exp(-e): each side's exp is within 1 ulp of the true value, and a value in (0, 1] has ulp <= u ... 2 u per term,
    2 u on their mean;
  * the sum of n terms in [0, 1]: n - 1 roundings of at most u * (partial sum) on each side, partial sums <= n, so
    after the division by n at most (n - 1) u each ... 2 (n - 1) u;
  * the division by n: one rounding each ... 2 u.
  |OKS_kernel - OKS_gauge| <= (2 n + 2) u <= (2 K + 2) u = c u with c = 2 K + 2.
The fixture keeps e < 29 for every pair (tests/cocoeval_reference.random_image, compact), so every exp argument is in
the range where both exp implementations state 1 ulp.

Flags.  Exact equality.  The matching compares OKS values with thresholds and with each other; the fixture condition
(asserted on the gauge's OKS before anything runs on the device) is that no OKS that can be a candidate, i.e. none above
the lowest threshold minus 1e-9, lies within 1e-9 of a threshold or of another OKS of its detection row, bit-identical
ground truths apart: 1e-9 is 10^5 times the OKS bound above, so both sides order them alike.

evaluate().  With identical flags tp, fp and npig are the same integers.  recall = tp / npig and precision =
tp / ((tp + fp) + eps) are each one or two correctly rounded float64 operations on identical operands: the same bits;
the test allows them one ulp of 1 (2^-52).  A stat is the mean of n <= T R = 1010 such values: the gauge sums them in
a loop, the module pairwise: the two sums differ by at most 2 (n - 1) u n, the means by 2 (n - 1) u, plus the inputs'
2^-52: |stat_module - stat_gauge| <= (n + 1) 2^-52 = 1011 * 2^-52 = 2.3e-13.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import cocoeval_reference as CR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RAGGED = ((0, 3), (3, 0), (1, 1), (20, 7), (33, 2), (5, 70))          # (D, G) per image
STAT_BOUND = 1011 * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def ragged_images(K):
    """The ragged batch: mixed visibilities, a ground truth without visible keypoints (image 3), a crowd (image 3),
    a bit-identical pair of ground truths (image 4), equal scores (image 5).  Read-only."""
    rng = np.random.default_rng(100 + K)
    images = []
    for i, (D, G) in enumerate(RAGGED):
        im = CR.random_image(rng, K, G, D, crowd_p=0.1, zero_visible=(i == 3), duplicate_gt=(i == 4),
                             equal_scores=(i == 5), compact=True)
        if i == 3:
            im["gt_crowd"][:] = False
            im["gt_crowd"][2] = True
        images.append(im)
    _freeze(images)
    return tuple(images)


@functools.lru_cache(maxsize=None)
def batch64():
    """64 seeded images, K = 17: 0 - 5 ground truths, 0 - 25 detections (more than max_dets = 20 in some), people of
    small, medium and large area, some crowds; every eighth image has a bit-identical pair of ground truths, every
    eighth equal scores, every sixteenth a ground truth without visible keypoints."""
    rng = np.random.default_rng(2024)
    images = []
    for i in range(64):
        G, D = int(rng.integers(0, 6)), int(rng.integers(0, 26))
        if i % 8 == 3:
            G = max(G, 2)
        images.append(CR.random_image(rng, 17, G, D, crowd_p=0.15, zero_visible=(i % 16 == 5),
                                      duplicate_gt=(i % 8 == 3), equal_scores=(i % 8 == 6)))
    _freeze(images)
    return tuple(images)


def _freeze(images):
    for im in images:
        for a in im.values():
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def gauge(name, K=17, max_dets=20):
    images = ragged_images(K) if name == "ragged" else batch64()
    return CR.evaluate(images, CR.default_sigmas(K), max_dets=max_dets)


def feed(ev, images, device=False, pieces=1):
    """Ground truths image by image (an image without any is registered too), detections in `pieces` calls."""
    for i, im in enumerate(images):
        ev.add_ground_truth(i, im["gt_kpts"], im["gt_bbox"], im["gt_area"], im["gt_crowd"])
    ids = np.concatenate([np.full(im["dt_kpts"].shape[0], i, dtype=np.int64) for i, im in enumerate(images)])
    kp = np.concatenate([im["dt_kpts"] for im in images])
    sc = np.concatenate([im["dt_score"] for im in images])
    ar = np.concatenate([im["dt_area"] for im in images])
    cuts = np.linspace(0, len(ids), pieces + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if device:
            ev.add_detections(ids[a:b], torch.from_numpy(kp[a:b]).cuda(), torch.from_numpy(sc[a:b]).cuda(),
                              torch.from_numpy(ar[a:b]).cuda())
        else:
            ev.add_detections(ids[a:b], kp[a:b], sc[a:b], ar[a:b])
    return ev


def evaluator(K=17, max_dets=20):
    from probpose_pytorch_amd import CocoKeypointEval
    return CocoKeypointEval(CR.default_sigmas(K), max_dets=max_dets)


def device_stages(images, K, max_dets):
    """OKS matrices per image, flags and npig from the three stages of the evaluator, as numpy."""
    ev = feed(evaluator(K, max_dets), images)
    b = ev._device_batch()
    oks = ev._oks(b)
    gt_matched, dt_matched, dt_ignore, npig = ev._match(b, oks)
    A, T = 3, 10
    offs = b["offs_host"]
    oks = oks.cpu().numpy()
    per_image = [oks[offs[2, i]:offs[2, i + 1]].reshape(offs[0, i + 1] - offs[0, i], offs[1, i + 1] - offs[1, i])
                 for i in range(len(images))]
    shape = lambda t, n: t.cpu().numpy()[:A * T * n].reshape(A, T, n).astype(bool)
    return (per_image, shape(dt_matched, b["Dtot"]), shape(dt_ignore, b["Dtot"]), shape(gt_matched, b["Gtot"]),
            npig.cpu().numpy(), offs)


def check_fixture(results, images):
    """The condition on the fixture (see the module docstring), on the gauge's float64 OKS."""
    thr = np.minimum(CR.OKS_THRESHOLDS, 1 - 1e-10)
    for r, im in zip(results, images):
        G = im["gt_kpts"].shape[0]
        twins = {(a, b) for a in range(G) for b in range(a + 1, G)
                 if im["gt_kpts"][a].tobytes() == im["gt_kpts"][b].tobytes() and im["gt_area"][a] == im["gt_area"][b]
                 and im["gt_bbox"][a].tobytes() == im["gt_bbox"][b].tobytes()}
        for row in r["oks"]:
            cand = [g for g in range(G) if row[g] > thr[0] - 1e-9]
            for g in cand:
                assert np.abs(row[g] - thr).min() > 1e-9, ("an OKS sits on a threshold", row[g])
            for i, a in enumerate(cand):
                for b in cand[i + 1:]:
                    assert (a, b) in twins or abs(row[a] - row[b]) > 1e-9, ("two OKS of a row coincide", row[a], row[b])


@pytest.mark.parametrize("K", [1, 17, 133])
def test_oks_matrices_against_the_gauge(K):
    """|OKS_kernel - OKS_gauge| <= (2 K + 2) 2^-53 on the ragged batch, every detection kept (D = 33 > 20)."""
    images = ragged_images(K)
    per_image, *_ = device_stages(images, K, max_dets=64)
    want = gauge("ragged", K, 64)["per_image"][0]
    bound = (2 * K + 2) * U
    worst, e_max, seen = 0.0, 0.0, 0
    for got, r, im, (D, G) in zip(per_image, want, images, RAGGED):
        assert got.shape == r["oks"].shape == (D, G)
        if got.size:
            worst = max(worst, float(np.abs(got - r["oks"]).max()) / bound)
            seen += got.size
            floor = -np.log(r["oks"].min()) if r["oks"].min() > 0 else np.inf
            e_max = max(e_max, floor)              # mean(exp(-e)) >= exp(-max e): max e >= -ln(OKS) of any pair
    print(f"K = {K}: {seen} OKS values, worst d / bound = {worst:.4f} (bound {bound:.3e}); "
          f"largest -ln(OKS) {e_max:.2f}")
    assert seen == sum(d * g for d, g in RAGGED) and e_max < 29.0
    assert worst <= 1.0


@pytest.mark.parametrize("name,K,max_dets", [("ragged", 17, 64), ("ragged", 133, 64), ("batch64", 17, 20)])
def test_flags_and_npig_are_the_gauges(name, K, max_dets):
    """Matched and ignore flags of every (area range, threshold, detection), the matched ground truths and npig: equal
    to evaluate_image's, for 3 area ranges x 10 thresholds; the duplicated ground truths and the equal scores are in
    both batches."""
    images = ragged_images(K) if name == "ragged" else batch64()
    want = gauge(name, K, max_dets)["per_image"]
    check_fixture(want[0], images)
    cut = any(r["dt_index"].size == 20 and im["dt_score"].size > 20 for r, im in zip(want[0], images))
    assert cut or name == "ragged"                       # max_dets cuts some image of the 64
    _, dt_matched, dt_ignore, gt_matched, npig, offs = device_stages(images, K, max_dets)
    for a in range(3):
        assert int(npig[a]) == sum(r["npig"] for r in want[a]), a
        for i, r in enumerate(want[a]):
            d0, d1, g0, g1 = offs[0, i], offs[0, i + 1], offs[1, i], offs[1, i + 1]
            assert d1 - d0 == r["dt_matched"].shape[1]
            assert np.array_equal(dt_matched[a, :, d0:d1], r["dt_matched"]), (a, i)
            assert np.array_equal(dt_ignore[a, :, d0:d1], r["dt_ignore"]), (a, i)
            assert np.array_equal(gt_matched[a, :, g0:g1], r["gt_matched"]), (a, i)
    # the cases are really in there: a detection that took the LATER of two identical ground truths, an ignored match,
    # an ignored miss
    twin = want[0][4 if name == "ragged" else 3]
    assert twin["oks"][:, 0].tobytes() == twin["oks"][:, 1].tobytes() and twin["gt_matched"][:, 1].any()
    assert dt_ignore[1].any() and (dt_ignore[1] & ~dt_matched[1]).any() and (dt_ignore[1] & dt_matched[1]).any()


def _compare(got, want):
    worst_pr = float(np.abs(got["precision"] - want["precision"]).max())
    worst_rc = float(np.abs(got["recall"] - want["recall"]).max())
    worst_stat = max(abs(got[k] - want[k]) for k in CR.STATS)
    return worst_pr, worst_rc, worst_stat


@pytest.mark.parametrize("device", [False, True])
def test_evaluate_end_to_end(device):
    """The 64-image batch through evaluate(), detections as numpy arrays and as device tensors: precision [T, R, A]
    and recall [T, A] within 2^-52 of the gauge's, the ten stats within 1011 * 2^-52 (module docstring)."""
    want = gauge("batch64")
    got = feed(evaluator(), batch64(), device=device).evaluate()
    assert got["precision"].shape == (10, 101, 3) and got["recall"].shape == (10, 3)
    assert got["precision"].dtype == np.float64 and all(isinstance(got[k], float) for k in CR.STATS)
    pr, rc, st = _compare(got, want)
    print(f"device tensors {device}: worst |d| precision {pr:.3e}, recall {rc:.3e} (bound {2.0 ** -52:.3e}); "
          f"stats {st:.3e} = {st / STAT_BOUND:.4f} of the bound; AP {got['AP']:.6f} APm {got['APm']:.6f} "
          f"APl {got['APl']:.6f} AR {got['AR']:.6f}")
    assert 0.05 < want["AP"] < 0.95 and want["APm"] > -1 and want["APl"] > -1       # a batch that says something
    assert pr <= 2.0 ** -52 and rc <= 2.0 ** -52 and st <= STAT_BOUND


def test_ragged_batch_end_to_end():
    """The ragged batch (images without detections, without ground truths, 70 ground truths in one image, 33
    detections cut to 20) through evaluate()."""
    for K in (1, 133):
        pr, rc, st = _compare(feed(evaluator(K), ragged_images(K)).evaluate(), gauge("ragged", K, 20))
        assert pr <= 2.0 ** -52 and rc <= 2.0 ** -52 and st <= STAT_BOUND, (K, pr, rc, st)


def test_anchor_case_on_the_device():
    """One ground truth, detection A (score 0.9, OKS 0.62), detection B (score 0.8, OKS 0.92): AP 0.6, AP50 1,
    AP75 0.5, AR 0.9 (derived in tests/test_cocoeval_reference.py)."""
    from tests.test_cocoeval_reference import SIG, anchor_image, tie_images, early_stop_image, envelope_images
    from probpose_pytorch_amd import CocoKeypointEval
    got = feed(CocoKeypointEval(SIG), [anchor_image()]).evaluate()
    for k, v in (("AP", 0.6), ("AP50", 1.0), ("AP75", 0.5), ("AR", 0.9), ("APm", 0.6), ("APl", -1.0), ("ARl", -1.0)):
        assert abs(got[k] - v) < 1e-12, (k, got[k])
    # two bit-identical ground truths: the later one is taken (OKS 0.9: at the nine thresholds up to 0.9)
    from tests.test_cocoeval_reference import duplicate_gt_image
    ev = feed(CocoKeypointEval(SIG), [duplicate_gt_image()])
    b = ev._device_batch()
    taken = ev._match(b, ev._oks(b))[0].cpu().numpy()[:60].reshape(3, 10, 2)
    assert taken[0, :8].tolist() == [[0, 1]] * 8 and taken[0, 9].tolist() == [0, 0]
    for a in range(3):      # ("large" ignores both and still marks the later one: an ignored match)
        assert np.array_equal(taken[a], CR.evaluate_image(duplicate_gt_image(), SIG, CR.AREA_RANGES[a])["gt_matched"])
    # the three rules the gauge was shown to tell from their mutations, on the device
    for images, k, v in ((tie_images(), "AP50", 1.0), ([early_stop_image()], "AP50", 1.0),
                         (envelope_images(), "AP50", 2 / 3)):
        assert abs(feed(CocoKeypointEval(SIG), images).evaluate()[k] - v) < 1e-12, (k, v)


def test_unknown_image_ids_and_empty_evaluators():
    """Detections of an image without ground-truth entry are false positives (unless ignored by area); an evaluator
    without ground truth reports -1, one without detections 0."""
    from tests.test_cocoeval_reference import SIG, AREA, _person
    from probpose_pytorch_amd import CocoKeypointEval
    kp, box = _person()
    ev = CocoKeypointEval(SIG)
    ev.add_ground_truth("a", kp[None], [box], [AREA])
    ev.add_detections(["zzz", "a"], np.stack([kp[:, :2], kp[:, :2]]), [0.9, 0.8], [AREA, AREA])
    got = ev.evaluate()
    images = [CR.make_image([kp], [box], [AREA], None, [kp[:, :2]], [0.8], [AREA]),
              CR.make_image(None, None, None, None, [kp[:, :2]], [0.9], [AREA])]
    want = CR.evaluate(images, SIG)
    assert abs(got["AP"] - 0.5) < 1e-12 and _compare(got, want)[2] <= STAT_BOUND
    ev.reset()
    ev.add_detections([1], kp[None, :, :2], [0.9], [AREA])
    assert all(v == -1.0 for k, v in ev.evaluate().items() if k in CR.STATS)
    ev.reset()
    assert all(v == -1.0 for k, v in ev.evaluate().items() if k in CR.STATS)
    ev.add_ground_truth(1, kp[None], [box], [AREA])
    got = ev.evaluate()
    assert got["AP"] == 0.0 and got["AR"] == 0.0 and got["APl"] == -1.0


def _bits(res):
    return res["precision"].tobytes() + res["recall"].tobytes() + np.array([res[k] for k in CR.STATS]).tobytes()


def test_repeatability_and_state():
    """Two evaluate() calls give equal bits; reset() and the same adds give equal bits; detections added in three
    calls equal detections added in one; evaluate() synchronises once."""
    ev = feed(evaluator(), batch64())
    first = _bits(ev.evaluate())
    assert _bits(ev.evaluate()) == first
    ev.reset()
    assert _bits(feed(ev, batch64()).evaluate()) == first
    assert _bits(feed(evaluator(), batch64(), pieces=3).evaluate()) == first
    assert _bits(feed(evaluator(), batch64(), device=True, pieces=2).evaluate()) == first
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            again = _bits(ev.evaluate())
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    print(f"evaluate(): {len(syncs)} synchronising call(s)")
    assert again == first and len(syncs) == 1, [str(w.message) for w in syncs]


def test_c_abi_refusals_launch_nothing():
    """Null pointers and offsets that are not monotone come back as errors with a message before any launch: the
    output buffers keep their sentinel."""
    from probpose_pytorch_amd import _lib
    L = _lib.lib()
    ev = feed(evaluator(), ragged_images(17)[2:4])
    b = ev._device_batch()
    oks = torch.full((b["oks_total"],), -7.0, dtype=torch.float64, device="cuda")
    variances = torch.from_numpy((ev.sigmas * 2) ** 2).cuda()
    flags = torch.full((30 * b["Dtot"],), 9, dtype=torch.uint8, device="cuda")
    flags2 = torch.full((30 * b["Dtot"],), 9, dtype=torch.uint8, device="cuda")
    gtm = torch.full((30 * b["Gtot"],), 9, dtype=torch.uint8, device="cuda")
    npig = torch.full((3,), -5, dtype=torch.int32, device="cuda")
    ranges, thr = torch.from_numpy(ev.area_ranges.copy()).cuda(), torch.from_numpy(ev.oks_thresholds.copy()).cuda()
    p = _lib.ptr

    def run_oks(host_offs, null=None):
        args = [p(b[k]) for k in ("offs", "dt_kpts", "gt_kpts", "gt_bbox", "gt_area", "gt_flags")]
        args += [p(variances), p(oks)]
        if null is not None:
            args[null] = None
        return L.pp_cocoeval_oks(b["n_img"], 17, b["Dtot"], b["Gtot"], b["oks_total"],
                                 None if host_offs is None else host_offs.ctypes.data, *args, _lib.stream_ptr())

    def run_match(host_offs, null=None):
        args = [p(b["offs"]), p(oks), p(b["gt_flags"]), p(b["gt_area"]), p(b["dt_area"]), p(ranges), p(thr), p(gtm),
                p(flags), p(flags2), p(npig)]
        if null is not None:
            args[null] = None
        return L.pp_cocoeval_match(b["n_img"], 3, 10, b["Dtot"], b["Gtot"], b["oks_total"],
                                   None if host_offs is None else host_offs.ctypes.data, *args, _lib.stream_ptr())

    good = b["offs_host"]
    swapped = good.copy()
    swapped[0, 1], swapped[0, 2] = good[0, 2], good[0, 1]                  # detections: 0, 21, 1
    back = good.copy()
    back[1, 1] = good[1, 2] + 1                                           # ground truths run backwards at the end
    for run in (run_oks, run_match):
        for bad in (swapped, back):
            assert run(bad) != 0 and b"not monotone" in L.pp_last_error(), L.pp_last_error()
        assert run(None) != 0 and b"null" in L.pp_last_error()
    for i in range(8):
        assert run_oks(good, null=i) != 0 and b"null argument" in L.pp_last_error()
    for i in range(11):
        assert run_match(good, null=i) != 0 and b"null argument" in L.pp_last_error()
    with pytest.raises(_lib.HipExtensionError, match="not monotone"):
        _lib.check(run_oks(swapped), "pp_cocoeval_oks")
    torch.cuda.synchronize()
    assert bool((oks == -7.0).all()) and bool((flags == 9).all()) and bool((flags2 == 9).all())
    assert bool((gtm == 9).all())
    assert bool((npig == -5).all())
    # and the same buffers are written once the arguments are right
    assert run_oks(good) == 0 and run_match(good) == 0, L.pp_last_error()
    torch.cuda.synchronize()
    assert bool((oks >= 0).all()) and bool((gtm <= 1).all()) and int(npig[0]) > 0
