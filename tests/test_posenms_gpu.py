"""PoseNMS and rescore_instances on the GPU against the plain-loop float64 gauge of tests/posenms_reference.py.

Bounds (u = 2^-53, the unit roundoff of float64; every OKS lies in [0, 1], every score of the fixtures in (0, 1)):

Rescoring.  The kernel and the gauge add the same float64 values in the same order, divide by the same integer and
multiply once, unfused (-ffp-contract=off), every operation correctly rounded: the same bits.  float32 inputs are
widened exactly on both sides.

OKS.  As in tests/test_cocoeval_gpu.py: the exponent e is the same bits on both sides; exp (1 ulp each side), the sum
of n <= K terms and the division differ: |OKS_kernel - OKS_gauge| <= (2 K + 2) u = c u.

keep / counts.  Exact equality.  Hard mode compares OKS with oks_thr, soft_linear too, and the soft modes compare
current scores with each other.  The fixture conditions, asserted on the gauge's values before anything touches the
device: (1) no pair OKS the gauge evaluates lies within 1e-9 of oks_thr: 1e-9 is 10^5 times c u, so both sides decide
alike; (2) in the soft modes, at every pick the two largest live scores differ by more than 1e-9 relative, which is
5000 times the score bound below, so both sides pick the same detection, and by induction over the picks both sides
apply the same sequence of pivots to every detection.  Excepted from (2) are the scores of bit-identical detections (same keypoints,
visibilities, area and input score: every operation on them has the same operands on either side, so they stay equal to
each other on both sides), and equal scores that are still UNTOUCHED input bits on both sides: no linear factor was applied to them (the decision OKS >= oks_thr is covered by (1)), and
every gaussian factor came from an OKS below 1e-9, whose OKS^2 / oks_thr < 2^-59 makes exp() return exactly 1 in any
implementation that is within an ulp (1 - 2^-59 is 64 times closer to 1 than to its neighbour).  Between such bit-equal
scores the stable rule decides, on both sides alike.  (3) At least 20 % of the detections are suppressed and at least
20 % kept.

scores.  Hard mode: the input bits.  soft_gaussian, one rescoring s <- s * exp(-OKS^2 / oks_thr):
  * x = OKS * OKS / oks_thr: the two OKS differ by c u, their squares by 2 c u; each side rounds the square (u) and the
    quotient (u x <= u / oks_thr): |x_kernel - x_gauge| <= (2 c + 4) u / oks_thr;
  * exp: the true values differ by that much relatively, each side's exp is within 1 ulp <= 2 u relative ... + 4 u;
  * the product: one rounding each side ... + 2 u.
  r = ((2 c + 4) / oks_thr + 6) u per rescoring, compounded over at most n = min(D, max_dets) rescorings (one per
  pick): |s_kernel - s_gauge| <= 1.001 n r s_gauge.  At K = 17, oks_thr = 0.9, n = 20: 2.0e-13.
soft_linear, one rescoring s <- s * (1 - OKS) where OKS >= oks_thr >= 0.5: the subtraction is exact on both sides
  (Sterbenz), so the factors differ by c u ABSOLUTELY (relatively by any amount as OKS -> 1, where the score goes to 0
  with them), the products round once each: the difference grows by at most (c + 2) u s_input per rescoring, factors
  and scores being at most 1 and s_input: |s_kernel - s_gauge| <= n (c + 3) u s_input.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import cocoeval_reference as CR
from tests import posenms_reference as PR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = (0, 1, 2, 3, 63, 64, 65, 130)           # D per image: empty, single lanes, the wave boundary from both sides
SEED = 7
OKS_THR = 0.9
MODE_ID = {"hard": 0, "soft_gaussian": 1, "soft_linear": 2}


def _freeze(images):
    for im in images:
        for a in im.values():
            if a is not None:
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ragged_images(K):
    """One image per size; the image of 65 has a bit-identical pair with one score (detections 0 and 1), the images of
    3, 64 and 130 have three equal scores.  Read-only."""
    rng = np.random.default_rng(SEED + K)
    images = [PR.random_image(rng, K, D, identical=(D == 65), equal_scores=(D in (3, 64, 130))) for D in SIZES]
    _freeze(images)
    return tuple(images)


@functools.lru_cache(maxsize=None)
def gauge(K, mode, vis_thr, max_dets=20):
    return PR.run(ragged_images(K), PR.default_sigmas(K), mode, OKS_THR, vis_thr, max_dets)


def _twins(im, a, b):
    return all(im[k][a].tobytes() == im[k][b].tobytes() for k in ("kpts", "area", "score")) and (
        im["vis"] is None or im["vis"][a].tobytes() == im["vis"][b].tobytes())


def check_fixture(want, mode, images):
    """Conditions (1) - (3) of the module docstring on the gauge's values."""
    for r, im in zip(want["per_image"], images):
        seen = np.asarray(r["oks_seen"], dtype=np.float64)
        assert seen.size == 0 or np.abs(seen - OKS_THR).min() > 1e-9, "a pair OKS sits on the threshold"
        for top, runner, untouched, a, b in r["gaps"]:
            if runner is None:
                continue
            assert (top == runner and (untouched or _twins(im, a, b))) or top - runner > 1e-9 * abs(top), (
                "two live scores coincide", top, runner)
    kept = float(want["keep"].mean())
    if mode == "hard" or want["max_dets"] >= 20:
        assert 0.2 <= kept <= 0.8, kept


def _gauge_checked(K, mode, vis_thr, max_dets=20):
    want = dict(gauge(K, mode, vis_thr, max_dets), max_dets=max_dets)
    check_fixture(want, mode, ragged_images(K))
    return want


def flat(images, with_vis=True, order=None):
    """The images' detections as one batch: ids, keypoints [M, K, 3] (the third column the visibility), scores, areas,
    visibilities; ``order`` permutes the batch."""
    K = images[0]["kpts"].shape[1]
    ids = np.concatenate([np.full(im["kpts"].shape[0], i, dtype=np.int64) for i, im in enumerate(images)])
    kp = np.concatenate([im["kpts"] for im in images])
    vis = np.concatenate([im["vis"] if im["vis"] is not None else np.ones((im["kpts"].shape[0], K)) for im in images])
    sc = np.concatenate([im["score"] for im in images])
    ar = np.concatenate([im["area"] for im in images])
    kp3 = np.concatenate([kp, vis[..., None]], axis=2)
    if order is not None:
        ids, kp3, sc, ar, vis = ids[order], kp3[order], sc[order], ar[order], vis[order]
    return ids, kp3, sc, ar, vis


def nms(K, mode, vis_thr, max_dets=20, **kwargs):
    from probpose_pytorch_amd import PoseNMS
    return PoseNMS(PR.default_sigmas(K), mode=mode, oks_thr=OKS_THR, vis_thr=vis_thr, max_dets=max_dets, **kwargs)


def device_inputs(K, order=None):
    ids, kp3, sc, ar, _ = flat(ragged_images(K), order=order)
    return (ids, torch.from_numpy(kp3).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(ar).cuda()), sc


def run_device(K, mode, vis_thr, max_dets=20, order=None):
    inputs, sc = device_inputs(K, order)
    return nms(K, mode, vis_thr, max_dets)(*inputs), sc


def score_bound(K, mode, max_dets):
    c, n = 2 * K + 2, min(max(SIZES), max_dets)
    if mode == "soft_gaussian":
        return 1.001 * n * ((2 * c + 4) / OKS_THR + 6) * U
    return n * (c + 3) * U


def compare(res, want, sc_in, K, mode, max_dets=20):
    keep, scores, counts = res.keep.cpu().numpy(), res.scores.cpu().numpy(), res.counts.cpu().numpy()
    assert keep.dtype == np.bool_ and scores.dtype == np.float64 and counts.dtype == np.int32
    nonempty = [i for i, D in enumerate(SIZES) if D]
    assert list(res.image_ids) == nonempty
    assert np.array_equal(keep, want["keep"]), np.nonzero(keep != want["keep"])[0]
    assert np.array_equal(counts, want["counts"][nonempty])
    if mode == "hard":
        assert scores.tobytes() == sc_in.tobytes()
        return 0.0
    bound = score_bound(K, mode, max_dets)
    scale = np.abs(want["scores"]) if mode == "soft_gaussian" else np.abs(sc_in)
    ratio = np.abs(scores - want["scores"]) / (bound * scale)
    worst = float(ratio.max())
    print(f"K = {K}, {mode}, max_dets {max_dets}: worst |d score| / bound = {worst:.4f} (bound {bound:.3e}); "
          f"kept {int(keep.sum())} of {keep.size}; rescored {int((want['scores'] != sc_in).sum())}")
    assert worst <= 1.0
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("K", [1, 17])
def test_rescore_is_the_gauge_bit_for_bit(K, dtype):
    """700 instances (three workgroups, the last one partial); row 0 has no keypoint above kpt_thr, row 1 one exactly
    at it (which does not count), row 2 all of them."""
    from probpose_pytorch_amd import rescore_instances
    rng = np.random.default_rng(11 + K)
    ks = rng.uniform(0.0, 1.0, (700, K))
    ks[0] = rng.uniform(0.0, 0.2, K)
    ks[1] = 0.2
    ks[2] = rng.uniform(0.3, 1.0, K)
    bs = rng.uniform(0.05, 1.0, 700)
    ks_t, bs_t = torch.from_numpy(ks).to(dtype), torch.from_numpy(bs).to(dtype)
    kpt_thr = float(torch.tensor(0.2, dtype=dtype)) if dtype == torch.float32 else 0.2
    ks_t[1] = kpt_thr
    want = PR.rescore(ks_t.to(torch.float64).numpy(), bs_t.to(torch.float64).numpy(), kpt_thr)
    got = rescore_instances(ks_t.cuda(), bs_t.cuda(), kpt_thr)
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (700,)
    assert want[0] == 0.0 and want[1] == 0.0 and want[2] > 0.0 and (want > 0).sum() > 500
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert rescore_instances(ks_t[:0].cuda(), bs_t[:0].cuda()).shape == (0,)


@pytest.mark.parametrize("vis_thr", [None, 0.2])
@pytest.mark.parametrize("mode", PR.MODES)
@pytest.mark.parametrize("K", [1, 17])
def test_keep_counts_and_scores_are_the_gauges(K, mode, vis_thr):
    """keep and counts equal the gauge's in every mode, with and without visibilities (the third keypoint column);
    scores are the input bits in hard mode and within the docstring's bound in the soft modes.  In the soft modes the
    kept set is the first max_dets = 20 picks."""
    want = _gauge_checked(K, mode, vis_thr)
    twins = want["per_image"][SIZES.index(65)]
    assert 1.0 in twins["oks_seen"]                                 # copies at jitter level 0: OKS exactly 1
    if (K, mode, vis_thr) == (17, "hard", None):                    # the bit-identical pair with one score: the
        assert twins["keep"][:2].tolist() == [True, False]          # earlier is kept and suppresses the later
    if mode != "hard":
        for r, D in zip(want["per_image"], SIZES):
            assert len(r["picks"]) == min(D, 20) and sorted(r["picks"]) == np.nonzero(r["keep"])[0].tolist()
    res, sc_in = run_device(K, mode, vis_thr)
    compare(res, want, sc_in, K, mode)


@pytest.mark.parametrize("mode", ["soft_gaussian", "soft_linear"])
def test_max_dets_one_keeps_the_first_pick(mode):
    want = _gauge_checked(17, mode, None, max_dets=1)
    assert want["counts"].tolist() == [min(D, 1) for D in SIZES]
    full = gauge(17, mode, None, 20)
    for r1, r20 in zip(want["per_image"], full["per_image"]):
        assert r1["picks"] == r20["picks"][:1]
    res, sc_in = run_device(17, mode, None, max_dets=1)
    compare(res, want, sc_in, 17, mode, max_dets=1)


def test_rescoring_first_and_kpt_scores_as_visibility():
    """With kpt_scores the instances are rescored first and kpt_scores is the visibility: the gauge chain is rescore ->
    nms_image on the rescored scores."""
    K, mode, vis_thr = 17, "hard", 0.2
    images = ragged_images(K)
    ids, kp3, box, ar, vis = flat(images)
    rescored = PR.rescore(vis, box, 0.3)
    cuts = np.cumsum([0] + [im["kpts"].shape[0] for im in images])
    again = [PR.make_image(im["kpts"], rescored[a:b], im["area"], im["vis"]) for im, a, b in zip(images, cuts, cuts[1:])]
    want = dict(PR.run(again, PR.default_sigmas(K), mode, OKS_THR, vis_thr), max_dets=20)
    check_fixture(want, mode, again)
    res = nms(K, mode, vis_thr, kpt_thr=0.3)(ids, torch.from_numpy(kp3[..., :2].copy()).cuda(),
                                             torch.from_numpy(box).cuda(), torch.from_numpy(ar).cuda(),
                                             kpt_scores=torch.from_numpy(vis).cuda())
    compare(res, want, rescored, K, mode)
    assert res.scores.cpu().numpy().tobytes() == rescored.tobytes()


def test_interleaved_images_and_repeatability():
    """The batch with its images interleaved (round robin, every image's own order kept) gives every detection the
    result it has in the grouped batch; two calls return the same bits; a call reads back the finiteness booleans of
    its inputs and nothing else."""
    K, mode, vis_thr = 17, "soft_gaussian", 0.2
    ids = flat(ragged_images(K))[0]
    rank = np.arange(ids.size) - np.concatenate([[0], np.cumsum(np.bincount(ids))])[ids]
    order = np.lexsort((ids, rank))
    assert not np.array_equal(order, np.arange(ids.size)) and (np.diff(ids[order][:12]) != 0).any()
    grouped, _ = run_device(K, mode, vis_thr)
    mixed, _ = run_device(K, mode, vis_thr, order=order)
    assert np.array_equal(mixed.keep.cpu().numpy(), grouped.keep.cpu().numpy()[order])
    assert mixed.scores.cpu().numpy().tobytes() == grouped.scores.cpu().numpy()[order].tobytes()
    first_seen = list(dict.fromkeys(ids[order].tolist()))
    assert list(mixed.image_ids) == first_seen
    by_id = dict(zip(grouped.image_ids, grouped.counts.cpu().numpy().tolist()))
    assert mixed.counts.cpu().numpy().tolist() == [by_id[i] for i in first_seen]

    inputs, _ = device_inputs(K)
    call = nms(K, mode, vis_thr)
    torch.cuda.synchronize()
    sync_mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            again = call(*inputs)
            syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode(sync_mode)
    print(f"PoseNMS call: {len(syncs)} synchronising call(s)")
    for name in ("keep", "scores", "counts"):
        a, b = getattr(again, name).cpu().numpy(), getattr(grouped, name).cpu().numpy()
        assert a.tobytes() == b.tobytes(), name
    assert len(syncs) == 1, [str(w.message) for w in syncs]


@pytest.mark.parametrize("mode", ["hard", "soft_gaussian"])
def test_entry_point_directly_with_empty_images(mode):
    """pp_posenms on offsets that hold images WITHOUT detections (the Python layer never builds those: an image is
    known by its detections), the batch ordered by the gauge's visiting order on the host; the sentinel of an output
    the kernel must not touch stays."""
    from probpose_pytorch_amd import _lib
    K, vis_thr = 17, 0.2
    images = ragged_images(K) + (PR.make_image(np.zeros((0, K, 2)), [], [], np.zeros((0, K))),)
    want = PR.run(images, PR.default_sigmas(K), mode, OKS_THR, vis_thr, 20)
    orders = [np.asarray(r["order"], dtype=np.int64) for r in want["per_image"]]
    off = np.concatenate([[0], np.cumsum([o.size for o in orders])]).astype(np.int64)
    cat = lambda key: np.concatenate([im[key][o] for im, o in zip(images, orders)])
    M = int(off[-1])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
           for a in (off, cat("kpts"), cat("vis"), cat("area"), cat("score"), (PR.default_sigmas(K) * 2) ** 2)]
    out = torch.full((M + 1,), -7.0, dtype=torch.float64, device="cuda")
    keep = torch.full((M + 1,), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(images) + 1,), -5, dtype=torch.int32, device="cuda")
    rc = _lib.lib().pp_posenms(len(images), K, M, off.ctypes.data, *[_lib.ptr(t) for t in dev], MODE_ID[mode],
                               OKS_THR, vis_thr, 20, _lib.ptr(out), _lib.ptr(keep), _lib.ptr(counts),
                               _lib.stream_ptr())
    _lib.check(rc, "pp_posenms")
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == want["counts"].tolist() + [-5] and want["counts"][0] == 0
    assert float(out[M]) == -7.0 and int(keep[M]) == 9
    got_keep = keep[:M].cpu().numpy().astype(bool)
    assert np.array_equal(got_keep, np.concatenate([r["keep"][o] for r, o in zip(want["per_image"], orders)]))


@functools.lru_cache(maxsize=None)
def eval_batch():
    """16 seeded images with ground truth: detections are jittered copies of the people (several per person) and
    strays, as a detector with overlapping boxes gives them."""
    rng = np.random.default_rng(77)
    images = [CR.random_image(rng, 17, int(rng.integers(1, 5)), int(rng.integers(6, 20)), crowd_p=0.0)
              for _ in range(16)]
    _freeze(images)
    return tuple(images)


def test_end_to_end_into_the_evaluator():
    """PoseNMS (device tensors) -> boolean index -> CocoKeypointEval.add_detections -> evaluate() against
    posenms_reference.run -> survivors -> cocoeval_reference.evaluate: every stat within the evaluator's bound, and
    the AP with NMS above the AP without it."""
    from probpose_pytorch_amd import CocoKeypointEval, PoseNMS
    from tests.test_cocoeval_gpu import STAT_BOUND, check_fixture as check_eval_fixture
    images = eval_batch()
    sig = CR.default_sigmas(17)
    as_nms = [PR.make_image(im["dt_kpts"], im["dt_score"], im["dt_area"]) for im in images]
    want_nms = dict(PR.run(as_nms, sig, "hard", OKS_THR), max_dets=20)
    check_fixture(want_nms, "hard", as_nms)
    survivors = []
    for im, r in zip(images, want_nms["per_image"]):
        s = dict(im)
        s.update(dt_kpts=im["dt_kpts"][r["keep"]], dt_score=im["dt_score"][r["keep"]], dt_area=im["dt_area"][r["keep"]])
        survivors.append(s)
    want, raw = CR.evaluate(survivors, sig), CR.evaluate(list(images), sig)
    check_eval_fixture(want["per_image"][0], survivors)
    print(f"gauge: AP {raw['AP']:.6f} without NMS, {want['AP']:.6f} with; kept {int(want_nms['keep'].sum())} of "
          f"{want_nms['keep'].size}")
    assert want["AP"] > raw["AP"]

    ids = np.concatenate([np.full(im["dt_kpts"].shape[0], i, dtype=np.int64) for i, im in enumerate(images)])
    kp = torch.from_numpy(np.concatenate([im["dt_kpts"] for im in images])).cuda()
    sc = torch.from_numpy(np.concatenate([im["dt_score"] for im in images])).cuda()
    ar = torch.from_numpy(np.concatenate([im["dt_area"] for im in images])).cuda()

    def evaluate(ids, kp, sc, ar):
        ev = CocoKeypointEval(sig)
        for i, im in enumerate(images):
            ev.add_ground_truth(i, im["gt_kpts"], im["gt_bbox"], im["gt_area"], im["gt_crowd"])
        ev.add_detections(ids, kp, sc, ar)
        return ev.evaluate()

    res = PoseNMS(sig, mode="hard", oks_thr=OKS_THR)(ids, kp, sc, ar)
    keep = res.keep
    got = evaluate(ids[keep.cpu().numpy()], kp[keep], res.scores[keep], ar[keep])
    got_raw = evaluate(ids, kp, sc, ar)
    worst = max(abs(got[k] - want[k]) for k in CR.STATS)
    print(f"device: AP {got_raw['AP']:.6f} without NMS, {got['AP']:.6f} with; worst |d stat| {worst:.3e} = "
          f"{worst / STAT_BOUND:.4f} of the bound")
    assert worst <= STAT_BOUND and got["AP"] > got_raw["AP"]


def test_python_refusals():
    from probpose_pytorch_amd import PoseNMS, rescore_instances
    K = 3
    nms3 = PoseNMS(np.full(K, 0.05))
    M = 4097
    kp = torch.zeros((M, K, 2), device="cuda")
    ones = torch.ones(M, device="cuda")
    ids = np.zeros(M, dtype=np.int64)
    ids[0] = 12
    ids[1:] = 34
    with pytest.raises(ValueError, match="image 12 has 4097 detections"):
        nms3(np.full(M, 12), kp, ones, ones)
    assert int(nms3(ids, kp, ones, ones).counts.sum()) == 2                 # 1 + 4096 fit: all identical, one kept each
    kp, ones, ids = kp[:5], ones[:5], [7, 7, 8, 8, 8]
    with pytest.raises(ValueError, match="either all device tensors or all host arrays"):
        nms3(ids, kp, ones.cpu(), ones)
    with pytest.raises(ValueError, match="either all device tensors or all host arrays"):
        nms3(ids, kp, ones, ones, kpt_scores=np.ones((5, K)))
    bad = ones.clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="box_scores: non-finite values"):
        nms3(ids, kp, bad, ones)
    with pytest.raises(ValueError, match="areas: non-finite values"):
        nms3(ids, kp, ones, bad * float("inf"))
    with pytest.raises(ValueError, match="vis_thr: needs visibilities"):
        PoseNMS(np.full(K, 0.05), vis_thr=0.2)(ids, kp, ones, ones)
    with pytest.raises(ValueError, match="keypoints: expected"):
        nms3(ids, kp[:, :2], ones, ones)
    with pytest.raises(ValueError, match="box_scores: expected a float dtype"):
        nms3(ids, kp, ones.long(), ones)
    with pytest.raises(ValueError, match="box_scores: expected \\[5\\]"):
        rescore_instances(torch.ones((5, K), device="cuda"), ones[:4])
    for kwargs in (dict(mode="softest"), dict(oks_thr=0.0), dict(oks_thr=1.5), dict(max_dets=0)):
        with pytest.raises(ValueError):
            PoseNMS(np.full(K, 0.05), **kwargs)
