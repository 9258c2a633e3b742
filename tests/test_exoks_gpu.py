"""CocoKeypointEval(ex_oks=True) on the GPU against the plain-loop float64 gauge of tests/exoks_reference.py.

Bounds (u = 2^-53; Ex-OKS and every precision / recall value lie in [0, 1]), restated from tests/test_cocoeval_gpu.py
with what Ex-OKS changes:

Ex-OKS.  Of the four kinds of term two are exact on both sides: 0 (missed) is not added or added as +0.0, 1 (reported
absent) is the same float64.  The other two are exp(-e): for "both" e = (dx^2 + dy^2) / (2 sigma)^2 / (area + eps) / 2
is the plain kernel's expression, for a false positive e = b b / (2 sigma)^2 / (area + eps) / 2 with b a max / min of
differences of the same inputs (max and min are exact); kernel and gauge evaluate either with the same operations in
the same order, unfused, so e is the same bits on both sides.  What differs, over the n <= K annotated keypoints:
  * exp(-e): each side within 1 ulp of the true value, a value in (0, 1] has ulp <= u ... 2 u per term, 2 u on the mean;
  * the sum of n terms in [0, 1]: n - 1 roundings of at most u * (partial sum) each side, partial sums <= n, after the
    division by n at most (n - 1) u each ... 2 (n - 1) u (an exact term still costs the rounding of its addition);
  * the division by n: one rounding each ... 2 u.
  |ExOKS_kernel - ExOKS_gauge| <= (2 n + 2) u <= (2 K + 2) u.
The fixture keeps e < 29 in every case (asserted on the gauge), where both exp implementations state 1 ulp.

Flags.  Exact equality, under the condition tests/test_cocoeval_gpu.check_fixture states, asserted on the gauge's
Ex-OKS before anything runs on the device (the seeds were chosen in tests/test_exoks_reference.py so that it holds).

evaluate().  As in tests/test_cocoeval_gpu.py: identical flags give identical integers, precision and recall within
2^-52, the ten stats within STAT_BOUND = 1011 * 2^-52.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cocoeval_reference as CR
from tests import exoks_reference as XR
from tests.test_cocoeval_gpu import STAT_BOUND, check_fixture

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def images_of(name, K=17, all_inside=False):
    return XR.ragged_images(K, all_inside) if name == "ragged" else XR.batch64()


@functools.lru_cache(maxsize=None)
def gauge(name, K=17, max_dets=20):
    return XR.evaluate(images_of(name, K), CR.default_sigmas(K), max_dets=max_dets)


def evaluator(K=17, max_dets=20, ex_oks=True, **kw):
    from probpose_pytorch_amd import CocoKeypointEval
    return CocoKeypointEval(CR.default_sigmas(K), max_dets=max_dets, ex_oks=ex_oks, **kw)


def feed(ev, images, device=False, pieces=1, presence_dtype=torch.float32):
    """Ground truths image by image with their windows, detections in `pieces` calls; as device tensors the presence
    is `presence_dtype` (the fixture's values are float32 values).  A plain evaluator gets neither."""
    ex = ev.ex_oks
    for i, im in enumerate(images):
        ev.add_ground_truth(i, im["gt_kpts"], im["gt_bbox"], im["gt_area"], im["gt_crowd"],
                            **(dict(windows=im["gt_window"]) if ex else {}))
    ids = np.concatenate([np.full(im["dt_kpts"].shape[0], i, dtype=np.int64) for i, im in enumerate(images)])
    kp, sc, ar, pr = (np.concatenate([im[k] for im in images]) for k in ("dt_kpts", "dt_score", "dt_area",
                                                                          "dt_presence"))
    cuts = np.linspace(0, len(ids), pieces + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if device:
            extra = dict(presence=torch.from_numpy(pr[a:b]).to(presence_dtype).cuda()) if ex else {}
            ev.add_detections(ids[a:b], torch.from_numpy(kp[a:b]).cuda(), torch.from_numpy(sc[a:b]).cuda(),
                              torch.from_numpy(ar[a:b]).cuda(), **extra)
        else:
            ev.add_detections(ids[a:b], kp[a:b], sc[a:b], ar[a:b], **(dict(presence=pr[a:b]) if ex else {}))
    return ev


def device_stages(images, K, max_dets):
    """Ex-OKS matrices per image, flags and npig from the three stages of the evaluator, as numpy."""
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


@pytest.mark.parametrize("K", [1, 17, 133])
def test_exoks_matrices_against_the_gauge(K):
    """|ExOKS_kernel - ExOKS_gauge| <= (2 K + 2) 2^-53 on the ragged batch, every detection kept (D = 33 > 20)."""
    images = images_of("ragged", K)
    want = gauge("ragged", K, 64)
    info = want["info"]
    assert all(info[c] > 0 for c in XR.CASES) and info["e_max"] < 29.0, info
    per_image, *_ = device_stages(images, K, max_dets=64)
    bound = (2 * K + 2) * U
    worst, seen = 0.0, 0
    for got, r, (D, G) in zip(per_image, want["per_image"][0], XR.RAGGED):
        assert got.shape == r["oks"].shape == (D, G)
        if got.size:
            worst = max(worst, float(np.abs(got - r["oks"]).max()) / bound)
            seen += got.size
    print(f"K = {K}: {seen} Ex-OKS values, worst d / bound = {worst:.4f} (bound {bound:.3e}); cases {info}")
    assert seen == sum(d * g for d, g in XR.RAGGED)
    assert worst <= 1.0


@pytest.mark.parametrize("name,max_dets", [("ragged", 64), ("batch64", 20)])
def test_flags_and_npig_are_the_gauges(name, max_dets):
    """Matched and ignore flags of every (area range, threshold, detection), the matched ground truths and npig: equal
    to the gauge's, 3 area ranges x 10 thresholds, K = 17; max_dets = 20 cuts some image of the 64."""
    images = images_of(name)
    want = gauge(name, 17, max_dets)["per_image"]
    check_fixture(want[0], images)
    cut = any(r["dt_index"].size == 20 and im["dt_score"].size > 20 for r, im in zip(want[0], images))
    assert cut or name == "ragged"
    _, dt_matched, dt_ignore, gt_matched, npig, offs = device_stages(images, 17, max_dets)
    for a in range(3):
        assert int(npig[a]) == sum(r["npig"] for r in want[a]), a
        for i, r in enumerate(want[a]):
            d0, d1, g0, g1 = offs[0, i], offs[0, i + 1], offs[1, i], offs[1, i + 1]
            assert d1 - d0 == r["dt_matched"].shape[1]
            assert np.array_equal(dt_matched[a, :, d0:d1], r["dt_matched"]), (a, i)
            assert np.array_equal(dt_ignore[a, :, d0:d1], r["dt_ignore"]), (a, i)
            assert np.array_equal(gt_matched[a, :, g0:g1], r["gt_matched"]), (a, i)
    assert dt_matched[0].any() and not dt_matched[0].all()


def _compare(got, want):
    worst_pr = float(np.abs(got["precision"] - want["precision"]).max())
    worst_rc = float(np.abs(got["recall"] - want["recall"]).max())
    worst_stat = max(abs(got[k] - want[k]) for k in CR.STATS)
    return worst_pr, worst_rc, worst_stat


@pytest.mark.parametrize("device", [False, True])
def test_evaluate_end_to_end(device):
    """The 64-image batch and the ragged batch through evaluate(), detections as numpy arrays and as device tensors
    with float32 presence: precision and recall within 2^-52 of the gauge's, the ten stats within 1011 * 2^-52, the
    same keys as the plain mode."""
    for name in ("batch64", "ragged"):
        want = gauge(name)
        got = feed(evaluator(), images_of(name), device=device).evaluate()
        assert sorted(got) == sorted(CR.STATS + ("precision", "recall"))
        assert got["precision"].shape == (10, 101, 3) and got["recall"].shape == (10, 3)
        assert all(isinstance(got[k], float) for k in CR.STATS)
        pr, rc, st = _compare(got, want)
        print(f"{name}, device tensors {device}: worst |d| precision {pr:.3e}, recall {rc:.3e}; stats {st:.3e} = "
              f"{st / STAT_BOUND:.4f} of the bound; AP {got['AP']:.6f} AR {got['AR']:.6f}")
        assert pr <= 2.0 ** -52 and rc <= 2.0 ** -52 and st <= STAT_BOUND
    assert 0.05 < gauge("batch64")["AP"] < 0.95


@pytest.mark.parametrize("K", [1, 17, 133])
def test_all_inside_and_present_is_the_plain_path_bit_for_bit(K):
    """Windows that hold every keypoint and presence 1: the Ex-OKS kernel's matrices are the plain kernel's bits, and
    so are the ten stats, precision and recall."""
    images = images_of("ragged", K, True)
    ex, plain = feed(evaluator(K, 64), images), feed(evaluator(K, 64, ex_oks=False), images)
    be, bp = ex._device_batch(), plain._device_batch()
    assert "dt_presence" not in bp and "gt_window" not in bp
    assert be["dt_presence"].shape == (be["Dtot"], K) and be["gt_window"].shape == (be["Gtot"], 4)
    oe, op = ex._oks(be), plain._oks(bp)
    assert be["oks_total"] == sum(d * g for d, g in XR.RAGGED) and torch.equal(oe, op)
    re, rp = ex.evaluate(), plain.evaluate()
    assert all(re[k] == rp[k] for k in CR.STATS)
    assert re["precision"].tobytes() == rp["precision"].tobytes() and re["recall"].tobytes() == rp["recall"].tobytes()
    # a threshold of 0 or 1 changes nothing while every presence is 1
    for thr in (0.0, 1.0):
        e2 = feed(evaluator(K, 64, presence_threshold=thr), images)
        assert torch.equal(e2._oks(e2._device_batch()), op)


def test_the_mode_and_the_threshold_matter():
    """On the ragged batch Ex-OKS and plain OKS give different stats (each as its gauge says), and so does another
    presence threshold; the cut to max_dets takes the presence rows along (a wrong row would move the stats)."""
    images = images_of("ragged")
    want_plain = CR.evaluate(images, CR.default_sigmas(17))
    want_low = XR.evaluate(images, CR.default_sigmas(17), tau=0.25)
    for want in (want_plain, want_low):
        check_fixture(want["per_image"][0], images)
    ex = feed(evaluator(), images).evaluate()
    plain = feed(evaluator(ex_oks=False), images).evaluate()
    assert _compare(plain, want_plain)[2] <= STAT_BOUND
    assert _compare(ex, gauge("ragged"))[2] <= STAT_BOUND
    moved = max(abs(ex[k] - plain[k]) for k in CR.STATS)
    print(f"AP plain {plain['AP']:.4f}, Ex-OKS {ex['AP']:.4f}; largest move of a stat {moved:.4f}")
    assert moved > 1e-3
    low = feed(evaluator(presence_threshold=0.25), images).evaluate()
    assert _compare(low, want_low)[2] <= STAT_BOUND
    assert max(abs(ex[k] - low[k]) for k in CR.STATS) > 1e-3


def _bits(res):
    return res["precision"].tobytes() + res["recall"].tobytes() + np.array([res[k] for k in CR.STATS]).tobytes()


def test_repeatability():
    """Two evaluate() calls give equal bytes; so do detections added in three calls, device tensors with float32 or
    float64 presence, and a reset() followed by the same adds."""
    ev = feed(evaluator(), images_of("batch64"))
    first = _bits(ev.evaluate())
    assert _bits(ev.evaluate()) == first
    assert _bits(feed(evaluator(), images_of("batch64"), pieces=3).evaluate()) == first
    assert _bits(feed(evaluator(), images_of("batch64"), device=True, pieces=2).evaluate()) == first
    assert _bits(feed(evaluator(), images_of("batch64"), device=True, presence_dtype=torch.float64).evaluate()) == first
    ev.reset()
    assert _bits(feed(ev, images_of("batch64")).evaluate()) == first


def test_device_presence_is_checked_in_the_one_readback():
    """A device presence tensor with a NaN or a value outside [0, 1] is refused when it is added, and nothing is
    kept of the call."""
    ev = evaluator()
    kp = torch.zeros((2, 17, 2), dtype=torch.float64, device="cuda")
    sc, ar = torch.tensor([0.5, 0.4], device="cuda"), torch.tensor([1.0, 2.0], device="cuda")
    for value in (float("nan"), float("inf"), -0.01, 1.01):
        pr = torch.full((2, 17), 0.5, dtype=torch.float32, device="cuda")
        pr[1, 3] = value
        with pytest.raises(ValueError, match="presence"):
            ev.add_detections([1, 1], kp, sc, ar, presence=pr)
    with pytest.raises(ValueError, match="presence"):           # host presence with device keypoints
        ev.add_detections([1, 1], kp, sc, ar, presence=np.full((2, 17), 0.5))
    with pytest.raises(ValueError, match="presence"):
        ev.add_detections([1, 1], kp.cpu().numpy(), sc.cpu().numpy(), ar.cpu().numpy(),
                          presence=torch.full((2, 17), 0.5, device="cuda"))
    assert not ev._dets and not ev._presence
    ev.add_detections([1, 1], kp, sc, ar, presence=torch.full((2, 17), 0.5, dtype=torch.float32, device="cuda"))
    assert ev._presence[0].is_cuda and ev._presence[0].dtype == torch.float64


def test_c_abi_refusals_launch_nothing():
    """A null pointer, a threshold outside [0, 1] and offsets that are not monotone come back as errors before any
    launch: the output buffer keeps its sentinel; with the arguments right it is written."""
    from probpose_pytorch_amd import _lib
    L = _lib.lib()
    ev = feed(evaluator(), images_of("ragged")[2:4])
    b = ev._device_batch()
    oks = torch.full((b["oks_total"],), -7.0, dtype=torch.float64, device="cuda")
    variances = torch.from_numpy((ev.sigmas * 2) ** 2).cuda()
    p = _lib.ptr

    def run(host_offs, thr=0.5, null=None):
        args = [p(b[k]) for k in ("offs", "dt_kpts", "gt_kpts", "gt_bbox", "gt_area", "gt_flags")]
        args += [p(variances), p(b["dt_presence"]), p(b["gt_window"]), p(oks)]
        if null is not None:
            args[null] = None
        return L.pp_cocoeval_exoks(b["n_img"], 17, b["Dtot"], b["Gtot"], b["oks_total"], host_offs.ctypes.data,
                                   *args[:9], thr, args[9], _lib.stream_ptr())

    good = b["offs_host"]
    swapped = good.copy()
    swapped[0, 1], swapped[0, 2] = good[0, 2], good[0, 1]
    assert run(swapped) != 0 and b"not monotone" in L.pp_last_error()
    for i in range(10):
        assert run(good, null=i) != 0 and b"null argument" in L.pp_last_error()
    for thr in (-0.5, 1.5, float("nan")):
        assert run(good, thr=thr) != 0 and b"presence_thr" in L.pp_last_error()
    torch.cuda.synchronize()
    assert bool((oks == -7.0).all())
    assert run(good) == 0, L.pp_last_error()
    torch.cuda.synchronize()
    assert bool((oks >= 0).all()) and bool((oks <= 1).all())


@pytest.mark.parametrize("ex_oks", [True, False])
def test_command_line(tmp_path, ex_oks):
    """python -m probpose_pytorch_amd.cocoeval as a child process on JSON files of the ragged batch: one JSON object
    on stdout, the ten stats, each within STAT_BOUND of the gauge's; with --ex-oks the windows are the images'
    (0, 0, width, height), without it the plain stats."""
    images = images_of("ragged")
    sizes = XR.image_sizes(images)
    if ex_oks:
        windowed = XR.with_image_windows(images, sizes)
        want = XR.evaluate(windowed, CR.COCO17_SIGMAS, tau=0.5)
        check_fixture(want["per_image"][0], windowed)
        extra = ["--ex-oks", "--presence-thr", "0.5"]
    else:
        want = CR.evaluate(images, CR.COCO17_SIGMAS)
        check_fixture(want["per_image"][0], images)
        extra = []
    _, _, gpath, rpath = XR.coco_files(tmp_path, images, sizes)
    run = subprocess.run([sys.executable, "-m", "probpose_pytorch_amd.cocoeval", gpath, rpath, "--sigmas", "coco17",
                          "--category-id", "1", "--max-dets", "20", *extra], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout)                    # nothing else on stdout
    assert sorted(got) == sorted(CR.STATS)
    worst = max(abs(got[k] - want[k]) for k in CR.STATS)
    print(f"{extra}: AP {got['AP']:.6f} (gauge {want['AP']:.6f}), worst |d| of a stat {worst:.3e}")
    assert want["AP"] > 0.05 and worst <= STAT_BOUND
