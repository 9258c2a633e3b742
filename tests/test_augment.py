"""Augmentation of probpose.dataset without a GPU: the parameter draw, the CPU-only worker side, the float64 restatement
(tests/augment_reference.py) against itself where mistakes usually hide, the image-against-keypoint direction with
planted faults, the worker's region against the whole frame, the host half of ``collate`` against the restatement and
the library's host-side argument checks."""
import ctypes as C
import pickle

import numpy as np
import PIL.Image
import pytest
import torch
from torch.utils.data import DataLoader

from tests import augment_reference as AR
from tests import dataset_reference as DR


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DR.write_tree(tmp_path_factory.mktemp("yolo"))


def _dataset(tree, **kw):
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import Augment, YOLOPoseDataset
    aug = Augment(flip_pairs=AR.FLIP_PAIRS, **kw)
    return YOLOPoseDataset(tree.parent, tree.name, Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS)),
                           target_single_class=0, augment=aug)


def _frame(ann):
    with PIL.Image.open(ann["image_path"]) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def test_exports():
    import probpose
    import probpose.dataset
    import probpose_pytorch_amd
    from probpose_pytorch_amd.dataset import Augment
    assert probpose.Augment is Augment and probpose.dataset.Augment is Augment and probpose_pytorch_amd.Augment is Augment
    assert "Augment" in probpose_pytorch_amd.__all__


def test_draw_is_a_pure_function_of_seed_epoch_index():
    from probpose_pytorch_amd.dataset import Augment
    a = Augment(flip_pairs=AR.FLIP_PAIRS, shift=0.1, seed=3)
    first = {(e, i): a.draw(e, i) for e in range(3) for i in range(40)}
    for (e, i) in reversed(list(first)):                         # another order of calls, another instance
        again = Augment(flip_pairs=AR.FLIP_PAIRS, shift=0.1, seed=3).draw(e, i)
        assert again.dtype == np.float64 and again.shape == (7,) and np.array_equal(again, first[e, i])
    p = np.stack(list(first.values()))
    assert len({v.tobytes() for v in first.values()}) == len(first)          # every (epoch, idx) has its own draw
    assert not np.array_equal(Augment(seed=4, shift=0.1).draw(0, 0), first[0, 0])
    assert set(p[:, 0]) == {0.0, 1.0} and 0.3 < p[:, 0].mean() < 0.7
    assert (p[:, 1] >= 0.75).all() and (p[:, 1] <= 1.25).all() and np.ptp(p[:, 1]) > 0.4
    assert (np.abs(p[:, 2]) <= np.radians(40.0)).all() and 0.4 < (p[:, 2] != 0).mean() < 0.8
    assert (np.abs(p[:, 3:5]) <= 0.1).all() and (np.abs(p[:, 5] - 1) <= 0.2).all() and (np.abs(p[:, 6]) <= 0.2).all()
    off = Augment(flip_prob=0.0, scale=(1.0, 1.0), rotate_prob=0.0, brightness=0.0, contrast=0.0).draw(5, 6)
    assert np.array_equal(off, [0, 1, 0, 0, 0, 1, 0])
    with pytest.raises(ValueError):
        Augment(scale=(1.2, 0.8))


def test_unaugmented_items_are_unchanged(tree):
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    plain = YOLOPoseDataset(tree.parent, tree.name, Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS)), 0)
    aug = _dataset(tree)
    with pytest.raises(TypeError):
        YOLOPoseDataset(tree.parent, tree.name, plain.codec, 0, augment=dict(flip_prob=0.5))
    for i in range(len(plain)):
        item = plain[i]
        assert len(item) == 3
        for a, b in zip(item, aug.plain_item(i)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def _identity(samples):
    return samples


def test_samples_do_not_depend_on_workers_or_order_and_the_dataset_pickles(tree):
    ds = _dataset(tree, shift=0.1, seed=11)
    ds.set_epoch(2)
    want = {i: ds[i] for i in reversed(range(len(ds)))}
    for i, s in want.items():
        region, kps, bbox, origin, params = s
        assert region.dtype == np.uint8 and region.flags.c_contiguous and kps.dtype == np.float32
        assert bbox.dtype == np.float64 and origin.dtype == np.int64 and origin.shape == (2,)
        assert np.array_equal(params, ds.augment.draw(2, i)) and not np.array_equal(params, ds.augment.draw(1, i))
    for workers in (0, 2):
        gen = torch.Generator().manual_seed(5)
        seen = []
        for batch in DataLoader(ds, batch_size=4, shuffle=True, num_workers=workers, collate_fn=_identity, generator=gen):
            for s in batch:
                i = [j for j in want if np.array_equal(want[j][2], s[2])][0]
                seen.append(i)
                for a, b in zip(s, want[i]):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (workers, i)
        assert sorted(seen) == list(range(len(ds))) and seen != sorted(seen)
    clone = pickle.loads(pickle.dumps(ds))
    assert clone.augment == ds.augment and clone.epoch == 2
    for a, b in zip(clone[4], want[4]):
        assert np.array_equal(a, b)
    ds.set_epoch(3)
    assert not np.array_equal(ds[4][4], want[4][4])
    with pytest.raises(ValueError, match="persistent"):
        ds.loader(4, num_workers=2, persistent_workers=True)


# ---- the restatement against itself ----------------------------------------------------------------------------------
BOXES = [(100.0, 60.0, 160.0, 200.0), (50.2, 60.7, 300.4, 270.9), (-30.0, -40.0, 150.0, 290.0), (900.5, 100.25, 250.0, 500.0)]


def test_keypoint_matrix_is_the_inverse_of_the_pixel_matrix():
    for box in BOXES:
        for params in AR.PARAM_GRID:
            for size in ((384, 384), (192, 256)):
                origin = AR.region_rect(box, params)[:2]
                prod = AR.matrix_product(box, origin, params, size)
                assert np.abs(prod - np.eye(3)).max() < 1e-12, (box, params, np.abs(prod - np.eye(3)).max())
    # identity parameters: the geometry of the un-augmented scale_box
    box, size = BOXES[1], (384, 384)
    ident = np.array([0, 1, 0, 0, 0, 1, 0.0])
    k = AR.keypoint_matrix(box, ident, size)
    want = np.array([[size[0] / box[2], 0, -box[0] / box[2] * size[0]], [0, size[1] / box[3], -box[1] / box[3] * size[1]]])
    assert np.abs(k - want).max() < 1e-10


def test_flip_is_an_involution_and_bad_pairs_are_refused():
    from probpose_pytorch_amd.dataset import Augment
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    assert np.array_equal(perm[perm], np.arange(DR.K)) and (perm != np.arange(DR.K)).sum() == 16
    assert np.array_equal(Augment(flip_pairs=AR.FLIP_PAIRS).permutation(DR.K), perm)
    box, size = BOXES[0], (384, 384)
    rng = np.random.default_rng(0)
    kps = np.concatenate([rng.uniform(50, 300, (DR.K, 2)), rng.integers(0, 2, (DR.K, 1)) * 2.0], -1)
    plain = AR.keypoints(kps, box, np.array([0, 1.1, 0.3, 0, 0, 1, 0.0]), perm, size, (4.0, 4.0))
    flipped = AR.keypoints(kps, box, np.array([1, 1.1, 0.3, 0, 0, 1, 0.0]), perm, size, (4.0, 4.0))
    # a flip mirrors the crop of the same box, scale and angle and swaps the slots; doing it twice undoes it
    assert np.allclose(flipped["crop"][perm][:, 0], size[0] - plain["crop"][:, 0], atol=1e-9)
    assert np.allclose(flipped["crop"][perm][:, 1], plain["crop"][:, 1], atol=1e-9)
    assert np.array_equal(flipped["visible"][perm], plain["visible"])
    for pairs in ([(1, 2), (2, 3)], [(1, 1)], [(1, 2), (3, 1)], [(0, DR.K)]):
        with pytest.raises(ValueError):
            AR.permutation(pairs, DR.K)
        with pytest.raises(ValueError):
            Augment(flip_pairs=pairs).permutation(DR.K)


def _blob_cases():
    for flip in (0, 1):
        for s in (0.85, 1.2):
            for theta in (-0.6, 0.0, 0.45):
                for shift in ((0.0, 0.0), (0.08, -0.08)):
                    yield np.array([flip, s, theta, shift[0], shift[1], 1.0, 0.0])


def test_image_and_keypoints_move_together_and_planted_faults_do_not():
    """One Gaussian blob at keypoint 1 of a black frame: the intensity centroid of the restated crop lies within half
    an output pixel of the restated keypoint, in the slot the flip sends it to.  Each planted fault breaks that in
    every case it applies to."""
    size, box = (96, 128), BOXES[0]
    kps = np.zeros((DR.K, 3))
    kps[:, :2] = (215.0, 190.0)
    kps[1, :2] = (150.3, 130.7)
    yy, xx = np.mgrid[0:300, 0:400]
    blob = 255.0 * np.exp(-(((xx + 0.5 - kps[1, 0]) ** 2 + (yy + 0.5 - kps[1, 1]) ** 2) / (2 * 5.0 ** 2)))
    frame = np.repeat(np.round(blob).astype(np.uint8)[..., None], 3, -1)
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    failed = {f: [] for f in ("theta_sign", "swap_no_mirror", "mirror_no_swap")}
    n = 0
    for params in _blob_cases():
        x0, y0, x1, y1 = AR.region_rect(box, params)
        img = AR.warp(frame, AR.pixel_matrix(box, (x0, y0), params, size), 1.0, 0.0, size, tap_offset=(x0, y0))[0]
        assert img.sum() > 20 and img[0].max() == img[-1].max() == img[:, 0].max() == img[:, -1].max() == 0
        vv, uu = np.mgrid[0:size[1], 0:size[0]]
        centroid = np.array([(img * (uu + 0.5)).sum(), (img * (vv + 0.5)).sum()]) / img.sum()
        slot = 2 if params[0] else 1
        err = np.abs(AR.keypoints(kps, box, params, perm, size, (4.0, 4.0))["crop"][slot] - centroid).max()
        assert err < 0.5, (params, err)
        n += 1
        for fault, applies in (("theta_sign", params[2] != 0), ("swap_no_mirror", params[0] == 1),
                               ("mirror_no_swap", params[0] == 1)):
            if applies:
                bad = AR.keypoints(kps, box, params, perm, size, (4.0, 4.0), fault=fault)["crop"][slot]
                failed[fault].append(np.abs(bad - centroid).max() >= 0.5)
    assert n == 24
    for fault, outcomes in failed.items():
        assert len(outcomes) >= 12 and all(outcomes), fault


def test_the_workers_region_holds_every_tap_inside_the_frame(tree):
    """The crop sampled from the region the worker cut == the crop sampled from the whole frame (zero outside it), bit
    for bit, for drawn and for gridded parameters; the region is the restatement's rectangle."""
    from probpose_pytorch_amd.dataset import augment_region
    ds = _dataset(tree, shift=0.15, seed=2)
    size = (96, 96)
    checked = 0
    for epoch in (0, 1):
        ds.set_epoch(epoch)
        for i, ann in enumerate(ds.annotations):
            region, _, bbox, origin, params = ds[i]
            rect = AR.region_rect(bbox, params)
            assert rect == augment_region(bbox, params) and tuple(origin) == rect[:2]
            assert region.shape == (rect[3] - rect[1], rect[2] - rect[0], 3)
            m = AR.pixel_matrix(bbox, origin, params, size)
            a = AR.warp(region, m, params[5], params[6], size)
            b = AR.warp(_frame(ann), m, params[5], params[6], size, tap_offset=origin)
            assert np.array_equal(a, b), (epoch, i)
            checked += 1
    assert checked == 18
    ann = ds.annotations[3]                                   # the box that leaves the frame
    for params in AR.PARAM_GRID:
        x0, y0, x1, y1 = augment_region(ann["bbox"], params)
        region = np.asarray(PIL.Image.fromarray(_frame(ann)).crop((x0, y0, x1, y1)))
        m = AR.pixel_matrix(ann["bbox"], (x0, y0), params, DR.INPUT_SIZE)
        assert np.array_equal(AR.warp(region, m, 1.0, 0.0, DR.INPUT_SIZE),
                              AR.warp(_frame(ann), m, 1.0, 0.0, DR.INPUT_SIZE, tap_offset=(x0, y0)))


def test_host_matrices_equal_the_restatement(tree):
    from probpose_pytorch_amd.dataset import augment_matrices
    ds = _dataset(tree)
    boxes = np.array([a["bbox"] for a in ds.annotations])
    for params in AR.PARAM_GRID:
        p = np.tile(params, (len(boxes), 1))
        origins = np.array([AR.region_rect(b, params)[:2] for b in boxes])
        for size in ((384, 384), (192, 256)):
            pixel, keypoint = augment_matrices(boxes, origins, p, size)
            for i, box in enumerate(boxes):
                assert np.abs(pixel[i] - AR.pixel_matrix(box, origins[i], params, size)).max() < 1e-10
                assert np.abs(keypoint[i] - AR.keypoint_matrix(box, params, size)).max() < 1e-10


def test_gpu_test_inputs_keep_every_keypoint_off_the_crop_border(tree):
    """The GPU tests compare the flags exactly, so the restatement must put every keypoint of their inputs at least
    MARGIN from a border of the crop, and further than the keypoint's own counted float32 bound (which grows with
    in_w / box width: 0.016 pixel for the tree's box of one pixel's width)."""
    ds = _dataset(tree)
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    scale = ds.codec.probmap.scale_factor
    worst_margin, worst_bound = np.inf, 0.0
    for ann in ds.annotations:
        for params in AR.PARAM_GRID:
            kp = AR.keypoints(np.array(ann["keypoints"], dtype=np.float32), ann["bbox"], params, perm, DR.INPUT_SIZE, scale)
            margin = AR.border_margin(kp["crop"], DR.INPUT_SIZE)
            assert (margin > kp["bound"]).all(), (ann["bbox"], params)
            worst_margin = min(worst_margin, margin.min())
            worst_bound = max(worst_bound, kp["bound"].max())
    print("smallest distance from a border", worst_margin, "largest float32 bound", worst_bound)
    assert worst_margin >= AR.MARGIN


# ---- the library's host checks ---------------------------------------------------------------------------------------
def _check_args(n=3, K=DR.K):
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    shapes = [(40, 50), (33, 21), (64, 64)][:n]
    offs, total = YOLOPoseDataset.pack_layout(shapes)
    sources = np.array([[off, w, h, 3 * w] for off, (h, w) in zip(offs, shapes)], dtype=np.int64)
    warp = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]), (n, 1))
    aff = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=np.float32), (n, 1))
    return sources, total, warp, aff, AR.permutation(AR.FLIP_PAIRS, K).astype(np.int32)


def _check(lib, sources, total, warp, aff, perm):
    from probpose_pytorch_amd import _lib
    p = [np.ascontiguousarray(a) for a in (sources, warp, aff, perm)]
    assert p[0].dtype == np.int64 and p[1].dtype == np.float64 and p[2].dtype == np.float32 and p[3].dtype == np.int32
    _lib.check(lib.pp_augment_check(len(p[0]), p[0].ctypes.data_as(C.c_void_p), int(total),
                                    p[1].ctypes.data_as(C.c_void_p), p[2].ctypes.data_as(C.c_void_p), len(p[3]),
                                    p[3].ctypes.data_as(C.c_void_p)), "pp_augment_check")


def test_host_checks_refuse_bad_arguments(built_lib):
    from probpose_pytorch_amd._lib import HipExtensionError
    sources, total, warp, aff, perm = _check_args()
    _check(built_lib, sources, total, warp, aff, perm)                         # as packed: accepted
    end = int(sources[-1, 0] + 3 * sources[-1, 1] * sources[-1, 2])
    _check(built_lib, sources, end + 4, warp, aff, perm)                       # exactly the padding: accepted

    def refused(match, **kw):
        args = dict(sources=sources, total=total, warp=warp, aff=aff, perm=perm)
        args.update(kw)
        with pytest.raises(HipExtensionError, match=match):
            _check(built_lib, **args)

    for bad_value in (np.nan, np.inf, -np.inf, 1e13):
        for col in (0, 2, 6, 7):
            bad = warp.copy()
            bad[1, col] = bad_value
            refused("not finite", warp=bad)
        bad = aff.copy()
        bad[2, 4] = bad_value
        refused("not finite", aff=bad)
    for two_by_two in ((0, 0, 0, 0), (1, 2, 2, 4), (1, 0, 0, 0), (3, 3, 3, 3)):
        bad = warp.copy()
        bad[0, [0, 1, 3, 4]] = two_by_two
        refused("singular pixel matrix", warp=bad)
        bad = aff.copy()
        bad[0, [0, 1, 3, 4]] = two_by_two
        refused("singular keypoint matrix", aff=bad)
    bad = aff.copy()
    bad[1, 6] = 0.5
    refused("flip flag", aff=bad)
    cycle = perm.copy()
    cycle[[1, 2, 3]] = [2, 3, 1]                                               # a permutation, but a 3-cycle
    refused("not an involution", perm=cycle)
    twice = perm.copy()
    twice[5] = 1                                                               # two slots read keypoint 1
    refused("not an involution", perm=twice)
    for out in (-1, DR.K):
        bad = perm.copy()
        bad[0] = out
        refused("outside", perm=bad)
    bad = sources.copy()
    bad[1, 0] += 2
    refused("misaligned", sources=bad, total=total + 64)
    for short in (end + 3, end, end - 1):
        refused("past the end", total=short)
    bad = sources.copy()
    bad[0, 3] = 3 * bad[0, 1] - 1
    refused("row stride", sources=bad)
