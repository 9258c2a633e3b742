"""Half-body crops, blur and erasing of ``Augment`` on the CPU against tests/augment_post_reference.py:
the draws (pure functions of (seed, epoch, idx), ``draw`` untouched by the new settings), the records, the half-body
rule with its fall-backs and two planted faults, the refusals of ``__post_init__`` and of ``pp_augment_post_check``."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from tests import augment_post_reference as PR
from tests import augment_reference as AR
from tests import dataset_reference as DR

UPPER = tuple(range(0, 11))             # of the tree's K = 20: 0..10 "upper body", 11..19 "lower body"
ALL_ON = dict(half_body_prob=0.6, upper_body=UPPER, half_body_min_keypoints=6, blur_prob=0.4, median_prob=0.3,
              erase_prob=0.7, erase_holes=(1, 4), erase_size=(0.1, 0.5), erase_fill=0.5)
POST_ON = {k: v for k, v in ALL_ON.items() if not k.startswith(("half", "upper"))}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DR.write_tree(tmp_path_factory.mktemp("yolo"))


def _augment(**kw):
    from probpose_pytorch_amd.dataset import Augment
    return Augment(flip_pairs=AR.FLIP_PAIRS, **kw)


def _dataset(tree, **kw):
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    return YOLOPoseDataset(tree.parent, tree.name, Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS)),
                           target_single_class=0, augment=_augment(**kw))


def _uniforms(seed, epoch, idx, stream, count):
    return np.random.Generator(np.random.Philox(key=seed, counter=[epoch, idx, stream, 0])).random(count)


# ---- draws ---------------------------------------------------------------------------------------------------------------
def test_new_fields_follow_seed_and_default_to_off():
    from probpose_pytorch_amd.dataset import Augment
    names = [f.name for f in dataclasses.fields(Augment)]
    assert names[:9] == ["flip_pairs", "flip_prob", "scale", "rotate_deg", "rotate_prob", "shift", "brightness",
                         "contrast", "seed"]
    assert names[9:] == ["half_body_prob", "upper_body", "half_body_min_keypoints", "half_body_padding", "blur_prob",
                         "blur_kernel", "median_prob", "median_kernel", "erase_prob", "erase_holes", "erase_size",
                         "erase_fill"]
    a = Augment()
    assert (a.half_body_prob, a.upper_body, a.half_body_min_keypoints, a.half_body_padding) == (0.0, (), 9, 1.5)
    assert (a.blur_prob, a.blur_kernel, a.median_prob, a.median_kernel) == (0.0, (3, 7), 0.0, (3, 5))
    assert (a.erase_prob, a.erase_holes, a.erase_size, a.erase_fill) == (0.0, (1, 1), (0.2, 0.4), 0.0)
    assert Augment((), 0.5, (0.75, 1.25), 40.0, 0.6, 0.0, 0.2, 0.2, 5).seed == 5           # positional, as before


def test_draw_is_bit_identical_with_the_new_settings_on_and_off():
    off, on = _augment(shift=0.1, seed=3), _augment(shift=0.1, seed=3, **ALL_ON)
    for e in range(3):
        for i in range(40):
            want = _uniforms(3, e, i, 0, 8)
            assert on.draw(e, i).tobytes() == off.draw(e, i).tobytes()
            assert off.draw(e, i)[1] == 0.75 + want[1] * 0.5                # still the eight uniforms of counter [e, i, 0, 0]


def test_draw_post_and_half_body_box_are_pure_and_match_the_restatement():
    a = _augment(seed=9, **ALL_ON)
    rng = np.random.default_rng(0)
    kps = np.concatenate([rng.uniform(0, 300, (DR.K, 2)), rng.integers(0, 3, (DR.K, 1))], 1)
    bbox = [10.0, 20.0, 280.0, 260.0]
    first = {}
    kinds, halves = set(), set()
    for e in range(2):
        for i in range(60):
            rec, box = a.draw_post(e, i, (192, 256)), a.half_body_box(e, i, kps, bbox)
            assert rec.dtype == np.int32 and rec.shape == (24,) and box.dtype == np.float64 and box.shape == (4,)
            want = PR.post_record(_uniforms(9, e, i, 1, 20), (192, 256), **POST_ON)
            assert np.array_equal(rec, want), (e, i)
            wbox, chosen = PR.half_body(_uniforms(9, e, i, 2, 2), kps, bbox, UPPER, 0.6, 6)
            assert np.allclose(box, wbox, rtol=0, atol=1e-12), (e, i)
            kinds.add((int(rec[0]), int(rec[1]), int(rec[2])))
            halves.add(None if chosen is None else chosen[0] in UPPER)
            first[e, i] = (rec, box)
    assert {k[:2] for k in kinds} == {(0, 0), (1, 3), (1, 5), (1, 7), (2, 3), (2, 5)}
    assert {k[2] for k in kinds} == {0, 1, 2, 3, 4} and halves == {None, True, False}
    for (e, i) in reversed(list(first)):                            # another order of calls, another instance
        b = _augment(seed=9, **ALL_ON)
        assert np.array_equal(b.draw_post(e, i, (192, 256)), first[e, i][0])
        assert np.array_equal(b.half_body_box(e, i, kps, bbox), first[e, i][1])
    holed = [first[k][0].tobytes() for k in first if first[k][0][2] > 0]
    assert len(holed) > 60 and len(set(holed)) == len(holed)        # every (epoch, idx) has its own rectangles
    assert not np.array_equal(_augment(seed=10, **ALL_ON).draw_post(0, 0, (192, 256)), first[0, 0][0])


def test_changing_one_setting_leaves_the_other_fields_alone():
    base = _augment(seed=2, **ALL_ON)
    size = (192, 256)

    def records(a):
        return np.stack([a.draw_post(0, i, size) for i in range(200)])

    want = records(base)
    got = records(dataclasses.replace(base, blur_prob=0.1, median_prob=0.6))          # the filter: holes untouched
    assert np.array_equal(got[:, 2:], want[:, 2:]) and not np.array_equal(got[:, :2], want[:, :2])
    got = records(dataclasses.replace(base, blur_kernel=(5, 5)))
    assert np.array_equal(got[:, [0] + list(range(2, 24))], want[:, [0] + list(range(2, 24))])
    assert set(got[got[:, 0] == 1, 1]) == {5} and np.array_equal(got[got[:, 0] == 2], want[want[:, 0] == 2])
    got = records(dataclasses.replace(base, erase_prob=0.2))                          # fewer samples with holes
    assert np.array_equal(got[:, :2], want[:, :2])
    keep = got[:, 2] > 0
    assert 0 < keep.sum() < (want[:, 2] > 0).sum() and np.array_equal(got[keep], want[keep])
    got = records(dataclasses.replace(base, erase_fill=0.25))
    assert np.array_equal(np.delete(got, 3, 1), np.delete(want, 3, 1)) and (got[:, 3] != want[:, 3]).all()
    got = records(dataclasses.replace(base, erase_size=(0.3, 0.3)))                   # sizes: kind, k, count untouched
    assert np.array_equal(got[:, :4], want[:, :4])
    got = records(dataclasses.replace(base, half_body_prob=0.0, shift=0.3, flip_prob=0.1))
    assert np.array_equal(got, want)


def test_defaults_give_the_five_tuple_and_the_zero_record(tree):
    ds = _dataset(tree, shift=0.1, seed=7)
    assert len(ds[0]) == 5 and not ds.augment.post
    for i in range(50):
        assert not ds.augment.draw_post(1, i, DR.INPUT_SIZE).any()
        assert np.array_equal(ds.augment.half_body_box(1, i, np.ones((DR.K, 3)), [1.0, 2.0, 3.0, 4.0]), [1, 2, 3, 4])
    on = _dataset(tree, shift=0.1, seed=7, erase_prob=0.5)
    for i in range(len(ds)):
        a, b = ds[i], on[i]
        assert len(b) == 6 and np.array_equal(b[5], on.augment.draw_post(0, i, DR.INPUT_SIZE))
        for x, y in zip(a, b):                                     # blur and erasing change nothing a worker hands over
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_records_stay_inside_the_crop():
    a = _augment(seed=1, blur_prob=0.5, median_prob=0.5, erase_prob=1.0, erase_holes=(1, 4), erase_size=(0.01, 1.0))
    for size in ((12, 20), (192, 256)):
        widths = set()
        for i in range(1000):
            rec = a.draw_post(0, i, size)
            assert rec[0] in (1, 2) and rec[1] in ((3, 5, 7) if rec[0] == 1 else (3, 5)) and 1 <= rec[2] <= 4
            assert not rec[20:].any()
            for j in range(4):
                x0, y0, x1, y1 = rec[4 + 4 * j:8 + 4 * j]
                if j < rec[2]:
                    assert 0 <= x0 < x1 <= size[0] and 0 <= y0 < y1 <= size[1]
                    widths.add(int(x1 - x0))
                else:
                    assert (x0, y0, x1, y1) == (0, 0, 0, 0)
        assert min(widths) <= max(1, size[0] // 48) and max(widths) == size[0]      # both ends of erase_size are reached


def _identity(samples):
    return samples


def test_samples_do_not_depend_on_workers(tree):
    ds = _dataset(tree, shift=0.1, seed=11, **ALL_ON)
    ds.set_epoch(2)
    want = {i: ds[i] for i in range(len(ds))}
    moved = 0
    for i, s in want.items():
        ann = ds.annotations[i]
        kps = np.array(ann["keypoints"], dtype=np.float32)
        assert len(s) == 6 and np.array_equal(s[5], ds.augment.draw_post(2, i, DR.INPUT_SIZE))
        assert np.array_equal(s[2], ds.augment.half_body_box(2, i, kps, ann["bbox"]))
        assert np.array_equal(s[1], kps)                                        # every keypoint keeps its label
        assert np.array_equal(s[4], ds.augment.draw(2, i))
        moved += not np.array_equal(s[2], ann["bbox"])
    assert 0 < moved < len(ds)
    for workers in (0, 2):
        gen = torch.Generator().manual_seed(5)
        seen = []
        for batch in DataLoader(ds, batch_size=4, shuffle=True, num_workers=workers, collate_fn=_identity, generator=gen):
            for s in batch:
                i = [j for j in want if np.array_equal(want[j][2], s[2])][0]
                seen.append(i)
                for a, b in zip(s, want[i]):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (workers, i)
        assert sorted(seen) == list(range(len(ds)))


# ---- the half-body rule ----------------------------------------------------------------------------------------------------
def _person(labels=None):
    """K = 20 keypoints of a standing figure in the box [100, 50, 120, 300]: 0..10 in its upper 40 %, 11..19 in its lower
    45 %; unlabelled keypoints lie at (0, 0) as annotation files store them."""
    rng = np.random.default_rng(5)
    kps = np.zeros((DR.K, 3))
    kps[:11, 0], kps[:11, 1] = rng.uniform(110, 210, 11), rng.uniform(60, 170, 11)
    kps[11:, 0], kps[11:, 1] = rng.uniform(120, 200, 9), rng.uniform(215, 345, 9)
    kps[:, 2] = 2 if labels is None else labels
    kps[kps[:, 2] == 0, :2] = 0.0
    return kps, np.array([100.0, 50.0, 120.0, 300.0])


def _rule_holds(box, kps, chosen, bbox, padding):
    """The properties §4.4d states of a half-body box: it contains the chosen labelled keypoints, is centred on the
    midpoint of their extents, and each side is max(extent * padding, a quarter of the original side)."""
    pts = kps[chosen, :2]
    lo, hi = pts.min(0), pts.max(0)
    side = np.maximum((hi - lo) * padding, 0.25 * bbox[2:])
    return (PR.box_contains(box, pts) and np.allclose(box[:2] + box[2:] / 2, (lo + hi) / 2, rtol=0, atol=1e-9)
            and np.allclose(box[2:], side, rtol=0, atol=1e-9))


def _find(a, kps, bbox, want_upper):
    """An (epoch, idx) whose uniforms qualify the sample and pick the wanted half (where both are possible)."""
    for i in range(200):
        r = _uniforms(a.seed, 0, i, 2, 2)
        if r[0] < a.half_body_prob and (r[1] < 0.7) == want_upper:
            return i, r
    raise AssertionError("no such draw")


def test_half_body_box_contains_the_chosen_keypoints_and_faults_do_not_pass():
    a = _augment(seed=4, half_body_prob=0.5, upper_body=UPPER)
    labels = np.full(DR.K, 2.0)
    labels[[2, 7, 13, 18]] = 0                                    # unlabelled: stored at (0, 0), far outside the figure
    labels[[3, 15]] = 1
    kps, bbox = _person(labels)
    for want_upper in (True, False):
        i, r = _find(a, kps, bbox, want_upper)
        box = a.half_body_box(0, i, kps, bbox)
        wbox, chosen = PR.half_body(r, kps, bbox, UPPER, 0.5)
        assert (chosen[0] in UPPER) == want_upper and all(kps[c, 2] > 0 for c in chosen)
        assert len(chosen) == (9 if want_upper else 7)
        assert np.allclose(box, wbox, rtol=0, atol=1e-12) and _rule_holds(box, kps, chosen, bbox, 1.5)
        for fault in ("unlabelled", "pad_centre"):
            fbox, _ = PR.half_body(r, kps, bbox, UPPER, 0.5, fault=fault)
            assert not _rule_holds(fbox, kps, chosen, bbox, 1.5), fault
            assert not np.allclose(box, fbox, rtol=0, atol=1e-6), fault
    # not drawn: the original box, the same object's values
    i = [j for j in range(200) if _uniforms(4, 0, j, 2, 2)[0] >= 0.5][0]
    assert np.array_equal(a.half_body_box(0, i, kps, bbox), bbox)
    with pytest.raises(ValueError):
        _augment(half_body_prob=0.5, upper_body=(3, 25)).half_body_box(0, 0, kps, bbox)


def test_half_body_falls_back_when_a_half_has_too_few_keypoints():
    a = _augment(seed=4, half_body_prob=1.0, upper_body=UPPER)
    for i in range(30):                                          # whatever r1 says
        labels = np.full(DR.K, 2.0)
        labels[1:11] = 0                                         # one upper keypoint left: the lower body is taken
        kps, bbox = _person(labels)
        box = a.half_body_box(0, i, kps, bbox)
        assert _rule_holds(box, kps, list(range(11, 20)), bbox, 1.5)
        labels = np.full(DR.K, 2.0)
        labels[13:] = 0                                          # two lower keypoints left: the upper body is taken
        kps, bbox = _person(labels)
        assert _rule_holds(a.half_body_box(0, i, kps, bbox), kps, list(range(11)), bbox, 1.5)
        labels = np.zeros(DR.K)
        labels[[0, 11, 12]] = 2                                  # neither half suffices
        kps, bbox = _person(labels)
        few = _augment(seed=4, half_body_prob=1.0, upper_body=UPPER, half_body_min_keypoints=3)
        assert np.array_equal(few.half_body_box(0, i, kps, bbox), bbox)
        labels = np.full(DR.K, 2.0)
        labels[8:] = 0                                           # eight labelled keypoints: below the default of nine
        kps, bbox = _person(labels)
        assert np.array_equal(a.half_body_box(0, i, kps, bbox), bbox)


def test_half_body_keeps_a_quarter_of_the_original_side_on_a_collinear_set():
    a = _augment(seed=4, half_body_prob=1.0, upper_body=UPPER, half_body_padding=1.2)
    kps, bbox = _person()
    kps[:11, 0] = 150.0                                          # the upper body on one vertical line
    kps[11:, 1] = 300.0                                          # the lower body on one horizontal line
    i, _ = _find(a, kps, bbox, True)
    box = a.half_body_box(0, i, kps, bbox)
    assert box[2] == 0.25 * bbox[2] and box[0] == 150.0 - box[2] / 2
    assert box[3] == np.ptp(kps[:11, 1]) * 1.2 and _rule_holds(box, kps, list(range(11)), bbox, 1.2)
    i, _ = _find(a, kps, bbox, False)
    box = a.half_body_box(0, i, kps, bbox)
    assert box[3] == 0.25 * bbox[3] and box[1] == 300.0 - box[3] / 2 and _rule_holds(box, kps, list(range(11, 20)), bbox, 1.2)


def test_the_other_half_leaves_the_crop():
    """Through the restated keypoint path of §4.4c (identity parameters): with the upper body chosen every lower-body
    keypoint comes out with in_image = 0 and keeps its label, and the other way round."""
    a = _augment(seed=4, half_body_prob=1.0, upper_body=UPPER)
    kps, bbox = _person()
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    identity = np.array([0, 1.0, 0, 0, 0, 1, 0])
    whole = AR.keypoints(kps, bbox, identity, perm, DR.INPUT_SIZE, (4.0, 4.0))
    assert whole["in_image"].all()
    for want_upper, inside, outside in ((True, slice(0, 11), slice(11, 20)), (False, slice(11, 20), slice(0, 11))):
        i, _ = _find(a, kps, bbox, want_upper)
        got = AR.keypoints(kps, a.half_body_box(0, i, kps, bbox), identity, perm, DR.INPUT_SIZE, (4.0, 4.0))
        assert got["in_image"][inside].all() and not got["in_image"][outside].any()
        assert got["visible"].all() and (got["visibility"] == 1).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_post_init_refusals():
    bad = [dict(half_body_prob=1.5, upper_body=UPPER), dict(blur_prob=-0.1), dict(median_prob=2.0), dict(erase_prob=1.01),
           dict(blur_prob=float("nan")), dict(blur_prob=0.6, median_prob=0.5), dict(blur_kernel=(3, 4)),
           dict(blur_kernel=(2, 7)), dict(blur_kernel=(3, 9)), dict(blur_kernel=(5, 3)), dict(median_kernel=(3, 7)),
           dict(median_kernel=(4, 4)), dict(erase_holes=(0, 2)), dict(erase_holes=(2, 1)), dict(erase_holes=(1, 5)),
           dict(erase_size=(0.0, 0.5)), dict(erase_size=(0.5, 0.4)), dict(erase_size=(0.2, 1.1)),
           dict(erase_fill=float("inf")), dict(erase_fill=float("nan")), dict(half_body_prob=0.3),
           dict(half_body_prob=0.3, upper_body=(-1, 2))]
    for kw in bad:
        with pytest.raises(ValueError):
            _augment(**kw)
    ok = _augment(blur_prob=0.5, median_prob=0.5, blur_kernel=(7, 7), median_kernel=(5, 5), erase_holes=(4, 4),
                  erase_size=(1.0, 1.0), erase_fill=-2.5, half_body_prob=1.0, upper_body=[0, 1])
    assert ok.upper_body == (0, 1) and ok.post


def _check(lib, records, in_w=12, in_h=9, filters=1):
    records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 24)
    return lib.pp_augment_post_check(len(records), ctypes.c_void_p(records.ctypes.data), in_w, in_h, filters)


def test_host_check_refuses_bad_records(built_lib):
    good = PR.record(1, 7, [(0, 0, 12, 9), (11, 8, 12, 9), (3, 2, 5, 4), (0, 0, 1, 1)], 0.5)
    assert _check(built_lib, [good, PR.record(2, 5), PR.record()]) == 0
    assert _check(built_lib, [PR.record(0, 0, [(1, 1, 2, 2)], -3.0)], filters=0) == 0

    def refused(rec, word, **kw):
        assert _check(built_lib, [PR.record(), rec], **kw) != 0, word
        assert word.encode() in built_lib.pp_last_error(), (word, built_lib.pp_last_error())

    def edit(index, value, base=good):
        rec = base.copy()
        rec[index] = value
        return rec

    refused(edit(0, 3), "kind")
    refused(edit(0, -1), "kind")
    refused(edit(1, 4), "kernel size")
    refused(edit(1, 9), "kernel size")
    refused(PR.record(2, 7), "kernel size")                          # a 7 x 7 median
    refused(PR.record(0, 3), "kernel size")                          # a size without a filter
    refused(PR.record(1, 7), "larger", in_w=12, in_h=5)
    refused(PR.record(2, 5), "larger", in_w=4, in_h=9)
    refused(edit(2, 5), "holes")
    refused(edit(2, -1), "holes")
    refused(edit(6, 0), "empty")                                     # x1 == x0
    refused(edit(15, 2), "empty")                                    # y1 == y0 of hole 2
    refused(edit(6, 13), "leaves")
    refused(edit(5, -1), "leaves")
    refused(edit(11, 10), "leaves")
    refused(edit(3, np.float32(np.inf).view(np.int32)), "finite")
    refused(edit(3, np.float32(np.nan).view(np.int32)), "finite")
    for j in range(20, 24):
        refused(edit(j, 1), "reserved")
    refused(PR.record(1, 3), "filters = 0", filters=0)
    refused(PR.record(2, 3), "filters = 0", filters=0)
    assert _check(built_lib, [edit(17, 99, PR.record(0, 0, [(0, 0, 1, 1)]))]) == 0      # a rectangle past n_holes is not read
    assert built_lib.pp_augment_post_check(0, ctypes.c_void_p(good.ctypes.data), 12, 9, 1) != 0
    assert built_lib.pp_augment_post_check(1, None, 12, 9, 1) != 0
    assert built_lib.pp_augment_post_check(1, ctypes.c_void_p(good.ctypes.data), 12, 9, 2) != 0


# ---- the restatement against numpy -------------------------------------------------------------------------------------------
def test_reflect_101_is_numpys_reflect():
    rng = np.random.default_rng(1)
    for h, w, k in ((9, 12, 3), (9, 12, 5), (9, 13, 7), (7, 7, 7), (3, 5, 3), (20, 70, 7)):
        plane = rng.random((h, w))
        r = k // 2
        padded = np.pad(plane, r, mode="reflect")
        want = np.stack([padded[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)], -1)
        assert np.array_equal(PR.windows(plane, k), want)
        assert np.allclose(PR.box_mean(plane, k), want.mean(-1), rtol=0, atol=1e-15)
        assert np.array_equal(PR.median(plane, k), np.median(want, axis=-1))
        assert np.array_equal(PR.reflect101(np.arange(-r, w + r), w), np.pad(np.arange(w), r, mode="reflect"))
    img = rng.random((3, 9, 12)).astype(np.float32)
    got, is_box = PR.apply(img, PR.record(2, 3, [(1, 2, 4, 5)], 0.25), 1)
    assert not is_box and got.dtype == np.float32 and (got[:, 2:5, 1:4] == 0.25).all()
    assert got[0, 0, 0] == np.median([img[0, abs(y), abs(x)] for y in (-1, 0, 1) for x in (-1, 0, 1)])
    got, is_box = PR.apply(img, PR.record(1, 3), 0)                  # filters = 0: the kind is not read
    assert not is_box and np.array_equal(got, img)
