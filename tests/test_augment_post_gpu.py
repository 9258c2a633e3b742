"""``pp_augment_post`` on the GPU against the float64 restatement of tests/augment_post_reference.py:
the median and the copy bit for bit, the box mean within k^2 u, the holes exactly, the floats around the output
untouched; then whole batches of ``YOLOPoseDataset`` with half-body crops, blur and erasing switched on."""
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_post_reference as PR
from tests import augment_reference as AR
from tests import dataset_reference as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096            # floats on either side of the output that must keep their bits
SENTINEL = np.float32(-123.456)
FILTERS = [(1, 3), (1, 5), (1, 7), (2, 3), (2, 5)]
LOADER_AUGMENT = dict(shift=0.1, seed=7)
UPPER = tuple(range(0, 11))
ALL_ON = dict(half_body_prob=0.6, upper_body=UPPER, half_body_min_keypoints=6, blur_prob=0.4, median_prob=0.3,
              erase_prob=0.7, erase_holes=(1, 4), erase_size=(0.1, 0.5), erase_fill=0.5)
WORST = {}              # class -> worst |d| / bound of a box mean, printed by the last test of the kernel section


def _tile():
    """(TILE_W, TILE_H) of augment_post_kernel, as the header states them and the kernel's source takes them."""
    header = open(os.path.join(ROOT, "include", "probpose_hip.h")).read()
    source = open(os.path.join(ROOT, "probpose_pytorch_amd", "csrc", "pp_augment_post.hip")).read()
    tile = tuple(int(re.search(rf"#define PP_AUGMENT_POST_TILE_{a}\s+(\d+)", header).group(1)) for a in "WH")
    assert "POST_TW = PP_AUGMENT_POST_TILE_W, POST_TH = PP_AUGMENT_POST_TILE_H" in source
    return tile


def _big_crops():
    """Crops larger than the tile in both directions, neither side a multiple of it: one per store form."""
    tw, th = _tile()
    sizes = [(2 * tw + 20, 2 * th + 5), (2 * tw + 22, 2 * th + 5)]
    assert all(w > tw and h > th and w % tw and h % th for w, h in sizes)
    assert sizes[0][0] % 4 == 0 and sizes[1][0] % 4 != 0
    return sizes


def _post(lib, img, records, filters, in_place=False, shift=0):
    """pp_augment_post on img (n, 3, h, w) f32.  The output lies between two guards of GUARD sentinel floats (``shift``
    more in front: an output that is not 16-byte aligned); in place, the input itself lies there.  Asserts that the
    guards kept their bits and returns the output."""
    from probpose_pytorch_amd import _lib
    img = np.ascontiguousarray(img, dtype=np.float32)
    records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, PR.WORDS)
    n, _, h, w = img.shape
    assert len(records) == n
    _lib.check(lib.pp_augment_post_check(n, records.ctypes.data, w, h, filters), "pp_augment_post_check")
    count = img.size
    lead = GUARD + shift
    host = np.full(count + 2 * GUARD + shift, SENTINEL, dtype=np.float32)
    if in_place:
        host[lead:lead + count] = img.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    out = buf[lead:lead + count]
    d_in = out if in_place else torch.from_numpy(img).cuda()
    d_rec = torch.from_numpy(records).cuda()
    _lib.check(lib.pp_augment_post(_lib.ptr(d_in), _lib.ptr(d_rec), n, w, h, filters, _lib.ptr(out), _lib.stream_ptr()),
               "pp_augment_post")
    got = buf.cpu().numpy()
    assert (got[:lead].view(np.uint32) == SENTINEL.view(np.uint32)).all()
    assert (got[lead + count:].view(np.uint32) == SENTINEL.view(np.uint32)).all()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), img)                       # the input is only read
    return got[lead:lead + count].reshape(img.shape)


def _compare(got, img, records, filters, what):
    """Every sample against the restatement: a box mean within k^2 u (its holes exactly), everything else bit for bit."""
    for i, rec in enumerate(np.asarray(records).reshape(-1, PR.WORDS)):
        want, is_box = PR.apply(img[i], rec, filters)
        if is_box:
            k = int(rec[1])
            ratio = float(np.abs(got[i].astype(np.float64) - want).max() / PR.box_bound(k))
            print(f"{what}: sample {i} box k = {k}: worst d/bound {ratio:.3f}")
            WORST[f"box k = {k}"] = max(WORST.get(f"box k = {k}", 0.0), ratio)
            assert ratio <= 1.0, (what, i, ratio)
            for j in range(int(rec[2])):
                x0, y0, x1, y1 = rec[4 + 4 * j:8 + 4 * j]
                assert (got[i][:, y0:y1, x0:x1].view(np.uint32) == rec[3].view(np.uint32)).all(), (what, i, j)
        else:
            assert want.dtype == np.float32
            assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (what, i, rec[:3])


def _random(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


# ---- filters ---------------------------------------------------------------------------------------------------------------
def test_every_filter_on_small_and_large_crops(built_lib):
    """12 x 9 (128-bit stores) and 13 x 9 (scalar stores), both smaller than one tile; crops of several tiles with a
    remainder in both directions, one per store form; n = 1 for every filter and the copy."""
    for w, h in [(12, 9), (13, 9)] + _big_crops():
        img = _random((1, 3, h, w), w * h)
        assert 0.0 <= img.min() and img.max() < 1.0
        for kind, k in [(0, 0)] + FILTERS:
            rec = PR.record(kind, k)
            _compare(_post(built_lib, img, rec, 1), img, rec, 1, f"{w} x {h}")
    # 128-bit shapes through the scalar form: an output that is 4-byte, not 16-byte, aligned
    img = _random((1, 3, 9, 12), 3)
    for kind, k in [(0, 0), (1, 5), (2, 3)]:
        rec = PR.record(kind, k, [(2, 1, 7, 6)], 0.75)
        _compare(_post(built_lib, img, rec, 1, shift=1), img, rec, 1, "unaligned output")
    rec = PR.record(0, 0, [(2, 1, 7, 6), (8, 0, 12, 9)], 0.75)
    _compare(_post(built_lib, img, rec, 0, in_place=True, shift=3), img, rec, 0, "unaligned output in place")


def test_kernel_size_equal_to_the_smaller_side(built_lib):
    """The reflected halo spans the whole side: row -r reads row r = the last row."""
    for (w, h), filters in (((12, 3), [(1, 3), (2, 3)]), ((3, 9), [(1, 3), (2, 3)]), ((8, 5), [(1, 5), (2, 5)]),
                            ((5, 13), [(1, 5), (2, 5)]), ((12, 7), [(1, 7)]), ((7, 7), [(1, 7)]), ((7, 70), [(1, 7)])):
        img = _random((1, 3, h, w), 7 * w + h)
        for kind, k in filters:
            assert k == min(w, h)
            rec = PR.record(kind, k)
            _compare(_post(built_lib, img, rec, 1), img, rec, 1, f"k = side, {w} x {h}")


def test_ties_reach_the_median(built_lib):
    """0 / 1 checkerboards (cells of 1, 2 and 3 pixels): every window holds many equal values."""
    for w, h in [(12, 9), (13, 9), _big_crops()[0]]:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([((yy // c + xx // c) % 2).astype(np.float32) for c in (1, 2, 3)])[None]
        for kind, k in FILTERS:
            rec = PR.record(kind, k)
            got = _post(built_lib, img, rec, 1)
            _compare(got, img, rec, 1, f"checkerboard {w} x {h}")
            if kind == 2:
                assert set(np.unique(got)) == {0.0, 1.0}


def test_mixed_batch_of_five(built_lib):
    for w, h in [(12, 9), (13, 9)] + _big_crops():
        img = _random((5, 3, h, w), 11 + w)
        records = np.stack([PR.record(2, 5, [(0, 0, 3, 2)], 0.5), PR.record(0, 0), PR.record(1, 7, [(w - 4, h - 5, w, h)]),
                            PR.record(2, 3), PR.record(1, 3, [(1, 1, 2, 2), (w // 2, 0, w // 2 + 3, h)], 1.0)])
        _compare(_post(built_lib, img, records, 1), img, records, 1, f"mixed batch {w} x {h}")


def test_print_the_worst_box_ratios():
    print("box mean, worst |d| / (k^2 u) per size:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert WORST and max(WORST.values()) <= 1.0


# ---- holes -----------------------------------------------------------------------------------------------------------------
def _hole_cases(w, h):
    return {
        "none": ([], 0.0),
        "a pixel in each corner": ([(0, 0, 1, 1), (w - 1, 0, w, 1), (0, h - 1, 1, h), (w - 1, h - 1, w, h)], 0.0),
        "one on each border": ([(2, 0, 5, 2), (0, 3, 2, 6), (w - 3, 2, w, 5), (4, h - 2, 9, h)], 0.0),
        "the whole crop": ([(0, 0, w, h)], 0.0),
        "two that overlap": ([(1, 1, 7, 6), (4, 3, 11, 8)], 0.0),
        "four with a fill": ([(0, 1, 4, 4), (5, 0, 8, h), (3, 5, w, 7), (w - 2, h - 2, w, h)], 0.625),
        "odd corners": ([(1, 2, 2, 3), (3, 1, 6, 8)], -1.5),
    }


def test_holes_in_place_and_behind_a_filter(built_lib):
    for w, h in [(12, 9), (13, 9)] + _big_crops():
        img = _random((1, 3, h, w), 5 * w + h)
        for what, (holes, fill) in _hole_cases(w, h).items():
            rec = PR.record(0, 0, holes, fill)
            got = _post(built_lib, img, rec, 0, in_place=True)
            _compare(got, img, rec, 0, f"{what}, in place, {w} x {h}")
            mask = np.zeros((h, w), dtype=bool)
            for x0, y0, x1, y1 in holes:
                mask[y0:y1, x0:x1] = True
            assert np.array_equal(got[0][:, ~mask].view(np.uint32), img[0][:, ~mask].view(np.uint32))
            assert (got[0][:, mask] == np.float32(fill)).all()
            for kind, k in ((0, 0), (1, 3), (2, 5)):
                rec = PR.record(kind, k, holes, fill)
                _compare(_post(built_lib, img, rec, 1), img, rec, 1, f"{what}, kind {kind}, {w} x {h}")
    # a hole of a large crop that touches one tile only, and one that crosses the tile borders
    tw, th = _tile()
    for w, h in _big_crops():
        img = _random((1, 3, h, w), 77)
        for holes in ([(tw + 1, th + 1, tw + 5, th + 3)], [(tw - 3, th - 2, 2 * tw + 4, 2 * th + 1), (0, 0, w, 1)]):
            rec = PR.record(0, 0, holes, 0.25)
            _compare(_post(built_lib, img, rec, 0, in_place=True), img, rec, 0, "tile borders, in place")
            _compare(_post(built_lib, img, PR.record(1, 5, holes, 0.25), 1), img, PR.record(1, 5, holes, 0.25), 1,
                     "tile borders, box")


def test_hole_free_samples_of_a_mixed_batch_keep_their_bits(built_lib):
    for w, h in [(12, 9), _big_crops()[1]]:
        img = _random((5, 3, h, w), 9)
        records = np.stack([PR.record(), PR.record(0, 0, [(1, 1, 5, 4)], 0.5), PR.record(),
                            PR.record(0, 0, [(0, 0, w, h)], 0.125), PR.record()])
        got = _post(built_lib, img, records, 0, in_place=True)
        _compare(got, img, records, 0, "erase-only batch")
        for i in (0, 2, 4):
            assert np.array_equal(got[i].view(np.uint32), img[i].view(np.uint32))
        assert (got[3] == np.float32(0.125)).all()


def test_the_entry_refuses_overlaps_and_bad_arguments(built_lib):
    """Return codes only: every one of these is refused on the host, before any launch."""
    from probpose_pytorch_amd import _lib
    n, w, h = 2, 12, 9
    buf = torch.zeros(4 * n * 3 * h * w, dtype=torch.float32, device="cuda")
    rec = torch.zeros(n * PR.WORDS, dtype=torch.int32, device="cuda")
    base, r, count = buf.data_ptr(), rec.data_ptr(), n * 3 * h * w
    s = _lib.stream_ptr()
    post = built_lib.pp_augment_post

    def refused(word, *args):
        assert post(*args, s) != 0, word
        assert word.encode() in built_lib.pp_last_error(), (word, built_lib.pp_last_error())

    refused("overlap", base, r, n, w, h, 1, base)                           # filters = 1 with in == out
    refused("overlap", base, r, n, w, h, 1, base + 4 * (count - 1))         # the last float of in is the first of out
    refused("overlap", base + 4 * (count - 1), r, n, w, h, 1, base)
    refused("overlap", base, r, n, w, h, 0, base + 16)                      # holes only: in == out or apart
    refused("null", None, r, n, w, h, 1, base)
    refused("null", base, None, n, w, h, 1, base + 4 * count)
    refused("null", base, r, n, w, h, 1, None)
    refused("misaligned", base + 2, r, n, w, h, 1, base + 4 * count)
    refused("misaligned", base, r + 1, n, w, h, 1, base + 4 * count)
    refused("misaligned", base, r, n, w, h, 1, base + 4 * count + 1)
    refused("bad shape", base, r, 0, w, h, 1, base + 4 * count)
    refused("bad shape", base, r, n, 0, h, 1, base + 4 * count)
    refused("bad shape", base, r, n, w, -1, 1, base + 4 * count)
    refused("bad shape", base, r, n, w, h, 2, base + 4 * count)
    torch.cuda.synchronize()
    assert not buf.any()


# ---- whole batches ---------------------------------------------------------------------------------------------------------
def _codec():
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    return Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DR.write_tree(tmp_path_factory.mktemp("yolo"))


def _dataset(tree, **kw):
    from probpose_pytorch_amd.dataset import Augment, YOLOPoseDataset
    return YOLOPoseDataset(tree.parent, tree.name, _codec(), target_single_class=0,
                           augment=Augment(flip_pairs=AR.FLIP_PAIRS, **LOADER_AUGMENT, **kw))


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_whole_batches_with_every_new_setting_on(tree, built_lib):
    ds = _dataset(tree, **ALL_ON)
    ds.set_epoch(1)
    samples = [ds[i] for i in range(len(ds))]
    assert all(len(s) == 6 for s in samples)
    records = np.stack([s[5] for s in samples])
    assert {0, 1, 2} <= set(records[:, 0]) and (records[:, 2] > 0).any() and (records[:, 2] == 0).any()
    assert any(not np.array_equal(s[2], a["bbox"]) for s, a in zip(samples, ds.annotations))       # half-body boxes
    img, gt = ds.collate(samples)
    torch.cuda.synchronize()
    # the existing augmented path on the same boxes: its image is the warp's output, its gt is the gt
    warped, want_gt = ds.collate([s[:5] for s in samples])
    assert all(torch.equal(gt[k], want_gt[k]) for k in want_gt) and gt.keys() == want_gt.keys()
    assert not gt["in_image"].all() and gt["in_image"].any()
    got, warped = img.cpu().numpy(), warped.cpu().numpy()
    _compare(got, warped, records, 1, "whole batch")
    assert not np.array_equal(got, warped)
    # no host synchronisation in the collate with the new launch
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ds.collate(samples)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same((img, gt), again)
    # the shuffled two-worker loader hands over the same rows, whatever the batch they come in
    seen = []
    for b_img, b_gt in ds.loader(batch_size=4, shuffle=True, num_workers=2):
        assert b_img.dtype == torch.float32 and tuple(b_img.shape[1:]) == (3, DR.INPUT_SIZE[1], DR.INPUT_SIZE[0])
        for b in range(b_img.shape[0]):
            i = [j for j in range(len(ds)) if torch.equal(b_img[b], img[j])]
            assert len(i) >= 1, b
            i = [j for j in i if all(torch.equal(b_gt[k][b], gt[k][j]) for k in gt)][0]
            seen.append(i)
    assert sorted(seen) == list(range(len(ds)))
    # erase only: holes in place, no second tensor, and the pixels outside the holes are the warp's
    erase = _dataset(tree, erase_prob=0.7, erase_holes=(1, 4), erase_size=(0.1, 0.5), erase_fill=0.5)
    erase.set_epoch(1)
    e_samples = [erase[i] for i in range(len(erase))]
    e_img, e_gt = erase.collate(e_samples)
    e_warped, e_want = erase.collate([s[:5] for s in e_samples])
    e_records = np.stack([s[5] for s in e_samples])
    assert not e_records[:, :2].any() and (e_records[:, 2] > 0).any()
    _compare(e_img.cpu().numpy(), e_warped.cpu().numpy(), e_records, 0, "erase-only batch")
    assert all(torch.equal(e_gt[k], e_want[k]) for k in e_want)
    with pytest.raises(ValueError):
        ds.collate(samples[:2] + [samples[2][:5]])                    # tuple lengths are not mixed


def test_defaults_give_todays_bits(tree, built_lib):
    from probpose_pytorch_amd.dataset import Augment, YOLOPoseDataset
    today = _dataset(tree)
    explicit = YOLOPoseDataset(tree.parent, tree.name, _codec(), target_single_class=0, augment=Augment(
        AR.FLIP_PAIRS, 0.5, (0.75, 1.25), 40.0, 0.6, 0.1, 0.2, 0.2, 7, half_body_prob=0.0, upper_body=UPPER,
        half_body_min_keypoints=9, half_body_padding=1.5, blur_prob=0.0, blur_kernel=(3, 7), median_prob=0.0,
        median_kernel=(3, 5), erase_prob=0.0, erase_holes=(1, 1), erase_size=(0.2, 0.4), erase_fill=0.0))
    a = [today[i] for i in range(len(today))]
    b = [explicit[i] for i in range(len(explicit))]
    assert all(len(s) == 5 for s in b)
    for s, t in zip(a, b):
        for x, y in zip(s, t):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    assert _same(today.collate(a), explicit.collate(b))
    # and the record of a sample that drew nothing changes no bit: kind 0, no holes, in place
    off = _dataset(tree, erase_prob=1e-12)
    c = [off[i] for i in range(len(off))]
    assert all(len(s) == 6 and not s[5].any() for s in c)
    assert _same(today.collate(a), off.collate(c))
