"""probpose.dataset without a GPU: the annotation parser, the CPU-only ``__getitem__``, the host-built multi-source
plan (tables == the single-frame builder's, applied in numpy == Pillow, argument checks) and the ground-truth
arithmetic restated in numpy float32 against ``frontend.scale_box`` / ``codec.encode``.

The parity batch is every class-0 instance of the tree of tests/dataset_reference.py: B = 9 from frames of three sizes,
with a box leaving the frame, .5 corners, an up-scaled, a down-scaled and a 1-pixel-wide box."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

from oracle import frontend_oracle as fo
from tests import dataset_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DR.write_tree(tmp_path_factory.mktemp("yolo"))


def _codec():
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    return Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS))


@pytest.fixture(scope="module")
def dataset(tree):
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    return YOLOPoseDataset(tree.parent, tree.name, _codec(), target_single_class=0)


def test_alias_module():
    import probpose.dataset
    import probpose_pytorch_amd.dataset
    from probpose.dataset import YOLOPoseDataset, parse_annotations  # noqa: F401
    assert probpose.dataset is probpose_pytorch_amd.dataset


def test_parse_annotations_equals_restatement(tree):
    from probpose_pytorch_amd.dataset import parse_annotations
    got, want = parse_annotations(tree), DR.parse_annotations(tree)
    assert len(got) == len(DR.INSTANCES) == len(want)
    assert got == want                      # same order, keys, bboxes and keypoints, value for value
    assert not any("unlabelled" in a["image_path"] for a in got)
    assert all(set(a) == {"image_path", "category_id", "bbox", "keypoints"} and a["category_id"] == 0 for a in got)
    flags = {kp[2] for a in got for kp in a["keypoints"]}
    assert flags == {0, 2}                  # the tree labels 0, 1 and 2; 1 is stored as 2
    for cls in (0, 1):
        only = parse_annotations(tree, target_single_class=cls)
        assert only == DR.parse_annotations(tree, target_single_class=cls)
        assert len(only) == sum(1 for i in DR.INSTANCES if i[1] == cls)


def test_parity_batch_covers_the_cases(dataset):
    assert len(dataset) == 9
    sizes = {PIL.Image.open(a["image_path"]).size for a in dataset.annotations}
    assert len(sizes) >= 3
    boxes = [a["bbox"] for a in dataset.annotations]
    assert any(b[0] < 0 for b in boxes) and any(b[0] % 1 == 0.5 for b in boxes)
    widths = [fo.round_box(b)[2] - fo.round_box(b)[0] for b in boxes]
    assert 1 in widths and max(widths) > DR.INPUT_SIZE[0] and any(1 < w < DR.INPUT_SIZE[0] for w in widths)


_CHILD = """
import pickle, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
from probpose_pytorch_amd.dataset import YOLOPoseDataset
from tests import dataset_reference as DR
assert not torch.cuda.is_available()
ds = YOLOPoseDataset({data!r}, {split!r}, Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS)), 0)
items = [ds[i] for i in range(len(ds))]
assert not torch.cuda.is_initialized()
pickle.dump((ds.annotations, items), open({out!r}, "wb"))
"""


def test_getitem_is_pillows_crop_and_needs_no_gpu(tree, tmp_path):
    out = str(tmp_path / "items.pkl")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    script = _CHILD.format(root=ROOT, data=str(tree.parent), split=tree.name, out=out)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    anns, items = pickle.load(open(out, "rb"))
    assert len(items) == 9
    for ann, (region, kps, bbox) in zip(anns, items):
        x, y, w, h = ann["bbox"]
        want = np.asarray(PIL.Image.open(ann["image_path"]).convert("RGB").crop((x, y, x + w, y + h)))
        assert region.dtype == np.uint8 and region.flags.c_contiguous and np.array_equal(region, want)
        assert kps.dtype == np.float32 and kps.shape == (DR.K, 3)
        assert np.array_equal(kps, np.array(ann["keypoints"], dtype=np.float32))
        assert bbox.dtype == np.float64 and list(bbox) == ann["bbox"]


# ---- the multi-source host plan ------------------------------------------------------------------------------------
def _pack(dataset):
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    regions = [dataset[i][0] for i in range(len(dataset))]
    shapes = [r.shape[:2] for r in regions]
    offs, total = YOLOPoseDataset.pack_layout(shapes)
    packed = np.full(total, 0xA5, dtype=np.uint8)          # the gaps and the padding are never part of a result
    for r, off in zip(regions, offs):
        packed[off:off + r.size] = r.reshape(-1)
    boxes = np.array([[0, 0, w, h] for h, w in shapes], dtype=np.int32)
    sources = np.array([[off, w, h, 3 * w] for off, (h, w) in zip(offs, shapes)], dtype=np.int64)
    return packed, boxes, sources


def _multi_plan(boxes, sources, src_bytes, size):
    from probpose_pytorch_amd import frontend
    plan = np.zeros(frontend.multi_plan_bytes(boxes, size) // 4, dtype=np.int32)
    n_blocks, lds = frontend.multi_plan_build(boxes, sources, src_bytes, size, plan.ctypes.data)
    return plan, n_blocks, lds


def _single_plan(lib, boxes, size):
    bp = boxes.ctypes.data_as(C.c_void_p)
    plan = np.zeros(lib.pp_frontend_plan_bytes(len(boxes), bp, size[0], size[1]) // 4, dtype=np.int32)
    nb, lds = C.c_int(0), C.c_longlong(0)
    assert lib.pp_frontend_plan_build(len(boxes), bp, size[0], size[1], plan.ctypes.data_as(C.c_void_p),
                                      C.byref(nb), C.byref(lds)) == 0
    return plan, nb.value, lds.value


def _apply(plan, c, n, packed, size):
    """Box c of a multi-source plan applied in numpy: (h, w, 3) uint8."""
    out_w, out_h = size
    h = plan[c * 16:(c + 1) * 16]
    off, sw, sh, stride = (int(v) for v in plan[n * 16 + 8 * c:n * 16 + 8 * c + 8].view(np.int64))
    src = packed[off:off + (sh - 1) * stride + 3 * sw]
    src = np.stack([src[r * stride:r * stride + 3 * sw].reshape(sw, 3) for r in range(sh)])
    x0, y0, cw, ch, ksh, ksv = (int(v) for v in h[:6])
    cur = fo.crop_zero_pad(src, (x0, y0, x0 + cw, y0 + ch)).astype(np.int64)
    half = 1 << (fo.PRECISION_BITS - 1)
    if h[12]:
        bh = plan[h[8]:h[8] + 2 * out_w].reshape(out_w, 2)
        kh = plan[h[9]:h[9] + ksh * out_w].reshape(out_w, ksh).astype(np.int64)
        tmp = np.zeros((ch, out_w, 3), np.int64)
        for xx in range(out_w):
            xmin, xmax = int(bh[xx, 0]), int(bh[xx, 1])
            ss = half + (cur[:, xmin:xmin + xmax] * kh[xx, :xmax][None, :, None]).sum(1)
            tmp[:, xx] = np.clip(ss >> fo.PRECISION_BITS, 0, 255)
        cur = tmp
    if h[13]:
        bv = plan[h[10]:h[10] + 2 * out_h].reshape(out_h, 2)
        kv = plan[h[11]:h[11] + ksv * out_h].reshape(out_h, ksv).astype(np.int64)
        res = np.zeros((out_h, out_w, 3), np.int64)
        for yy in range(out_h):
            ymin, ymax = int(bv[yy, 0]), int(bv[yy, 1])
            ss = half + (cur[ymin:ymin + ymax] * kv[yy, :ymax][:, None, None]).sum(0)
            res[yy] = np.clip(ss >> fo.PRECISION_BITS, 0, 255)
        cur = res
    return cur.astype(np.uint8)


def test_multi_plan_tables_equal_the_single_frame_builder(built_lib, dataset):
    packed, boxes, sources = _pack(dataset)
    n, size = len(boxes), DR.INPUT_SIZE
    assert all(off % 16 == 0 for off in sources[:, 0]) and packed.size >= sources[-1, 0] + 3 * sources[-1, 1] * sources[-1, 2] + 4
    multi, nb_m, lds_m = _multi_plan(boxes, sources, packed.size, size)
    single, nb_s, lds_s = _single_plan(built_lib, boxes, size)
    assert (nb_m, lds_m) == (nb_s, lds_s) and multi.size == single.size + 8 * n
    assert np.array_equal(multi[n * 16:n * 24].view(np.int64).reshape(n, 4), sources)
    # the block table: the same (box, first row) pairs, every pair once
    assert np.array_equal(multi[n * 24:n * 24 + 2 * nb_m], single[n * 16:n * 16 + 2 * nb_s])
    for c in range(n):
        hm, hs = multi[c * 16:(c + 1) * 16], single[c * 16:(c + 1) * 16]
        for slot in (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15):
            assert hm[slot] == hs[slot], (c, slot)
        for off_slot, count in ((8, 2 * size[0]), (9, hm[4] * size[0]), (10, 2 * size[1]), (11, hm[5] * size[1])):
            assert hm[off_slot] == hs[off_slot] + 8 * n
            assert np.array_equal(multi[hm[off_slot]:hm[off_slot] + count], single[hs[off_slot]:hs[off_slot] + count])


def test_multi_plan_applied_in_numpy_equals_pillow(built_lib, dataset):
    packed, boxes, sources = _pack(dataset)
    plan, _, _ = _multi_plan(boxes, sources, packed.size, DR.INPUT_SIZE)
    for c, ann in enumerate(dataset.annotations):
        frame = np.asarray(PIL.Image.open(ann["image_path"]).convert("RGB"))
        want = fo.scale_box_pil(frame, ann["bbox"], DR.INPUT_SIZE)
        got = _apply(plan, c, len(boxes), packed, DR.INPUT_SIZE)
        got = (got.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(2, 0, 1)
        assert np.array_equal(got, want), ann["bbox"]


def test_multi_plan_rejects_misaligned_and_overlong_sources(built_lib, dataset):
    from probpose_pytorch_amd._lib import HipExtensionError
    packed, boxes, sources = _pack(dataset)
    _multi_plan(boxes, sources, packed.size, DR.INPUT_SIZE)                       # the layout as packed is accepted
    bad = sources.copy()
    bad[2, 0] += 2
    with pytest.raises(HipExtensionError, match="misaligned"):
        _multi_plan(boxes, bad, packed.size + 64, DR.INPUT_SIZE)
    end = int(sources[-1, 0] + 3 * sources[-1, 1] * sources[-1, 2])
    _multi_plan(boxes, sources, end + 4, DR.INPUT_SIZE)                           # exactly the padding: accepted
    for short in (end + 3, end, end - 1):                                         # the last region ends too late
        with pytest.raises(HipExtensionError, match="past the end"):
            _multi_plan(boxes, sources, short, DR.INPUT_SIZE)
    bad = sources.copy()
    bad[0, 3] = 3 * bad[0, 1] - 1                                                 # a stride shorter than a row
    with pytest.raises(HipExtensionError, match="row stride"):
        _multi_plan(boxes, bad, packed.size, DR.INPUT_SIZE)
    with pytest.raises(ValueError):
        _multi_plan(boxes, sources[:-1], packed.size, DR.INPUT_SIZE)


# ---- ground-truth arithmetic ---------------------------------------------------------------------------------------
def test_ground_truth_arithmetic_equals_scale_box_and_encode(dataset, monkeypatch):
    """The float32 restatement the device kernel is tested against == the project's host expressions:
    frontend.scale_box's keypoint lines and codec.encode's in_image / heatmap_keypoints (their launches stubbed out:
    only the host arithmetic runs)."""
    from probpose_pytorch_amd import frontend
    from probpose_pytorch_amd.codec import ProbMap
    monkeypatch.setattr(frontend, "crop_resize", lambda image, boxes, size: [None])
    W, H = DR.HEATMAP_SIZE
    monkeypatch.setattr(ProbMap, "encode_device",
                        lambda self, kp, vis: (torch.zeros(1, DR.K, H, W), torch.zeros(1, DR.K)))
    codec = dataset.codec
    kps_raw = np.stack([np.array(a["keypoints"], dtype=np.float32) for a in dataset.annotations])
    boxes = np.array([a["bbox"] for a in dataset.annotations], dtype=np.float64)
    crop, hm, in_image, visible, visibility = DR.ground_truth_f32(kps_raw, boxes, DR.INPUT_SIZE,
                                                                  codec.probmap.scale_factor)
    on_zero = on_edge = 0
    for b, ann in enumerate(dataset.annotations):
        _, kps = frontend.scale_box(None, ann["bbox"], DR.INPUT_SIZE, np.array(ann["keypoints"], dtype=np.float32))
        assert kps.dtype == np.float32 and np.array_equal(kps[:, :2], crop[b])
        enc = codec.encode(kps[None, :, :2], kps[None, :, 2] == 2)
        assert np.array_equal(enc["in_image"][0], in_image[b])
        assert enc["heatmap_keypoints"].dtype == np.float32 and np.array_equal(enc["heatmap_keypoints"][0], hm[b])
        assert np.array_equal(kps[:, 2] == 2, visible[b]) and np.array_equal(np.minimum(kps[:, 2], 1), visibility[b])
        on_zero += int(((crop[b] == 0).any(-1) & in_image[b]).sum())
        on_edge += int(((crop[b, :, 0] == DR.INPUT_SIZE[0]) | (crop[b, :, 1] == DR.INPUT_SIZE[1])).sum())
        assert not in_image[b][(crop[b, :, 0] == DR.INPUT_SIZE[0]) | (crop[b, :, 1] == DR.INPUT_SIZE[1])].any()
    assert on_zero >= 1 and on_edge >= 2        # keypoints exactly on 0 (inside) and exactly on in_w / in_h (outside)
    unlabelled = [b for b, a in enumerate(dataset.annotations) if round(a["bbox"][2]) == 37]
    assert in_image.any() and not in_image.all() and visible.any() and not visible[unlabelled[0]].any()


def test_loader_refuses_more_than_15_workers(dataset):
    with pytest.raises(ValueError, match="num_workers"):
        dataset.loader(4, num_workers=16)
    assert dataset.loader(4, num_workers=0).collate_fn == dataset.collate
