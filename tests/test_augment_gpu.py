"""Augmentation of probpose.dataset on the GPU against the float64 restatement of tests/augment_reference.py:
``pp_augment_warp`` element by element within a bound counted from its float32 roundings (bit for bit on integer-exact
inputs), ``pp_dataset_ground_truth_affine`` within its counted bound with the flags exact, the maps against the oracle
bit for bit, whole batches from a shuffled loader with workers over two epochs, the un-augmented bits, and one training
step on an augmented batch."""
import numpy as np
import PIL.Image
import pytest
import torch

from oracle import probpose_oracle as orc
from tests import augment_reference as AR
from tests import dataset_reference as DR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 4096            # floats on either side of the warp's output that must keep their bits
LOADER_AUGMENT = dict(shift=0.1, seed=7)


def _codec():
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    return Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return DR.write_tree(tmp_path_factory.mktemp("yolo"))


@pytest.fixture(scope="module")
def dataset(tree, built_lib):
    from probpose_pytorch_amd.dataset import Augment, YOLOPoseDataset
    return YOLOPoseDataset(tree.parent, tree.name, _codec(), target_single_class=0,
                           augment=Augment(flip_pairs=AR.FLIP_PAIRS, **LOADER_AUGMENT))


@pytest.fixture(scope="module")
def plain(tree, built_lib):
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    return YOLOPoseDataset(tree.parent, tree.name, _codec(), target_single_class=0)


def _frame(ann):
    with PIL.Image.open(ann["image_path"]) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def test_dataset_takes_an_augment(dataset):
    from probpose_pytorch_amd.dataset import Augment
    assert isinstance(dataset.augment, Augment) and len(dataset[0]) == 5


# ---- pixels ------------------------------------------------------------------------------------------------------------
def _warp(lib, regions, offsets, total, mats, colour, size):
    """pp_augment_warp on regions placed at the given byte offsets of a ``total``-byte buffer (0xA5 between and behind
    them).  Returns the (n, 3, h, w) result; asserts that the floats around the output kept their bits."""
    from probpose_pytorch_amd import _lib
    n, (in_w, in_h) = len(regions), size
    packed = np.full(total, 0xA5, dtype=np.uint8)
    sources = np.empty((n, 4), dtype=np.int64)
    for i, (r, off) in enumerate(zip(regions, offsets)):
        packed[off:off + r.size] = r.reshape(-1)
        sources[i] = (off, r.shape[1], r.shape[0], 3 * r.shape[1])
    warp = np.empty((n, 8), dtype=np.float64)
    warp[:, :6], warp[:, 6:] = np.asarray(mats, dtype=np.float64).reshape(n, 6), np.asarray(colour, dtype=np.float64)
    aff = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32), (n, 1))
    perm = np.arange(DR.K, dtype=np.int32)
    _lib.check(lib.pp_augment_check(n, sources.ctypes.data, total, warp.ctypes.data, aff.ctypes.data, DR.K,
                                    perm.ctypes.data), "pp_augment_check")
    d_src = torch.from_numpy(packed).cuda()
    assert d_src.numel() == total
    d_sources, d_warp = torch.from_numpy(sources).cuda(), torch.from_numpy(warp).cuda()
    count = n * 3 * in_h * in_w
    sentinel = np.float32(-123.456)
    buf = torch.full((count + 2 * GUARD,), float(sentinel), dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + count]
    _lib.check(lib.pp_augment_warp(_lib.ptr(d_src), _lib.ptr(d_sources), _lib.ptr(d_warp), n, in_w, in_h,
                                   _lib.ptr(out), _lib.stream_ptr()), "pp_augment_warp")
    got = buf.cpu().numpy()
    assert (got[:GUARD] == sentinel).all() and (got[GUARD + count:] == sentinel).all()
    assert not (got[GUARD:GUARD + count] == sentinel).any()
    return got[GUARD:GUARD + count].reshape(n, 3, in_h, in_w)


def _layout(regions):
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    return YOLOPoseDataset.pack_layout([r.shape[:2] for r in regions])


def _compare(got, regions, mats, colour, size, what):
    worst = 0.0
    for i, (r, m, (c, b)) in enumerate(zip(regions, mats, colour)):
        want = AR.warp(r, np.asarray(m, dtype=np.float64), float(np.float32(c)), float(np.float32(b)), size)
        # the restatement takes float32(c), float32(b) as the kernel does; warp_bound still counts their rounding
        ratio = np.abs(got[i].astype(np.float64) - want).max() / AR.warp_bound(c, b)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, i, ratio)
    print(f"{what}: worst d/bound {worst:.3f}")
    return worst


def _regions(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def test_warp_integer_exact_inputs_come_out_bit_for_bit(built_lib):
    """Identity matrix with integer offsets: every tap weight is 0 or 1, c = 1, b = 0: the result is pixel / 255 in
    float32, or 0 where the lattice leaves the region (offsets of both signs: all four edges)."""
    for size in ((384, 384), (192, 256)):
        regions = _regions([(300, 200), (400, 401), (17, 23)], 1)
        shifts = [(-5, 7), (9, -11), (-180, -120)]
        mats = [[[1, 0, tx], [0, 1, ty]] for tx, ty in shifts]
        offs, total = _layout(regions)
        got = _warp(built_lib, regions, offs, total, mats, [(1.0, 0.0)] * 3, size)
        for i, (r, (tx, ty)) in enumerate(zip(regions, shifts)):
            want = np.zeros((size[1], size[0], 3), dtype=np.float32)
            vv, uu = np.mgrid[0:size[1], 0:size[0]]
            x, y = uu + tx, vv + ty
            inside = (x >= 0) & (x < r.shape[1]) & (y >= 0) & (y < r.shape[0])
            want[inside] = r[y[inside], x[inside]].astype(np.float32) / np.float32(255)
            assert inside.any() and not inside.all()
            assert np.array_equal(got[i], want.transpose(2, 0, 1)), (size, i)


def _affine(rng, shape, size):
    """A rotation + scale that looks at the region's middle and reaches over its edges."""
    h, w = shape
    th, s = rng.uniform(-0.7, 0.7), rng.uniform(0.8, 1.3)
    a = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) * [s * w / size[0], s * h / size[1]]
    t = np.array([w / 2, h / 2]) - a @ np.array([size[0] / 2, size[1] / 2]) + rng.uniform(-3, 3, 2)
    return np.concatenate([a, t[:, None]], 1)


def test_warp_against_the_restatement(built_lib):
    rng = np.random.default_rng(3)
    worst = 0.0
    for size in ((384, 384), (192, 256)):
        # a batch of mixed region sizes, one region a single pixel, with rotations, scales and colour terms
        shapes = [(310, 205), (64, 500), (1, 1), (129, 131), (2, 3), (450, 333)]
        regions = _regions(shapes, 4)
        mats = [_affine(rng, s, size) for s in shapes]
        colour = [(1.0, 0.0), (1.2, 0.2), (0.8, -0.2), (1.13, -0.07), (0.9, 0.1), (1.2, -0.2)]
        offs, total = _layout(regions)
        worst = max(worst, _compare(_warp(built_lib, regions, offs, total, mats, colour, size), regions, mats, colour,
                                    size, f"mixed batch {size}"))
        # edges and corners: taps half in and half out (a half-pixel lattice that starts one pixel outside)
        regions = _regions([(200, 200), (130, 97)], 5)
        mats = [[[1, 0, -1.5], [0, 1, -1.5]], [[0.5, 0, -0.75], [0, 0.5, -0.75]]]
        if size == (192, 256):
            mats = [[[1.05, 0, -1.5], [0, 0.79, -1.5]], [[0.51, 0, -0.75], [0, 0.38, -0.75]]]
        offs, total = _layout(regions)
        got = _warp(built_lib, regions, offs, total, mats, [(1.0, 0.0)] * 2, size)
        assert got[0][:, 0, 0].max() == 0 and 0 < got[0][:, 1, 1].max() <= 0.25 + 1e-6   # a corner: one tap of four
        worst = max(worst, _compare(got, regions, mats, [(1.0, 0.0)] * 2, size, f"edges {size}"))
    # B = 1
    regions = _regions([(77, 91)], 6)
    mats = [_affine(rng, (77, 91), (384, 384))]
    offs, total = _layout(regions)
    worst = max(worst, _compare(_warp(built_lib, regions, offs, total, mats, [(1.1, 0.05)], (384, 384)), regions, mats,
                                [(1.1, 0.05)], (384, 384), "B = 1"))
    print(f"pixels: worst d/bound over the classes {worst:.3f}")


def test_warp_byte_offset_classes_and_the_last_region(built_lib):
    """Regions at each offset class the C ABI allows (multiples of 4: 0, 4, 8, 12 mod 16) with odd widths, so that rows
    start at every byte alignment; the last region ends exactly PP_FRONTEND_SRC_PAD bytes before the end of the device
    buffer and its last pixels are read (the lattice covers the whole region)."""
    size = (192, 256)
    shapes = [(37, 41), (53, 29), (31, 47), (45, 35)]
    regions = _regions(shapes, 7)
    offsets, end = [], 0
    for cls, r in zip((0, 4, 8, 12), regions):
        off = -(-end // 16) * 16 + cls
        offsets.append(off)
        end = off + r.size
    assert [o % 16 for o in offsets] == [0, 4, 8, 12]
    total = end + 4
    mats = [[[w / size[0], 0, -0.5 + 0.5 * w / size[0]], [0, h / size[1], -0.5 + 0.5 * h / size[1]]] for h, w in shapes]
    colour = [(1.0, 0.0), (1.2, -0.1), (0.85, 0.15), (1.0, 0.0)]
    got = _warp(built_lib, regions, offsets, total, mats, colour, size)
    _compare(got, regions, mats, colour, size, "offset classes")
    # the last region alone, last in its buffer, integer-exact: its final pixel arrives bit for bit
    last = regions[-1]
    got = _warp(built_lib, [last], [12], 12 + last.size + 4, [[[1, 0, 35 - 192], [0, 1, 45 - 256]]], [(1.0, 0.0)], size)
    assert np.array_equal(got[0][:, -1, -1], last[-1, -1].astype(np.float32) / np.float32(255))
    assert np.array_equal(got[0][:, 256 - 45:, 192 - 35:], (last.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


# ---- keypoints, flags, maps --------------------------------------------------------------------------------------------
def test_keypoints_flags_and_maps(dataset):
    from probpose_pytorch_amd import _lib
    from probpose_pytorch_amd.dataset import augment_matrices
    lib = _lib.lib()
    anns = dataset.annotations
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    pm = dataset.codec.probmap
    scale = np.asarray(pm.scale_factor, dtype=np.float32)
    cases = [(a, p) for a in anns for p in AR.PARAM_GRID]
    B, K, (in_w, in_h) = len(cases), DR.K, DR.INPUT_SIZE
    want = [AR.keypoints(np.array(a["keypoints"], dtype=np.float32), a["bbox"], p, perm, DR.INPUT_SIZE, scale)
            for a, p in cases]
    for w in want:                                                     # on the CPU first: the inputs are fit
        margin = AR.border_margin(w["crop"], DR.INPUT_SIZE)
        assert margin.min() >= AR.MARGIN and (margin > w["bound"]).all()
    boxes = np.array([a["bbox"] for a, _ in cases])
    params = np.array([p for _, p in cases])
    origins = np.array([AR.region_rect(a["bbox"], p)[:2] for a, p in cases])
    _, keypoint = augment_matrices(boxes, origins, params, DR.INPUT_SIZE)
    aff = np.zeros((B, 8), dtype=np.float32)
    aff[:, :6], aff[:, 6] = keypoint.reshape(B, 6), params[:, 0]
    kps = np.stack([np.array(a["keypoints"], dtype=np.float32) for a, _ in cases])
    d_k, d_a = torch.from_numpy(kps).cuda(), torch.from_numpy(aff).cuda()
    d_p = torch.from_numpy(perm.astype(np.int32)).cuda()
    crop, hm = (torch.empty(B, K, 2, device="cuda") for _ in range(2))
    enc, visibility = (torch.empty(B, K, device="cuda") for _ in range(2))
    in_image, visible = (torch.empty(B, K, dtype=torch.bool, device="cuda") for _ in range(2))
    _lib.check(lib.pp_dataset_ground_truth_affine(_lib.ptr(d_k), _lib.ptr(d_a), _lib.ptr(d_p), B, K, in_w, in_h,
                                                  float(scale[0]), float(scale[1]), _lib.ptr(crop), _lib.ptr(hm),
                                                  _lib.ptr(enc), _lib.ptr(in_image), _lib.ptr(visible),
                                                  _lib.ptr(visibility), _lib.stream_ptr()),
               "pp_dataset_ground_truth_affine")
    g_crop, g_hm = crop.cpu().numpy().astype(np.float64), hm.cpu().numpy()
    worst_crop = worst_hm = 0.0
    flipped_moved = 0
    for i, w in enumerate(want):
        worst_crop = max(worst_crop, (np.abs(g_crop[i] - w["crop"]) / w["bound"]).max())
        worst_hm = max(worst_hm, (np.abs(g_hm[i].astype(np.float64) - w["hm"]) / w["hm_bound"]).max())
        assert np.array_equal(in_image[i].cpu().numpy(), w["in_image"]), cases[i]
        assert np.array_equal(visible[i].cpu().numpy(), w["visible"]), cases[i]
        assert np.array_equal(visibility[i].cpu().numpy(), w["visibility"].astype(np.float32)), cases[i]
        assert np.array_equal(enc[i].cpu().numpy(), w["visible"].astype(np.float32)), cases[i]
        if params[i, 0]:
            flipped_moved += int((w["visible"] != (kps[i, :, 2] == 2)).sum())
    print(f"keypoints: worst d/bound crop {worst_crop:.3f}, heatmap {worst_hm:.3f}")
    assert worst_crop <= 1.0 and worst_hm <= 1.0
    assert flipped_moved > 0                                           # the flip really moved visibility values
    assert any(w["in_image"].any() and not w["in_image"].all() for w in want)
    # maps: the oracle's generator on the device's own float32 heatmap keypoints, bit for bit
    heat, _ = pm.encode_device_tensors(hm, enc)
    heat = heat.cpu().numpy()
    g_vis = enc.cpu().numpy()
    for i in range(0, B, 5):
        ref, _ = orc.generate_probmaps(DR.HEATMAP_SIZE, g_hm[i][None], g_vis[i][None], DR.SIGMAS, -1)
        assert np.array_equal(heat[i], ref), cases[i]


# ---- whole batches -------------------------------------------------------------------------------------------------------
def _restated(dataset, epoch):
    perm = AR.permutation(AR.FLIP_PAIRS, DR.K)
    scale = np.asarray(dataset.codec.probmap.scale_factor, dtype=np.float32)
    out = []
    for i, ann in enumerate(dataset.annotations):
        params = dataset.augment.draw(epoch, i)
        img, kp = AR.sample(_frame(ann), ann["bbox"], np.array(ann["keypoints"], dtype=np.float32), params, perm,
                            DR.INPUT_SIZE, scale)
        margin = AR.border_margin(kp["crop"], DR.INPUT_SIZE)
        assert margin.min() >= AR.MARGIN and (margin > kp["bound"]).all(), (epoch, i)       # fit for exact flags
        heat, _ = orc.generate_probmaps(DR.HEATMAP_SIZE, kp["hm"][None], kp["visible"][None].astype(np.float32),
                                        DR.SIGMAS, -1)
        out.append(dict(img=img, kp=kp, heat=heat, params=params))
    return out


def _epoch(dataset, epoch):
    dataset.set_epoch(epoch)
    rows = []
    for img, gt in dataset.loader(batch_size=8, shuffle=True, num_workers=2):
        assert img.dtype == torch.float32 and tuple(img.shape[1:]) == (3, DR.INPUT_SIZE[1], DR.INPUT_SIZE[0])
        assert gt["heatmaps"].dtype == torch.float32 and gt["in_image"].dtype == torch.bool
        assert gt["keypoints_visible"].dtype == torch.bool and gt["keypoints_visibility"].dtype == torch.float32
        B = img.shape[0]
        assert tuple(gt["heatmaps"].shape) == (B, DR.K, DR.HEATMAP_SIZE[1], DR.HEATMAP_SIZE[0])
        assert all(tuple(gt[k].shape) == (B, 1, DR.K) for k in ("in_image", "keypoints_visible", "keypoints_visibility"))
        for b in range(B):
            rows.append((img[b].cpu().numpy(), {k: v[b].cpu().numpy() for k, v in gt.items()}))
    return rows


def _match(rows, want):
    """Row -> sample index (the loader shuffles): the restated image it is closest to.  Every comparison is asserted."""
    found = {}
    worst_img = worst_heat = 0.0
    for img, gt in rows:
        dist = [np.abs(img[:, ::8, ::8] - w["img"][:, ::8, ::8]).max() for w in want]
        i = int(np.argmin(dist))
        assert i not in found
        found[i] = (img, gt)
        w = want[i]
        ratio = np.abs(img.astype(np.float64) - w["img"]).max() / AR.warp_bound(w["params"][5], w["params"][6])
        worst_img = max(worst_img, ratio)
        assert ratio <= 1.0, (i, ratio)
        kp = w["kp"]
        assert np.array_equal(gt["in_image"][0], kp["in_image"]) and np.array_equal(gt["keypoints_visible"][0], kp["visible"])
        assert np.array_equal(gt["keypoints_visibility"][0], kp["visibility"].astype(np.float32))
        # a map value moves by at most max |d/dr exp(-r^2 / (2 s))| = exp(-1/2) / sqrt(s) <= 0.818 (s >= 0.55) per
        # heatmap pixel of keypoint error, in x and in y; 2 u for the float32 store on either side
        bound = 0.818 * kp["hm_bound"].sum(-1)[:, None, None] + 2 * U
        ratio = (np.abs(gt["heatmaps"].astype(np.float64) - w["heat"]) / bound).max()
        worst_heat = max(worst_heat, ratio)
        assert ratio <= 1.0, (i, ratio)
    assert sorted(found) == list(range(len(want)))
    print(f"whole batch: worst d/bound image {worst_img:.3f}, maps {worst_heat:.3f}")
    return found


def test_loader_batches_over_two_epochs(dataset):
    want0, want1 = _restated(dataset, 0), _restated(dataset, 1)
    first = _match(_epoch(dataset, 0), want0)
    again = _match(_epoch(dataset, 0), want0)
    second = _match(_epoch(dataset, 1), want1)
    assert max(w["heat"].max() for w in want0) > 0.5
    for i in first:
        assert np.array_equal(first[i][0], again[i][0])
        for k in first[i][1]:
            assert np.array_equal(first[i][1][k], again[i][1][k]), k
        assert not np.array_equal(first[i][0], second[i][0])
    # no host synchronisation in collate (once the per-dataset constants are on the device)
    dataset.set_epoch(0)
    samples = [dataset[i] for i in range(len(dataset))]
    img, gt = dataset.collate(samples)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        img2, gt2 = dataset.collate(samples)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(img, img2) and all(torch.equal(gt[k], gt2[k]) for k in gt)
    for i in first:
        assert np.array_equal(img[i].cpu().numpy(), first[i][0])          # the batch composition does not matter


def test_unaugmented_bits_are_unchanged(dataset, plain):
    anns = plain.annotations[:4]
    img, gt = plain.collate([plain[i] for i in range(4)])
    want_img, want = DR.batch(anns)
    assert np.array_equal(img.cpu().numpy(), want_img)
    for k in want:
        assert np.array_equal(gt[k].cpu().numpy(), want[k]), k
    for i in (1, 3):                                   # reference_item of an augmented dataset is the un-augmented item
        a_img, a_gt = dataset.reference_item(i)
        p_img, p_gt = plain.reference_item(i)
        assert torch.equal(a_img, p_img) and torch.equal(a_img, img[i])
        for k in p_gt:
            assert torch.equal(a_gt[k], p_gt[k]) and torch.equal(a_gt[k], gt[k][i]), k


def test_one_training_step_on_an_augmented_batch(dataset):
    """train.py's model at depth 2 (as tests/test_dataset_gpu.py builds it) takes one step on an augmented batch."""
    from probpose_pytorch_amd import FusedAdamW
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_head_state, synthetic_vit_state
    from tests import loss_grad_reference as LG
    K, C, heads, depth, size = DR.K, 384, 12, 2, DR.INPUT_SIZE
    dataset.set_epoch(0)
    img, gt = dataset.collate([dataset[i] for i in range(4)])
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 and float(img.std()) > 0.05
    loss_fn = ProbPoseLoss(dataset.codec, freeze_error=True, differentiable=True)
    backbone = ScratchViTBackbone(size, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True)
    backbone.model.load_state_dict(synthetic_vit_state(size, 16, C, depth, seed=12))
    head = ProbMapHead(C, K, [(4, 4), (2, 2), (2, 2)], (256, 256), (4, 4), final_layer_kernel_size=1, freeze_error=True,
                       normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().train()
    opt = FusedAdamW(model.parameters(), lr=3e-4, max_grad_norm=1.0)
    opt.zero_grad()
    losses = loss_fn(gt, model(img))
    loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
    loss.backward()
    opt.step()
    print("weighted loss on the augmented batch:", float(loss.detach()))
    assert np.isfinite(float(loss.detach())) and all(np.isfinite(float(v.detach())) for v in losses.values())
