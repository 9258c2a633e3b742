"""probpose.dataset on the GPU: ``collate`` against the reference's per-sample path (Pillow for the pixels, the oracle's
float64 generator for the maps), bit for bit; the multi-source launch against the single-frame one; the ground-truth
kernel against its numpy float32 restatement; staging-buffer reuse; workers; and train.py's loop fed by a collated
batch.  The parity batch is the one of tests/test_dataset.py (tests/dataset_reference.py writes the tree)."""
import numpy as np
import PIL.Image
import pytest
import torch

from oracle import frontend_oracle as fo
from tests import dataset_reference as DR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, built_lib):
    from probpose_pytorch_amd.codec import ArgMaxProbMap, Codec
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    tree = DR.write_tree(tmp_path_factory.mktemp("yolo"))
    return YOLOPoseDataset(tree.parent, tree.name, Codec(ArgMaxProbMap(DR.INPUT_SIZE, DR.HEATMAP_SIZE, DR.SIGMAS)),
                           target_single_class=0)


def _check_batch(img, gt, anns):
    B, (w, h), (W, H) = len(anns), DR.INPUT_SIZE, DR.HEATMAP_SIZE
    want_img, want = DR.batch(anns)
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (B, 3, h, w)
    shapes = dict(heatmaps=(B, DR.K, H, W), in_image=(B, 1, DR.K), keypoints_visible=(B, 1, DR.K),
                  keypoints_visibility=(B, 1, DR.K))
    dtypes = dict(heatmaps=torch.float32, in_image=torch.bool, keypoints_visible=torch.bool,
                  keypoints_visibility=torch.float32)
    assert set(gt) == set(shapes)
    got_img = img.cpu().numpy()
    for b, ann in enumerate(anns):
        assert np.array_equal(got_img[b], want_img[b]), ("img", ann["bbox"], np.abs(got_img[b] - want_img[b]).max())
    for k in shapes:
        assert gt[k].is_cuda and gt[k].dtype == dtypes[k] and tuple(gt[k].shape) == shapes[k], k
        g = gt[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        for b, ann in enumerate(anns):
            assert np.array_equal(g[b], want[k][b]), (k, ann["bbox"])
    return want_img, want


def test_collate_equals_the_reference_items(dataset):
    samples = [dataset[i] for i in range(len(dataset))]
    assert len(samples) == 9
    img, gt = dataset.collate(samples)
    _, want = _check_batch(img, gt, dataset.annotations)
    assert want["heatmaps"].max() > 0.5                                       # the batch has real maps in it
    assert want["in_image"].any() and not want["in_image"].all()


def test_batch_of_one_and_unlabelled_instance(dataset):
    i = [b for b, a in enumerate(dataset.annotations) if round(a["bbox"][2]) == 37][0]
    img, gt = dataset.collate([dataset[i]])
    _, want = _check_batch(img, gt, [dataset.annotations[i]])
    assert float(gt["heatmaps"].abs().max()) == 0.0 and not bool(gt["keypoints_visible"].any())
    assert float(gt["keypoints_visibility"].abs().max()) == 0.0
    assert want["in_image"].any() and np.array_equal(gt["in_image"].cpu().numpy(), want["in_image"])
    with pytest.raises(ValueError):
        dataset.collate([])


def test_reference_item_equals_the_batch_row(dataset):
    img, gt = dataset.collate([dataset[i] for i in range(len(dataset))])
    for i in (0, 3, 8):
        one, g1 = dataset.reference_item(i)
        assert tuple(one.shape) == (3, DR.INPUT_SIZE[1], DR.INPUT_SIZE[0]) and torch.equal(one, img[i])
        assert tuple(g1["heatmaps"].shape) == (DR.K, DR.HEATMAP_SIZE[1], DR.HEATMAP_SIZE[0])
        for k in gt:
            assert torch.equal(g1[k], gt[k][i]), k
        for k in ("in_image", "keypoints_visible", "keypoints_visibility"):
            assert tuple(g1[k].shape) == (1, DR.K)


def test_single_frame_through_the_multi_source_entry(built_lib):
    """One region, many boxes that all name it == frontend.crop_resize on the same frame, for both sizes' paths."""
    from probpose_pytorch_amd import frontend
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    frame = DR._frame(480, 640, 5)
    boxes_xywh = [(10.0, 20.0, 100.0, 200.0), (50.2, 60.7, 300.4, 420.9), (0.5, 1.5, 192.0, 256.0),
                  (33.0, 44.0, 192.0, 256.0), (5.0, 5.0, 192.0, 100.0), (5.0, 5.0, 80.0, 256.0),
                  (-30.0, -40.0, 150.0, 300.0), (500.0, 380.0, 200.0, 200.0), (100.0, 100.0, 1.0, 1.0),
                  (0.0, 0.0, 640.0, 480.0), (200.0, 100.0, 37.0, 51.0), (639.0, 479.0, 1.0, 1.0),
                  (600.0, 440.0, 40.0, 40.0)]
    (off,), total = YOLOPoseDataset.pack_layout([frame.shape[:2]])
    packed = torch.zeros(total, dtype=torch.uint8)
    packed[off:off + frame.size] = torch.from_numpy(frame.reshape(-1))
    d_packed, d_frame = packed.cuda(), torch.from_numpy(frame).cuda()
    boxes = frontend.round_boxes(boxes_xywh)
    sources = np.tile(np.array([[off, 640, 480, 3 * 640]], dtype=np.int64), (len(boxes), 1))
    for size in ((192, 256), (384, 384)):
        plan = np.zeros(frontend.multi_plan_bytes(boxes, size) // 4, dtype=np.int32)
        n_blocks, lds = frontend.multi_plan_build(boxes, sources, total, size, plan.ctypes.data)
        got = frontend.crop_resize_multi(d_packed, torch.from_numpy(plan).cuda(), len(boxes), n_blocks, lds, size)
        want = frontend.crop_resize(d_frame, boxes_xywh, size)
        assert torch.equal(got, want), size
        for i in (6, 7, 11):
            assert np.array_equal(got[i].cpu().numpy(), fo.scale_box_pil(frame, boxes_xywh[i], size))


def test_ground_truth_kernel_equals_the_float32_restatement(built_lib):
    from probpose_pytorch_amd import _lib
    rng = np.random.default_rng(5)
    B, K, (w, h) = 7, 20, DR.INPUT_SIZE
    boxes = np.stack([rng.uniform(-50, 900, B), rng.uniform(-50, 600, B), rng.uniform(1, 700, B),
                      rng.uniform(1, 700, B)], -1)
    boxes[0] = (64.0, 32.0, 128.0, 128.0)
    kps = np.concatenate([rng.uniform(-100, 1500, (B, K, 2)), rng.integers(0, 2, (B, K, 1)) * 2.0], -1).astype(np.float32)
    kps[0, :3, :2] = [(64.0, 32.0), (192.0, 100.0), (100.0, 160.0)]      # exactly 0, exactly in_w, exactly in_h
    scale = ((np.array(DR.INPUT_SIZE) - 1) / (np.array(DR.HEATMAP_SIZE) - 1)).astype(np.float32)
    d_k, d_b = torch.from_numpy(kps).cuda(), torch.from_numpy(boxes).cuda()
    crop, hm = (torch.empty(B, K, 2, device="cuda") for _ in range(2))
    enc, visibility = (torch.empty(B, K, device="cuda") for _ in range(2))
    in_image, visible = (torch.empty(B, K, dtype=torch.bool, device="cuda") for _ in range(2))
    _lib.check(built_lib.pp_dataset_ground_truth(_lib.ptr(d_k), _lib.ptr(d_b), B, K, w, h, float(scale[0]),
                                                 float(scale[1]), _lib.ptr(crop), _lib.ptr(hm), _lib.ptr(enc),
                                                 _lib.ptr(in_image), _lib.ptr(visible), _lib.ptr(visibility),
                                                 _lib.stream_ptr()), "pp_dataset_ground_truth")
    want = DR.ground_truth_f32(kps, boxes, DR.INPUT_SIZE, scale)
    for g, wnt in zip((crop, hm, in_image, visible, visibility), want):
        assert np.array_equal(g.cpu().numpy(), wnt)
    assert np.array_equal(enc.cpu().numpy(), want[3].astype(np.float32))
    assert want[0][0, 0, 0] == 0 and want[0][0, 1, 0] == w and want[0][0, 2, 1] == h
    assert want[2][0, 0] and not want[2][0, 1] and not want[2][0, 2]


def test_repeated_collate_with_copies_in_flight(dataset):
    """Two collates issued behind a long kernel queue: the first one's copies have not run when the second packs its
    buffers, so it must take fresh staging buffers; all calls give the same bits."""
    samples = [dataset[i] for i in range(len(dataset))] * 4           # B = 36
    first_img, first = dataset.collate(samples)
    torch.cuda.synchronize()
    before = len(dataset._staging)
    x = torch.randn(8192, 8192, device="cuda")
    for _ in range(12):
        x = (x @ x) * 1e-4
    a = dataset.collate(samples)
    b = dataset.collate(samples)
    assert len(dataset._staging) >= before + 2                        # b could not reuse what a's copies still read
    torch.cuda.synchronize()
    taken = len(dataset._staging)
    c = dataset.collate(samples)
    assert len(dataset._staging) == taken                             # everything has completed: buffers are reused
    for img, gt in (a, b, c):
        assert torch.equal(img, first_img)
        for k in first:
            assert torch.equal(gt[k], first[k]), k


def test_loader_with_workers_equals_collate(dataset):
    want_img, want = dataset.collate([dataset[i] for i in range(len(dataset))])
    for workers in (0, 2):
        batches = list(dataset.loader(4, num_workers=workers))
        assert [int(b[0].shape[0]) for b in batches] == [4, 4, 1]
        assert torch.equal(torch.cat([b[0] for b in batches]), want_img)
        for k in want:
            assert torch.equal(torch.cat([b[1][k] for b in batches]), want[k]), k


def test_train_py_loop_on_a_collated_batch(dataset):
    """The reduced-depth model of tests/test_model_train_gpu.py (depth 2, K = 20, 384x384, 96x96 maps) with
    FusedAdamW(max_grad_norm=1.0): the losses on a collated batch are the losses on the batch the reference's
    per-sample path builds (both hold the same numbers), and six steps on it lower the weighted loss."""
    from probpose_pytorch_amd import FusedAdamW
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.loss import ProbPoseLoss
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_head_state, synthetic_vit_state
    from tests import loss_grad_reference as LG
    K, C, heads, depth, size = DR.K, 384, 12, 2, DR.INPUT_SIZE
    pools = [(4, 4), (2, 2), (2, 2)]
    anns = dataset.annotations[:4]
    img, gt = dataset.collate([dataset[i] for i in range(4)])
    ref_img, ref_gt = DR.batch(anns)
    ref_gt = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ref_gt.items()}
    assert torch.equal(img.cpu(), torch.from_numpy(ref_img))
    loss_fn = ProbPoseLoss(dataset.codec, freeze_error=True, differentiable=True)
    backbone = ScratchViTBackbone(size, 16, embed_dim=C, depth=depth, num_heads=heads, differentiable=True)
    backbone.model.load_state_dict(synthetic_vit_state(size, 16, C, depth, seed=12))
    head = ProbMapHead(C, K, pools, (256, 256), (4, 4), final_layer_kernel_size=1, freeze_error=True,
                       normalize=1.0, differentiable=True)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=3, deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().train()
    opt = FusedAdamW(model.parameters(), lr=3e-4, max_grad_norm=1.0)
    hist = []
    for step in range(6):
        opt.zero_grad()
        pred = model(img)
        losses = loss_fn(gt, pred)
        if step == 0:
            ref_losses = loss_fn(ref_gt, pred)
            assert set(losses) == set(ref_losses)
            for k in losses:
                print(k, float(losses[k].detach()), float(ref_losses[k].detach()))
                assert torch.equal(losses[k].detach(), ref_losses[k].detach()), k
        loss = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))
        loss.backward()
        hist.append(float(loss.detach()))
        opt.step()
    print("weighted loss per step:", hist)
    assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
