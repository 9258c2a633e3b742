"""TEST INFRASTRUCTURE ONLY: numpy / PIL restatement of the reference's probpose/dataset.py (parse_annotations,
scale_box, YOLOPoseDataset.__getitem__ and torch's default collate of its items), written from its behaviour, plus the
small YOLO tree tests/test_dataset.py and tests/test_dataset_gpu.py share.

Pixels go through Pillow itself (oracle.frontend_oracle.scale_box_pil), the maps through the oracle's generator
(oracle.probpose_oracle.probmap_encode).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import PIL.Image

from oracle import frontend_oracle as fo
from oracle import probpose_oracle as orc

K = 20
INPUT_SIZE = (384, 384)       # [w, h]
HEATMAP_SIZE = (96, 96)       # [W, H]
SIGMAS = np.linspace(0.025, 0.107, K)


# ---- the reference, restated -------------------------------------------------------------------------------------------
def parse_annotations(split_folder, target_single_class=None):
    """One record per label line of every image that has a label file, in directory order; boxes centre -> corner in
    pixels, keypoints in pixels, visibility 1 stored as 2, every category 0."""
    split_folder = Path(split_folder)
    out = []
    for image_path in list((split_folder / "images").iterdir()):
        with PIL.Image.open(image_path) as im:
            width, height = im.size
        label = split_folder / "labels" / (image_path.stem + ".txt")
        if not label.exists():
            continue
        for line in label.read_text().splitlines(keepends=True):
            f = line.strip().split()
            if target_single_class is not None and int(f[0]) != target_single_class:
                continue
            xc, yc, bw, bh = float(f[1]) * width, float(f[2]) * height, float(f[3]) * width, float(f[4]) * height
            kps = []
            for j in range(5, len(f), 3):
                v = int(f[j + 2])
                kps.append([float(f[j]) * width, float(f[j + 1]) * height, 2 if v == 1 else v])
            out.append(dict(image_path=str(image_path), category_id=0, bbox=[xc - bw / 2, yc - bh / 2, bw, bh],
                            keypoints=kps))
    return out


def scale_box(image: np.ndarray, bbox, image_size, kps: np.ndarray):
    """Crop + LANCZOS resize on Pillow (as float32 CHW in [0, 1]) and the keypoints moved into the crop's frame with
    the un-rounded box; kps float32, bbox Python floats: numpy's float32 arithmetic."""
    img = fo.scale_box_pil(image, bbox, image_size)
    kps[:, 0] = (kps[:, 0] - bbox[0]) / bbox[2] * image_size[0]
    kps[:, 1] = (kps[:, 1] - bbox[1]) / bbox[3] * image_size[1]
    return img, kps


def getitem(ann, input_size=INPUT_SIZE, heatmap_size=HEATMAP_SIZE, sigmas=SIGMAS, sigma=-1):
    with PIL.Image.open(ann["image_path"]) as im:
        frame = np.asarray(im.convert("RGB"), dtype=np.uint8)
    img, kps = scale_box(frame, ann["bbox"], input_size, np.array(ann["keypoints"], dtype=np.float32))
    kps = kps[None, :, :]
    visible = kps[:, :, 2] == 2
    visibility = np.minimum(kps[:, :, 2], 1)
    enc = orc.probmap_encode(kps[:, :, :2], visible, input_size, heatmap_size, sigmas, sigma)
    return img, dict(heatmaps=enc["heatmaps"], in_image=enc["in_image"], keypoints_visible=visible,
                     keypoints_visibility=visibility)


def batch(anns, **kw):
    """What torch's default collate makes of the items: stacked along a new first axis."""
    items = [getitem(a, **kw) for a in anns]
    return (np.stack([i[0] for i in items]),
            {k: np.stack([i[1][k] for i in items]) for k in items[0][1]})


def ground_truth_f32(kps_raw: np.ndarray, boxes: np.ndarray, input_size, scale_factor):
    """The device's ground-truth arithmetic, operation by operation in numpy float32.  kps_raw [B, K, 3] f32, boxes
    [B, 4] f64 -> crop-frame keypoints, heatmap-pixel keypoints, in_image, keypoints_visible, keypoints_visibility."""
    f = np.float32
    b = boxes.astype(f)[:, None, :]
    x = ((kps_raw[..., 0] - b[..., 0]) / b[..., 2]) * f(input_size[0])
    y = ((kps_raw[..., 1] - b[..., 1]) / b[..., 3]) * f(input_size[1])
    crop = np.stack([x, y], -1)
    assert crop.dtype == f
    hm = crop / np.asarray(scale_factor, dtype=f)
    in_image = (x >= 0) & (x < f(input_size[0])) & (y >= 0) & (y < f(input_size[1]))
    v = kps_raw[..., 2]
    return crop, hm, in_image, v == 2, np.minimum(v, f(1))


# ---- the shared tree ---------------------------------------------------------------------------------------------------
def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = ((np.sin(xx / 13.0) + np.cos(yy / 19.0)) * 60 + 128).clip(0, 255).astype(np.uint8)
    img[:, : w // 2] = (img[:, : w // 2] // 4 + smooth[:, : w // 2, None] * 3 // 4).astype(np.uint8)
    return img


# frames (h, w); frame "a" has power-of-two sides, so that pixel / side * side is exact for its dyadic boxes
FRAMES = {"a": (256, 512), "b": (360, 500), "c": (720, 1280), "unlabelled": (100, 120)}
# (frame, class, [x, y, w, h] in pixels, what it is there for)
INSTANCES = [
    ("a", 0, (0.5, 1.5, 192.0, 200.0), ".5 corners: round-half-to-even"),
    ("a", 0, (64.0, 32.0, 128.0, 128.0), "up-scaled; keypoints exactly on 0 and on in_w"),
    ("a", 0, (100.0, 50.0, 1.0, 40.0), "one pixel wide"),
    ("a", 0, (-30.0, -40.0, 150.0, 290.0), "leaves the frame top-left and bottom"),
    ("a", 1, (10.0, 10.0, 80.0, 120.0), "another class"),
    ("b", 0, (50.2, 60.7, 300.4, 270.9), "fractional corners"),
    ("b", 0, (380.0, 250.0, 200.0, 200.0), "leaves the frame bottom-right"),
    ("b", 0, (200.0, 100.0, 37.0, 51.0), "up-scaled, all keypoints unlabelled"),
    ("c", 0, (100.0, 30.0, 700.0, 650.0), "down-scaled"),
    ("c", 0, (600.0, 200.0, 384.0, 384.0), "identity size: a copy"),
    ("c", 1, (900.5, 100.25, 250.0, 500.0), "down-scaled vertically, another class"),
]


def write_tree(root, split="train"):
    """Write the frames as PNG and one label file per labelled frame under root/split; returns root / split."""
    folder = Path(root) / split
    (folder / "images").mkdir(parents=True)
    (folder / "labels").mkdir()
    rng = np.random.default_rng(2024)
    lines = {name: [] for name in FRAMES}
    for n, (name, cls, (x, y, w, h), what) in enumerate(INSTANCES):
        H, W = FRAMES[name]
        # keypoints around the box, some outside it; flags 0, 1 and 2
        kx = rng.uniform(x - 0.15 * w, x + 1.15 * w, K)
        ky = rng.uniform(y - 0.15 * h, y + 1.15 * h, K)
        v = rng.integers(0, 3, K)
        if "on 0 and on in_w" in what:
            kx[:3], ky[:3], v[:3] = (64.0, 192.0, 100.0), (32.0, 100.0, 160.0), (2, 2, 1)
        if "unlabelled" in what:
            v[:] = 0
        fields = [str(cls)] + [repr(float(t)) for t in ((x + w / 2) / W, (y + h / 2) / H, w / W, h / H)]
        for i in range(K):
            fields += [repr(float(kx[i] / W)), repr(float(ky[i] / H)), str(int(v[i]))]
        lines[name].append(" ".join(fields))
    for seed, (name, (H, W)) in enumerate(FRAMES.items()):
        PIL.Image.fromarray(_frame(H, W, 100 + seed), "RGB").save(folder / "images" / f"{name}.png")
        if lines[name]:
            (folder / "labels" / f"{name}.txt").write_text("\n".join(lines[name]) + "\n")
    return folder
