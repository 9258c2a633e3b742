"""Mirror of the reference's ``probpose/dataset.py``: YOLO pose annotations -> ``(img, gt)`` training batches.

The reference does everything per sample in DataLoader workers (dataset.py:116-135: PIL crop, LANCZOS resize, ToDtype,
keypoint rescale, ``codec.encode`` = K float64 numpy maps).  Here a worker only reads and decodes the file and cuts
the integer crop region out of it (``__getitem__``, CPU only); ``collate`` assembles the batch on the GPU:

* the B regions are packed into one pinned staging buffer and copied asynchronously, the plan (per-box Pillow
  coefficient tables, source records, workgroup table) together with the raw keypoints and the un-rounded boxes in a
  second asynchronous copy;
* three launches: the multi-source crop/resize (csrc/pp_frontend.hip, bit-identical to Pillow), the ground-truth
  assembly (csrc/pp_dataset.hip: crop-frame and heatmap-pixel keypoints, the three flag arrays) and
  ``pp_encode_probmaps`` on those device buffers.

No host synchronisation and no per-sample launch.  There is no CPU fallback: ``collate`` needs the GPU.

With ``augment=Augment(...)`` the samples are flipped, scaled, rotated, shifted and colour-jittered on the way: the
worker draws the sample's parameters from a counter-based generator keyed by (seed, epoch, index) and cuts the bounding
rectangle of the transformed box; ``collate`` folds the geometry into two 2x3 matrices per sample and replaces launches
one and two by ``pp_augment_warp`` (bilinear) and ``pp_dataset_ground_truth_affine`` (csrc/pp_augment.hip).  With
``augment=None`` nothing changes.

``Augment`` has three more steps, off by default: a half-body crop replaces the sample's box in the worker
before anything else looks at it; a box or median blur and random erasing ride along as one int32 record per sample
(a sixth tuple entry) and cost one more launch, ``pp_augment_post`` (csrc/pp_augment_post.hip), between the warp and
the keypoint kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path
from typing import Sequence, Tuple

import numpy as np
import PIL.Image
import torch
from torch.utils.data import DataLoader, Dataset, get_worker_info

from . import _lib, frontend
from ._buffers import PinnedStaging
from .flip import pair_permutation

_REGION_ALIGN = 16          # byte alignment of a region in the packed buffer (a multiple of frontend.SRC_ALIGN)
MAX_WORKERS = 15            # 16 processes may hold one GPU open: the workers (which inherit it) plus the main process


def _image_size(path: str):
    """(width, height) from the file header: ``pymage_size`` as the reference (dataset.py:24) where it is installed,
    else Pillow, which reads only the header for ``.size`` as well."""
    try:
        import pymage_size
    except ImportError:
        with PIL.Image.open(path) as im:
            return im.size
    return pymage_size.get_image_size(path).get_dimensions()


def _track(seq):
    try:
        from rich.progress import track
    except ImportError:
        return seq
    return track(seq)


def parse_annotations(split_folder: Path, target_single_class: int | None = None):
    """Reference dataset.py:20-68: one dict per labelled instance of ``split_folder/images/*`` with the keys
    image_path, category_id (always 0), bbox [x, y, w, h] in pixels and keypoints [[x, y, v], ...] in pixels, a
    labelled visibility of 1 stored as 2.  Images without a label file are skipped."""
    split_folder = Path(split_folder)
    annotations = []
    image_paths = list((split_folder / "images").iterdir())
    for image_path in _track(image_paths):
        width, height = _image_size(str(image_path))
        label_path = split_folder / "labels" / image_path.with_suffix(".txt").name
        if not label_path.exists():
            print(f"Label file {label_path} does not exist, skipping image {image_path.name}")
            continue
        with open(label_path, "r") as f:
            lines = f.readlines()
        for line in lines:
            parts = line.strip().split()
            if target_single_class is not None and int(parts[0]) != target_single_class:
                continue
            xc, yc = float(parts[1]) * width, float(parts[2]) * height
            bw, bh = float(parts[3]) * width, float(parts[4]) * height
            kps = []
            for j in range(5, len(parts), 3):
                v = int(parts[j + 2])
                kps.append([float(parts[j]) * width, float(parts[j + 1]) * height, 2 if v == 1 else v])
            annotations.append({"image_path": str(image_path), "category_id": 0,
                                "bbox": [xc - bw / 2, yc - bh / 2, bw, bh], "keypoints": kps})
    return annotations


@dataclass(frozen=True)
class Augment:
    """Random augmentation of a training sample, applied on the GPU by ``YOLOPoseDataset.collate``.

    flip_pairs   (i, j) keypoint index pairs that trade places under a horizontal flip; disjoint, below K
    flip_prob    probability of the flip
    scale        (lo, hi): a uniform factor on the box size; above 1 shows more context
    rotate_deg   the angle is uniform in +-rotate_deg, applied with probability rotate_prob
    shift        uniform +- fraction of the box width / height added to the box centre
    brightness   b uniform in +-brightness;  contrast: c uniform in 1 +- contrast;  pixel = clamp(c * x + b, 0, 1)
    seed         key of the generator

    For output pixel (u, v) of an in_w x in_h crop: n = ((u + 0.5) / in_w - 0.5, (v + 0.5) / in_h - 0.5); with flip
    n.x = -n.x; p = (n.x * bw * s, n.y * bh * s); the source point is centre + (tx * bw, ty * bh) + R(theta) p in image
    pixels with pixel centres at half-integers, R(theta) = [[cos, -sin], [sin, cos]].  The box is stretched to the
    input size as the un-augmented path stretches it; the rotation is a rotation in image space.  The pixels are
    bilinear, not LANCZOS: identity parameters give the un-augmented geometry, not its bits.

    Three more steps, all off by default:

    half_body_prob, upper_body, half_body_min_keypoints, half_body_padding
                 with probability half_body_prob a sample with at least half_body_min_keypoints labelled keypoints
                 (v > 0) is cut around its upper body (the indices of ``upper_body``) or its lower body (every other
                 index below K): see ``half_body_box``.  Every keypoint keeps its label; those outside the new crop
                 come out with in_image = 0.
    blur_prob, blur_kernel (lo, hi)
                 box blur of the warped crop: the mean of a k x k window, k uniform over the odd sizes in [lo, hi]
                 (3, 5, 7), reflect-101 borders
    median_prob, median_kernel (lo, hi)
                 median blur instead, sizes 3 and 5; blur_prob + median_prob <= 1, a sample gets at most one of them
    erase_prob, erase_holes (lo, hi), erase_size (lo, hi), erase_fill
                 with probability erase_prob, lo..hi rectangles (at most 4) of the crop are set to erase_fill, the
                 width and the height of each an independent uniform fraction in erase_size of the crop's
    Blur and erasing act on the pixels after the warp and change no label (``draw_post``)."""
    flip_pairs: Sequence[Tuple[int, int]] = ()
    flip_prob: float = 0.5
    scale: Tuple[float, float] = (0.75, 1.25)
    rotate_deg: float = 40.0
    rotate_prob: float = 0.6
    shift: float = 0.0
    brightness: float = 0.2
    contrast: float = 0.2
    seed: int = 0
    half_body_prob: float = 0.0
    upper_body: Sequence[int] = ()
    half_body_min_keypoints: int = 9
    half_body_padding: float = 1.5
    blur_prob: float = 0.0
    blur_kernel: Tuple[int, int] = (3, 7)
    median_prob: float = 0.0
    median_kernel: Tuple[int, int] = (3, 5)
    erase_prob: float = 0.0
    erase_holes: Tuple[int, int] = (1, 1)
    erase_size: Tuple[float, float] = (0.2, 0.4)
    erase_fill: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "flip_pairs", tuple((int(i), int(j)) for i, j in self.flip_pairs))
        object.__setattr__(self, "scale", (float(self.scale[0]), float(self.scale[1])))
        if not 0 < self.scale[0] <= self.scale[1]:
            raise ValueError(f"Augment: scale={self.scale}; expected 0 < lo <= hi")
        if not (0 <= self.flip_prob <= 1 and 0 <= self.rotate_prob <= 1):
            raise ValueError("Augment: flip_prob and rotate_prob are probabilities")
        if self.shift < 0 or self.brightness < 0 or self.contrast < 0 or self.rotate_deg < 0 or self.seed < 0:
            raise ValueError("Augment: shift, brightness, contrast, rotate_deg and seed must not be negative")
        object.__setattr__(self, "upper_body", tuple(int(i) for i in self.upper_body))
        object.__setattr__(self, "erase_size", (float(self.erase_size[0]), float(self.erase_size[1])))
        object.__setattr__(self, "erase_fill", float(self.erase_fill))
        for name in ("half_body_prob", "blur_prob", "median_prob", "erase_prob"):
            if not 0 <= getattr(self, name) <= 1:
                raise ValueError(f"Augment: {name}={getattr(self, name)} is not a probability")
        if self.blur_prob + self.median_prob > 1:
            raise ValueError("Augment: blur_prob + median_prob exceeds 1 (a sample gets one filter at most)")
        for name, allowed in (("blur_kernel", (3, 5, 7)), ("median_kernel", (3, 5))):
            lo, hi = getattr(self, name)
            if lo != int(lo) or hi != int(hi) or int(lo) not in allowed or int(hi) not in allowed or lo > hi:
                raise ValueError(f"Augment: {name}={(lo, hi)}; expected lo <= hi, both of the odd sizes {allowed}")
            object.__setattr__(self, name, (int(lo), int(hi)))
        lo, hi = self.erase_holes
        if lo != int(lo) or hi != int(hi) or not 1 <= lo <= hi <= 4:
            raise ValueError(f"Augment: erase_holes={(lo, hi)}; expected 1 <= lo <= hi <= 4")
        object.__setattr__(self, "erase_holes", (int(lo), int(hi)))
        if not 0 < self.erase_size[0] <= self.erase_size[1] <= 1:
            raise ValueError(f"Augment: erase_size={self.erase_size}; expected 0 < lo <= hi <= 1")
        if not math.isfinite(self.erase_fill) or not math.isfinite(float(np.float32(self.erase_fill))):
            raise ValueError(f"Augment: erase_fill={self.erase_fill} is not a finite float32")
        if self.half_body_prob > 0 and not self.upper_body:
            raise ValueError("Augment: half_body_prob > 0 needs the keypoint indices of upper_body")
        if any(i < 0 for i in self.upper_body) or len(set(self.upper_body)) != len(self.upper_body):
            raise ValueError(f"Augment: upper_body={self.upper_body}; expected distinct indices, none negative")
        if self.half_body_min_keypoints < 0 or not self.half_body_padding > 0:
            raise ValueError("Augment: half_body_min_keypoints must not be negative and half_body_padding must be positive")

    @property
    def post(self) -> bool:
        """Does a sample carry a ``draw_post`` record (any of blur, median blur and erasing switched on)?"""
        return self.blur_prob > 0 or self.median_prob > 0 or self.erase_prob > 0

    def draw(self, epoch: int, idx: int) -> np.ndarray:
        """float64 [flip (0 or 1), s, theta (radians), tx, ty, c, b] of sample ``idx`` in epoch ``epoch``: a pure
        function of (seed, epoch, idx).  Eight uniforms are drawn whatever the settings, so that changing one setting
        leaves the other parameters of every sample as they were."""
        r = np.random.Generator(np.random.Philox(key=int(self.seed), counter=[int(epoch), int(idx), 0, 0])).random(8)
        lo, hi = self.scale
        theta = math.radians((2.0 * r[3] - 1.0) * self.rotate_deg) if r[2] < self.rotate_prob else 0.0
        return np.array([1.0 if r[0] < self.flip_prob else 0.0, lo + r[1] * (hi - lo), theta,
                         (2.0 * r[4] - 1.0) * self.shift, (2.0 * r[5] - 1.0) * self.shift,
                         1.0 + (2.0 * r[6] - 1.0) * self.contrast, (2.0 * r[7] - 1.0) * self.brightness],
                        dtype=np.float64)

    def _uniforms(self, epoch: int, idx: int, stream: int, count: int) -> np.ndarray:
        """``count`` uniforms of sample ``idx`` in epoch ``epoch`` from the counter [epoch, idx, stream, 0]; stream 0
        is ``draw``'s, so the streams here never change what ``draw`` returns."""
        return np.random.Generator(np.random.Philox(key=int(self.seed),
                                                    counter=[int(epoch), int(idx), int(stream), 0])).random(count)

    def half_body_box(self, epoch: int, idx: int, keypoints, bbox) -> np.ndarray:
        """float64 [x, y, w, h]: the box of sample ``idx`` in epoch ``epoch``, a pure function of (seed, epoch, idx)
        and the sample's annotation.  Two uniforms from the counter [epoch, idx, 2, 0], whatever the settings.

        The sample qualifies when r0 < half_body_prob and it has at least half_body_min_keypoints labelled keypoints
        (v > 0).  With >= 2 labelled upper-body and >= 3 labelled lower-body keypoints the upper body is taken when
        r1 < 0.7, else the lower; with only one half sufficient, that half; else, or when the sample does not
        qualify, ``bbox`` is returned as it is.  The new box is centred on the midpoint of the extents of the chosen
        labelled keypoints, each side max(extent * half_body_padding, 0.25 * the original side), and is not clipped
        to the frame (the region crop pads with zero)."""
        r = self._uniforms(epoch, idx, 2, 2)
        bbox = np.array(bbox, dtype=np.float64).reshape(4)
        kps = np.asarray(keypoints, dtype=np.float64).reshape(-1, 3)
        K = kps.shape[0]
        if any(i >= K for i in self.upper_body):
            raise ValueError(f"Augment: upper_body={self.upper_body} names a keypoint outside 0..{K - 1}")
        labelled = kps[:, 2] > 0
        if not (r[0] < self.half_body_prob and int(labelled.sum()) >= self.half_body_min_keypoints):
            return bbox
        is_upper = np.zeros(K, dtype=bool)
        is_upper[list(self.upper_body)] = True
        upper, lower = labelled & is_upper, labelled & ~is_upper
        upper_ok, lower_ok = int(upper.sum()) >= 2, int(lower.sum()) >= 3
        if upper_ok and lower_ok:
            chosen = upper if r[1] < 0.7 else lower
        elif upper_ok or lower_ok:
            chosen = upper if upper_ok else lower
        else:
            return bbox
        lo, hi = kps[chosen, :2].min(0), kps[chosen, :2].max(0)
        centre = (lo + hi) / 2
        side = np.maximum((hi - lo) * self.half_body_padding, 0.25 * bbox[2:])
        return np.concatenate([centre - side / 2, side])

    def draw_post(self, epoch: int, idx: int, input_size) -> np.ndarray:
        """int32 [24], the record of sample ``idx`` in epoch ``epoch`` that ``pp_augment_post`` takes: {kind, k,
        n_holes, fill (float32 bits), 4 x {x0, y0, x1, y1}, 4 x 0}; kind 0 none (k = 0), 1 box blur, 2 median blur;
        the rectangles half-open, in pixels of the in_w x in_h crop.  Twenty uniforms from the counter
        [epoch, idx, 1, 0], whatever the settings: r0 the kind, r1 the size, r2 and r3 whether and how many holes,
        r[4 + 4 j .. 7 + 4 j] width, height, x0 and y0 of hole j."""
        r = self._uniforms(epoch, idx, 1, 20)
        in_w, in_h = int(input_size[0]), int(input_size[1])
        rec = np.zeros(24, dtype=np.int32)
        kind = 1 if r[0] < self.blur_prob else 2 if r[0] < self.blur_prob + self.median_prob else 0
        if kind:
            lo, hi = self.blur_kernel if kind == 1 else self.median_kernel
            sizes = list(range(lo, hi + 1, 2))
            rec[0], rec[1] = kind, sizes[min(int(r[1] * len(sizes)), len(sizes) - 1)]
        lo, hi = self.erase_holes
        rec[2] = lo + min(int(r[3] * (hi - lo + 1)), hi - lo) if r[2] < self.erase_prob else 0
        rec[3] = np.float32(self.erase_fill).view(np.int32)
        elo, ehi = self.erase_size
        for j in range(int(rec[2])):
            rw, rh, rx, ry = r[4 + 4 * j:8 + 4 * j]
            w = min(max(int(round((elo + rw * (ehi - elo)) * in_w)), 1), in_w)
            h = min(max(int(round((elo + rh * (ehi - elo)) * in_h)), 1), in_h)
            x0, y0 = min(int(rx * (in_w - w + 1)), in_w - w), min(int(ry * (in_h - h + 1)), in_h - h)
            rec[4 + 4 * j:8 + 4 * j] = (x0, y0, x0 + w, y0 + h)
        return rec

    def permutation(self, K: int) -> np.ndarray:
        """int32 [K]: the keypoint that output slot k of a flipped sample reads."""
        return pair_permutation(self.flip_pairs, K, "Augment")


def augment_region(bbox, params) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1) of the pixels the warp of a sample can read: the bounding rectangle of the scaled, rotated,
    shifted box, rounded outward, plus the one pixel on every side that a bilinear tap next to its edge reaches."""
    x, y, bw, bh = (float(v) for v in bbox)
    _, s, theta, tx, ty, _, _ = (float(v) for v in params)
    cx, cy = x + bw / 2 + tx * bw, y + bh / 2 + ty * bh
    hw, hh, co, si = bw * s / 2, bh * s / 2, math.cos(theta), math.sin(theta)
    xs = [cx + co * px - si * py for px in (-hw, hw) for py in (-hh, hh)]
    ys = [cy + si * px + co * py for px in (-hw, hw) for py in (-hh, hh)]
    return (math.floor(min(xs)) - 1, math.floor(min(ys)) - 1, math.ceil(max(xs)) + 1, math.ceil(max(ys)) + 1)


def augment_matrices(bboxes, origins, params, input_size):
    """The geometry of ``Augment`` as matrices, numpy float64, for B samples at once.  bboxes [B, 4] un-rounded
    [x, y, w, h], origins [B, 2] of the regions in image pixels, params [B, 7] of ``Augment.draw``.  Returns
    (pixel [B, 2, 3], keypoint [B, 2, 3]): ``pixel`` maps an output pixel index (u, v, 1) to the region's pixel-index
    coordinates (pixel (i, j) centred at (i, j): the half-integer centres of image and crop are folded in);
    ``keypoint`` maps an image-pixel keypoint (kx, ky, 1) to crop coordinates (the frame of the un-augmented
    ``scale_box``: the crop's left edge at 0, its right edge at in_w)."""
    bboxes, origins, params = (np.asarray(a, dtype=np.float64) for a in (bboxes, origins, params))
    in_w, in_h = float(input_size[0]), float(input_size[1])
    bw, bh = bboxes[:, 2], bboxes[:, 3]
    f = 1.0 - 2.0 * params[:, 0]
    s, theta = params[:, 1], params[:, 2]
    cx = bboxes[:, 0] + bw / 2 + params[:, 3] * bw
    cy = bboxes[:, 1] + bh / 2 + params[:, 4] * bh
    co, si = np.cos(theta), np.sin(theta)
    gx, gy = f * bw * s / in_w, bh * s / in_h                 # source pixels per output pixel along the box's axes
    pixel = np.empty((len(bboxes), 2, 3))
    pixel[:, 0, 0], pixel[:, 0, 1] = co * gx, -si * gy
    pixel[:, 1, 0], pixel[:, 1, 1] = si * gx, co * gy
    hu, hv = 0.5 - in_w / 2, 0.5 - in_h / 2
    pixel[:, 0, 2] = cx - origins[:, 0] - 0.5 + pixel[:, 0, 0] * hu + pixel[:, 0, 1] * hv
    pixel[:, 1, 2] = cy - origins[:, 1] - 0.5 + pixel[:, 1, 0] * hu + pixel[:, 1, 1] * hv
    keypoint = np.empty((len(bboxes), 2, 3))
    keypoint[:, 0, 0], keypoint[:, 0, 1] = co / gx, si / gx
    keypoint[:, 1, 0], keypoint[:, 1, 1] = -si / gy, co / gy
    keypoint[:, 0, 2] = in_w / 2 - keypoint[:, 0, 0] * cx - keypoint[:, 0, 1] * cy
    keypoint[:, 1, 2] = in_h / 2 - keypoint[:, 1, 0] * cx - keypoint[:, 1, 1] * cy
    return pixel, keypoint


class _RawBatch(list):
    """The samples of a batch that a DataLoader worker hands to the main process uncollated."""


class _DeviceLoader(DataLoader):
    """A DataLoader calls ``collate_fn`` inside its workers when it has any; ``YOLOPoseDataset.collate`` passes the
    samples through there, and this iterator finishes the batch in the main process, where the GPU is."""

    def __iter__(self):
        for batch in super().__iter__():
            yield self.dataset._collate_device(batch) if isinstance(batch, _RawBatch) else batch


class YOLOPoseDataset(Dataset):
    """Reference dataset.py:93-135 with the per-sample pixel and target work moved into ``collate`` (module
    docstring).  ``codec`` is a ``Codec`` whose ``probmap`` gives input_size [w, h], heatmap_size [W, H] and sigmas."""

    def __init__(self, root: Path, split: str, codec, target_single_class: int | None = None,
                 augment: Augment | None = None):
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"YOLOPoseDataset: augment must be an Augment or None, not {type(augment).__name__}")
        self.root = root
        self.split = split
        self.codec = codec
        self.target_single_class = target_single_class
        self.augment = augment
        self.epoch = 0
        self.annotations = parse_annotations(Path(root) / split, target_single_class)
        self._staging = PinnedStaging()
        self._perm = None            # (K, device, host int32 [K], device int32 [K]) of the flip permutation

    def __getstate__(self):          # workers started by spawn get a copy: without the pinned buffers and their events
        state = dict(self.__dict__)
        state["_staging"] = PinnedStaging()
        state["_perm"] = None
        return state

    def set_epoch(self, epoch: int):
        """The epoch that keys the augmentation parameters.  Call it before iterating a loader: its workers take the
        value with their copy of the dataset when the iteration starts."""
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.annotations)

    def __getitem__(self, idx):
        """CPU only.  Without ``augment``: ``plain_item(idx)``.  With it: (region, keypoints, bbox, origin, params),
        where params float64 (7,) is ``augment.draw(epoch, idx)``, region the uint8 (h, w, 3) pixels of ``image.crop``
        of ``augment_region(bbox, params)`` (zero outside the frame) and origin int64 (2,) that rectangle's corner.
        With ``augment.half_body_prob`` above 0, bbox is ``augment.half_body_box(epoch, idx, keypoints, bbox)`` here and
        in everything after it.  With any of blur, median blur and erasing switched on, a sixth entry follows: the
        int32 (24,) record ``augment.draw_post(epoch, idx, input size)``."""
        if getattr(self, "augment", None) is None:
            return self.plain_item(idx)
        ann = self.annotations[idx]
        bbox = np.asarray(ann["bbox"], dtype=np.float64)
        keypoints = np.array(ann["keypoints"], dtype=np.float32).reshape(-1, 3)
        if self.augment.half_body_prob > 0:
            bbox = self.augment.half_body_box(self.epoch, idx, keypoints, bbox)
        params = self.augment.draw(self.epoch, idx)
        x0, y0, x1, y1 = augment_region(bbox, params)
        with PIL.Image.open(ann["image_path"]) as im:
            region = np.asarray(im.convert("RGB").crop((x0, y0, x1, y1)), dtype=np.uint8)
        item = (np.ascontiguousarray(region), keypoints, bbox, np.array([x0, y0], dtype=np.int64), params)
        if self.augment.post:
            item += (self.augment.draw_post(self.epoch, idx, self._input_size()),)
        return item

    def plain_item(self, idx):
        """CPU only.  Returns (region, keypoints, bbox): the uint8 (h, w, 3) pixels of ``image.crop`` of the rounded
        box (all that Pillow's resize reads; zero outside the frame), the keypoints float32 (K, 3) in image pixels
        and the un-rounded bbox float64 (4,)."""
        ann = self.annotations[idx]
        bbox = np.asarray(ann["bbox"], dtype=np.float64)
        x0, y0, x1, y1 = (int(v) for v in frontend.round_boxes([bbox])[0])
        with PIL.Image.open(ann["image_path"]) as im:
            region = np.asarray(im.convert("RGB").crop((x0, y0, x1, y1)), dtype=np.uint8)
        return np.ascontiguousarray(region), np.array(ann["keypoints"], dtype=np.float32).reshape(-1, 3), bbox

    # ---- batch assembly on the device --------------------------------------------------------------------------
    def collate(self, samples):
        """``collate_fn`` of the loader: samples of ``__getitem__`` -> (img (B, 3, h, w) f32 in [0, 1], gt dict of
        heatmaps (B, K, H, W) f32, in_image / keypoints_visible (B, 1, K) bool, keypoints_visibility (B, 1, K) f32) on
        the current device.  Inside a DataLoader worker it only passes the samples on (see ``loader``)."""
        if get_worker_info() is not None:
            return _RawBatch(samples)
        return self._collate_device(samples)

    @staticmethod
    def pack_layout(shapes):
        """Byte offsets of (h, w) regions packed back to back, each at a multiple of 16 with tight rows (stride 3 w),
        and the size of the buffer: the last region's end plus the padding the kernel's dword loads want."""
        offs, end = [], 0
        for h, w in shapes:
            off = -(-end // _REGION_ALIGN) * _REGION_ALIGN
            offs.append(off)
            end = off + 3 * int(h) * int(w)
        total = -(-(end + frontend.SRC_PAD) // _REGION_ALIGN) * _REGION_ALIGN
        return offs, total

    def _collate_device(self, samples):
        if len(samples) and len(samples[0]) == 5:
            return self._launch_augmented(*self._upload_augmented(samples))
        if len(samples) and len(samples[0]) == 6:
            return self._launch_post(*self._upload_post(samples))
        return self._launch(*self._upload(samples))

    def _pack(self, samples, fields):
        """What both uploads start with: check the samples (tuples of ``fields`` entries), pack the regions back to
        back and issue copy 1, the pixels.  Returns (B, K, shapes, offs, total, d_src)."""
        _lib.require_device()
        B = len(samples)
        if B == 0:
            raise ValueError("YOLOPoseDataset.collate: an empty batch")
        K = int(samples[0][1].shape[0])
        for s in samples:
            region, kps = s[0], s[1]
            if len(s) != fields:
                raise ValueError("YOLOPoseDataset.collate: augmented and un-augmented samples in one batch")
            if region.dtype != np.uint8 or region.ndim != 3 or region.shape[2] != 3 or region.size == 0:
                raise ValueError(f"YOLOPoseDataset.collate: a region of shape {region.shape}, dtype {region.dtype}")
            if kps.shape != (K, 3):
                raise ValueError(f"YOLOPoseDataset.collate: keypoints of shapes {(K, 3)} and {kps.shape} in one batch")
        shapes = [s[0].shape[:2] for s in samples]
        offs, total = self.pack_layout(shapes)
        slot = self._staging.take(total)
        host = slot[0].numpy()
        for s, off in zip(samples, offs):
            host[off:off + s[0].size] = s[0].reshape(-1)
        d_src = torch.empty(total, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        d_src.copy_(slot[0][:total], non_blocking=True)
        slot[1].record()
        return B, K, shapes, offs, total, d_src

    def _input_size(self):
        pm = self.codec.probmap
        return int(pm.input_size[0]), int(pm.input_size[1])

    def _upload(self, samples):
        """Host half of ``collate``: pack, build the plan, issue the two copies.  Returns what ``_launch`` takes."""
        B, K, shapes, offs, total, d_src = self._pack(samples, 3)
        in_w, in_h = self._input_size()
        # copy 2: the plan, then the boxes (f64) and the raw keypoints (f32); built while copy 1 runs
        boxes = np.array([[0, 0, w, h] for h, w in shapes], dtype=np.int32)
        sources = np.array([[off, w, h, 3 * w] for off, (h, w) in zip(offs, shapes)], dtype=np.int64)
        plan_bytes = frontend.multi_plan_bytes(boxes, (in_w, in_h))
        box_off = -(-plan_bytes // 8) * 8
        kp_off = box_off + 32 * B
        meta_bytes = kp_off + 12 * B * K
        slot = self._staging.take(meta_bytes)
        n_blocks, lds = frontend.multi_plan_build(boxes, sources, total, (in_w, in_h), slot[0].data_ptr())
        host = slot[0].numpy()
        host[box_off:kp_off].view(np.float64).reshape(B, 4)[:] = [s[2] for s in samples]
        host[kp_off:meta_bytes].view(np.float32).reshape(B, K, 3)[:] = [s[1] for s in samples]
        d_meta = torch.empty(meta_bytes, dtype=torch.uint8, device=d_src.device)
        d_meta.copy_(slot[0][:meta_bytes], non_blocking=True)
        slot[1].record()
        return d_src, d_meta, B, K, n_blocks, lds, box_off, kp_off

    def _ground_truth(self, img, B, K, entry, *args):
        """What both launches end with: the keypoint kernel ``entry(*args, B, K, input size, scale, outputs)``, then
        the maps.  Returns collate's (img, gt dict)."""
        pm = self.codec.probmap
        dev = img.device
        f32 = torch.empty((6, B, K), dtype=torch.float32, device=dev)    # crop xy (2), heatmap xy (2), encode vis, visibility
        flags = torch.empty((2, B, 1, K), dtype=torch.bool, device=dev)  # in_image, keypoints_visible
        kp_crop, kp_hm = f32[0:2].view(B, K, 2), f32[2:4].view(B, K, 2)
        sx, sy = (float(v) for v in np.asarray(pm.scale_factor, dtype=np.float32))
        with torch.cuda.device(dev):
            _lib.launch(entry, *args, B, K, *self._input_size(), sx, sy, kp_crop, kp_hm, f32[4], flags[0], flags[1],
                        f32[5])
        heat, _ = pm.encode_device_tensors(kp_hm, f32[4])
        return img, dict(heatmaps=heat, in_image=flags[0], keypoints_visible=flags[1],
                         keypoints_visibility=f32[5].view(B, 1, K))

    def _launch(self, d_src, d_meta, B, K, n_blocks, lds, box_off, kp_off):
        """Device half of ``collate``: the three launches on the uploaded buffers (crops; keypoints and flags; maps)."""
        img = frontend.crop_resize_multi(d_src, d_meta, B, n_blocks, lds, self._input_size())
        meta = d_meta.data_ptr()
        return self._ground_truth(img, B, K, "pp_dataset_ground_truth", meta + kp_off, meta + box_off)

    # ---- the augmented batch: the same two copies, then warp, keypoints, maps ---------------------------------------
    def _permutation(self, K, dev):
        """The flip permutation for K keypoints, validated and uploaded once per dataset."""
        if self._perm is None or self._perm[:2] != (K, dev):
            perm = self.augment.permutation(K)
            self._perm = (K, dev, perm, torch.from_numpy(perm).to(dev))
        return self._perm[2], self._perm[3]

    def _upload_augmented(self, samples, fields=5):
        """Host half of the augmented ``collate``: pack the regions (copy 1); build the source records, the two
        matrices per sample in float64 and the keypoints into the meta buffer (copy 2); have the library check them.
        With ``fields=6`` (``_upload_post``) the samples' ``draw_post`` records follow the keypoints in copy 2."""
        _lib.require_device()
        if self.augment is None:
            raise ValueError("YOLOPoseDataset.collate: augmented samples, but the dataset has augment=None")
        B, K, shapes, offs, total, d_src = self._pack(samples, fields)
        perm, d_perm = self._permutation(K, d_src.device)
        # copy 2: [B x 4 i64 source records][B x 8 f64 pixel matrix, c, b][B x 8 f32 keypoint matrix, flip, 0][keypoints]
        params = np.stack([s[4] for s in samples])
        pixel, keypoint = augment_matrices(np.stack([s[2] for s in samples]), np.stack([s[3] for s in samples]),
                                           params, self._input_size())
        warp_off, aff_off, kp_off = 32 * B, 96 * B, 128 * B
        post_off = kp_off + 12 * B * K
        meta_bytes = post_off + (4 * _lib.PP_AUGMENT_POST_WORDS * B if fields == 6 else 0)
        slot = self._staging.take(meta_bytes)
        host = slot[0].numpy()
        host[:warp_off].view(np.int64).reshape(B, 4)[:] = [[off, w, h, 3 * w] for off, (h, w) in zip(offs, shapes)]
        warp = host[warp_off:aff_off].view(np.float64).reshape(B, 8)
        warp[:, :6], warp[:, 6], warp[:, 7] = pixel.reshape(B, 6), params[:, 5], params[:, 6]
        aff = host[aff_off:kp_off].view(np.float32).reshape(B, 8)
        aff[:, :6], aff[:, 6], aff[:, 7] = keypoint.reshape(B, 6), params[:, 0], 0.0
        host[kp_off:post_off].view(np.float32).reshape(B, K, 3)[:] = [s[1] for s in samples]
        base = slot[0].data_ptr()
        _lib.call("pp_augment_check", B, base, total, base + warp_off, base + aff_off, K, perm)
        if fields == 6:
            for s in samples:
                if s[5].shape != (_lib.PP_AUGMENT_POST_WORDS,) or s[5].dtype != np.int32:
                    raise ValueError(f"YOLOPoseDataset.collate: a post record of shape {s[5].shape}, dtype {s[5].dtype}")
            host[post_off:meta_bytes].view(np.int32).reshape(B, _lib.PP_AUGMENT_POST_WORDS)[:] = [s[5] for s in samples]
            _lib.call("pp_augment_post_check", B, base + post_off, *self._input_size(), self._post_filters())
        d_meta = torch.empty(meta_bytes, dtype=torch.uint8, device=d_src.device)
        d_meta.copy_(slot[0][:meta_bytes], non_blocking=True)
        slot[1].record()
        return d_src, d_meta, d_perm, B, K

    def _launch_augmented(self, d_src, d_meta, d_perm, B, K):
        """Device half of the augmented ``collate``: warp, keypoints and flags, maps."""
        in_w, in_h = self._input_size()
        meta = d_meta.data_ptr()
        img = torch.empty((B, 3, in_h, in_w), dtype=torch.float32, device=d_src.device)
        with torch.cuda.device(d_src.device):
            _lib.launch("pp_augment_warp", d_src, meta, meta + 32 * B, B, in_w, in_h, img)
        return self._ground_truth(img, B, K, "pp_dataset_ground_truth_affine", meta + 128 * B, meta + 96 * B, d_perm)

    # ---- the augmented batch with blur / erasing: the records ride on copy 2, one launch more behind the warp ---------
    def _post_filters(self):
        """``pp_augment_post``'s mode: 1 when a sample can carry a filter, else 0 (holes only, in place)."""
        return 1 if self.augment.blur_prob > 0 or self.augment.median_prob > 0 else 0

    def _upload_post(self, samples):
        """Host half of ``collate`` for 6-tuples: ``_upload_augmented`` with the records appended to copy 2, checked on
        the host (``pp_augment_post_check``) before the copy is issued."""
        return self._upload_augmented(samples, fields=6)

    def _launch_post(self, d_src, d_meta, d_perm, B, K):
        """Device half of ``collate`` for 6-tuples: warp, blur / holes, keypoints and flags, maps.  Holes alone are
        written in place into the warp's output; a filter writes a second tensor, which becomes img."""
        in_w, in_h = self._input_size()
        meta = d_meta.data_ptr()
        filters = self._post_filters()
        img = torch.empty((B, 3, in_h, in_w), dtype=torch.float32, device=d_src.device)
        out = torch.empty_like(img) if filters else img
        with torch.cuda.device(d_src.device):
            _lib.launch("pp_augment_warp", d_src, meta, meta + 32 * B, B, in_w, in_h, img)
            _lib.launch("pp_augment_post", img, meta + 128 * B + 12 * B * K, B, in_w, in_h, filters, out)
        return self._ground_truth(out, B, K, "pp_dataset_ground_truth_affine", meta + 128 * B, meta + 96 * B, d_perm)

    def loader(self, batch_size, shuffle=False, num_workers=0, **kw):
        """A DataLoader over this dataset whose batches are ``collate``'s.  The workers do file reading, decoding and
        the integer crop; the batch is assembled in the main process."""
        if num_workers > MAX_WORKERS:
            raise ValueError(f"YOLOPoseDataset.loader: num_workers={num_workers}; at most {MAX_WORKERS} (the workers "
                             "inherit the open GPU, and 16 processes in all may hold it)")
        if "collate_fn" in kw:
            raise TypeError("YOLOPoseDataset.loader sets collate_fn itself")
        if getattr(self, "augment", None) is not None and kw.get("persistent_workers"):
            raise ValueError("YOLOPoseDataset.loader: persistent workers keep the epoch they were started with; with "
                             "augment set, start the workers per epoch")
        return _DeviceLoader(self, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                             collate_fn=self.collate, **kw)

    def reference_item(self, idx):
        """The reference's ``__getitem__`` value (dataset.py:130-135): img (3, h, w) and the gt dict with heatmaps
        (K, H, W) and the three (1, K) arrays, as device tensors, through the batch path with B = 1.  Always the
        un-augmented item, whatever ``augment`` is."""
        img, gt = self._collate_device([self.plain_item(idx)])
        return img[0], {k: v[0] for k, v in gt.items()}
