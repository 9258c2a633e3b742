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
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import PIL.Image
import torch
from torch.utils.data import DataLoader, Dataset, get_worker_info

from . import _lib, frontend

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

    def __init__(self, root: Path, split: str, codec, target_single_class: int | None = None):
        self.root = root
        self.split = split
        self.codec = codec
        self.target_single_class = target_single_class
        self.annotations = parse_annotations(Path(root) / split, target_single_class)
        self._staging = []           # [(pinned host buffer, event after its last copy)]

    def __getstate__(self):          # workers started by spawn get a copy: without the pinned buffers and their events
        state = dict(self.__dict__)
        state["_staging"] = []
        return state

    def __len__(self):
        return len(self.annotations)

    def __getitem__(self, idx):
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
    def _staging_buffer(self, nbytes: int):
        """A pinned host buffer that no earlier asynchronous copy can still be reading: one whose event has completed,
        or a new one.  Never waits."""
        for slot in self._staging:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._staging.append(slot)
        return slot

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
        return self._launch(*self._upload(samples))

    def _upload(self, samples):
        """Host half of ``collate``: pack, build the plan, issue the two copies.  Returns what ``_launch`` takes."""
        _lib.require_device()
        B = len(samples)
        if B == 0:
            raise ValueError("YOLOPoseDataset.collate: an empty batch")
        pm = self.codec.probmap
        in_w, in_h = int(pm.input_size[0]), int(pm.input_size[1])
        K = int(samples[0][1].shape[0])
        for region, kps, _ in samples:
            if region.dtype != np.uint8 or region.ndim != 3 or region.shape[2] != 3 or region.size == 0:
                raise ValueError(f"YOLOPoseDataset.collate: a region of shape {region.shape}, dtype {region.dtype}")
            if kps.shape != (K, 3):
                raise ValueError(f"YOLOPoseDataset.collate: keypoints of shapes {(K, 3)} and {kps.shape} in one batch")
        dev = torch.device("cuda", torch.cuda.current_device())
        shapes = [s[0].shape[:2] for s in samples]
        offs, total = self.pack_layout(shapes)
        # copy 1: the pixels
        slot = self._staging_buffer(total)
        host = slot[0].numpy()
        for (region, _, _), off in zip(samples, offs):
            host[off:off + region.size] = region.reshape(-1)
        d_src = torch.empty(total, dtype=torch.uint8, device=dev)
        d_src.copy_(slot[0][:total], non_blocking=True)
        slot[1].record()
        # copy 2: the plan, then the boxes (f64) and the raw keypoints (f32); built while copy 1 runs
        boxes = np.array([[0, 0, w, h] for h, w in shapes], dtype=np.int32)
        sources = np.array([[off, w, h, 3 * w] for off, (h, w) in zip(offs, shapes)], dtype=np.int64)
        plan_bytes = frontend.multi_plan_bytes(boxes, (in_w, in_h))
        box_off = -(-plan_bytes // 8) * 8
        kp_off = box_off + 32 * B
        meta_bytes = kp_off + 12 * B * K
        slot = self._staging_buffer(meta_bytes)
        n_blocks, lds = frontend.multi_plan_build(boxes, sources, total, (in_w, in_h), slot[0].data_ptr())
        host = slot[0].numpy()
        host[box_off:kp_off].view(np.float64).reshape(B, 4)[:] = [s[2] for s in samples]
        host[kp_off:meta_bytes].view(np.float32).reshape(B, K, 3)[:] = [s[1] for s in samples]
        d_meta = torch.empty(meta_bytes, dtype=torch.uint8, device=dev)
        d_meta.copy_(slot[0][:meta_bytes], non_blocking=True)
        slot[1].record()
        return d_src, d_meta, B, K, n_blocks, lds, box_off, kp_off

    def _launch(self, d_src, d_meta, B, K, n_blocks, lds, box_off, kp_off):
        """Device half of ``collate``: the three launches on the uploaded buffers."""
        pm = self.codec.probmap
        in_w, in_h = int(pm.input_size[0]), int(pm.input_size[1])
        dev = d_src.device
        # launch 1: crops
        img = frontend.crop_resize_multi(d_src, d_meta, B, n_blocks, lds, (in_w, in_h))
        # launch 2: keypoints and flags
        f32 = torch.empty((6, B, K), dtype=torch.float32, device=dev)    # crop xy (2), heatmap xy (2), encode vis, visibility
        flags = torch.empty((2, B, 1, K), dtype=torch.bool, device=dev)  # in_image, keypoints_visible
        kp_crop, kp_hm = f32[0:2].view(B, K, 2), f32[2:4].view(B, K, 2)
        sx, sy = (float(v) for v in np.asarray(pm.scale_factor, dtype=np.float32))
        with torch.cuda.device(dev):
            rc = _lib.lib().pp_dataset_ground_truth(d_meta.data_ptr() + kp_off, d_meta.data_ptr() + box_off, B, K,
                                                    in_w, in_h, sx, sy, _lib.ptr(kp_crop), _lib.ptr(kp_hm),
                                                    _lib.ptr(f32[4]), _lib.ptr(flags[0]), _lib.ptr(flags[1]),
                                                    _lib.ptr(f32[5]), _lib.stream_ptr())
        _lib.check(rc, "pp_dataset_ground_truth")
        # launch 3: the maps
        heat, _ = pm.encode_device_tensors(kp_hm, f32[4])
        return img, dict(heatmaps=heat, in_image=flags[0], keypoints_visible=flags[1],
                         keypoints_visibility=f32[5].view(B, 1, K))

    def loader(self, batch_size, shuffle=False, num_workers=0, **kw):
        """A DataLoader over this dataset whose batches are ``collate``'s.  The workers do file reading, decoding and
        the integer crop; the batch is assembled in the main process."""
        if num_workers > MAX_WORKERS:
            raise ValueError(f"YOLOPoseDataset.loader: num_workers={num_workers}; at most {MAX_WORKERS} (the workers "
                             "inherit the open GPU, and 16 processes in all may hold it)")
        if "collate_fn" in kw:
            raise TypeError("YOLOPoseDataset.loader sets collate_fn itself")
        return _DeviceLoader(self, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                             collate_fn=self.collate, **kw)

    def reference_item(self, idx):
        """The reference's ``__getitem__`` value (dataset.py:130-135): img (3, h, w) and the gt dict with heatmaps
        (K, H, W) and the three (1, K) arrays, as device tensors, through the batch path with B = 1."""
        img, gt = self._collate_device([self[idx]])
        return img[0], {k: v[0] for k, v in gt.items()}
