"""Front end of the path: person boxes of an RGB frame -> network input crops on the GPU.

Counterpart of the reference's ``dataset.scale_box`` (dataset.py:71-90: ``image.crop(box)`` then
``.resize(image_size, PIL.Image.LANCZOS)`` and the keypoint rescale) followed by the
``v2.ToImage(); v2.ToDtype(torch.float32, scale=True)`` transform (dataset.py:107-112,
inference.py:74-82).  The pixel arithmetic is Pillow's; ``crop_resize`` reproduces it bit for bit
(csrc/pp_frontend.hip): the per-box coefficient tables are built on the host by the library with
Pillow's own double-precision expressions, the two resampling passes run in one HIP kernel.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib


def round_boxes(boxes_xywh) -> np.ndarray:
    """[x, y, w, h] boxes (dataset.py:74-80 passes (x, y, x+w, y+h) to Image.crop) -> the integer
    (x0, y0, x1, y1) Pillow crops: ``map(int, map(round, box))`` (Image.crop), i.e. Python's
    round-half-to-even on the float corner coordinates."""
    out = np.empty((len(boxes_xywh), 4), dtype=np.int32)
    for i, b in enumerate(boxes_xywh):
        x, y, w, h = (float(v) for v in b)
        out[i] = [int(round(x)), int(round(y)), int(round(x + w)), int(round(y + h))]
    return out


class FrontendPlan:
    """Host-built tables for one set of boxes and one output size (reusable across frames)."""

    def __init__(self, boxes_xyxy: np.ndarray, input_size: Sequence[int], device):
        self.boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
        self.n = int(self.boxes.shape[0])
        self.out_w, self.out_h = int(input_size[0]), int(input_size[1])
        nbytes = _lib.call("pp_frontend_plan_bytes", self.n, self.boxes, self.out_w, self.out_h)
        host = np.empty((max(int(nbytes), 4) // 4,), dtype=np.int32)
        nb, lds = C.c_int(0), C.c_longlong(0)
        _lib.call("pp_frontend_plan_build", self.n, self.boxes, self.out_w, self.out_h, host, C.byref(nb), C.byref(lds))
        self.host = host
        self.n_blocks, self.lds_bytes = int(nb.value), int(lds.value)
        self.dev = torch.from_numpy(host).to(device) if device is not None else None


def crop_resize(image: torch.Tensor, boxes_xywh, input_size: Sequence[int], plan: FrontendPlan = None) -> torch.Tensor:
    """image: (H, W, 3) uint8 RGB on the GPU; boxes [x, y, w, h] in pixels (floats allowed);
    input_size = [w, h].  Returns (n, 3, h, w) float32 in [0, 1] on the GPU: for every box exactly
    ``ToDtype(float32, scale=True)(ToImage()(image.crop(box).resize(input_size, LANCZOS)))``."""
    _lib.require_device(image)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise TypeError("image must be a (H, W, 3) uint8 tensor (RGB, channels last)")
    if image.stride(2) != 1 or image.stride(1) != 3:
        image = image.contiguous()
    if plan is None:
        plan = FrontendPlan(round_boxes(boxes_xywh), input_size, image.device)
    out = torch.empty((plan.n, 3, plan.out_h, plan.out_w), dtype=torch.float32, device=image.device)
    if plan.n == 0:
        return out
    with torch.cuda.device(image.device):
        _lib.launch("pp_frontend_crop_resize", image, int(image.shape[1]), int(image.shape[0]), int(image.stride(0)),
                    plan.dev, plan.n, plan.n_blocks, plan.lds_bytes, plan.out_w, plan.out_h, out)
    return out


SRC_ALIGN, SRC_PAD = 4, 4     # PP_FRONTEND_SRC_ALIGN / PP_FRONTEND_SRC_PAD of include/probpose_hip.h


def multi_plan_bytes(boxes_xyxy: np.ndarray, input_size: Sequence[int]) -> int:
    """Bytes of the multi-source plan for these integer boxes (host only)."""
    boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
    return int(_lib.call("pp_frontend_multi_plan_bytes", int(boxes.shape[0]), boxes, int(input_size[0]),
                         int(input_size[1])))


def multi_plan_build(boxes_xyxy: np.ndarray, sources: np.ndarray, src_bytes: int, input_size: Sequence[int],
                     plan_ptr: int) -> Tuple[int, int]:
    """Build the multi-source plan (host only, no GPU) into the ``multi_plan_bytes`` bytes of host memory at
    ``plan_ptr``.  boxes_xyxy [n, 4] int32, each in the pixel frame of its own source; sources [n, 4] int64 =
    (byte offset into the packed source buffer, width, height, row stride in bytes); src_bytes: that buffer's size.
    Offsets must be multiples of SRC_ALIGN and every region must end SRC_PAD bytes before the end of the buffer.
    Returns (workgroups of the launch, LDS bytes per workgroup)."""
    boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
    src = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1, 4)
    if src.shape[0] != boxes.shape[0]:
        raise ValueError(f"{boxes.shape[0]} boxes but {src.shape[0]} source records")
    nb, lds = C.c_int(0), C.c_longlong(0)
    _lib.call("pp_frontend_multi_plan_build", int(boxes.shape[0]), boxes, src, int(src_bytes), int(input_size[0]),
              int(input_size[1]), plan_ptr, C.byref(nb), C.byref(lds))
    return int(nb.value), int(lds.value)


def crop_resize_multi(src: torch.Tensor, plan_dev: torch.Tensor, n: int, n_blocks: int, lds_bytes: int,
                      input_size: Sequence[int]) -> torch.Tensor:
    """One launch over n boxes that each read their own region of the packed uint8 source buffer ``src`` (on the GPU),
    as the device copy ``plan_dev`` of a ``multi_plan_build`` plan (built for a buffer of at most ``src.numel()``
    bytes) describes.  Returns (n, 3, h, w) float32 in [0, 1]; per box the bits of ``crop_resize``."""
    _lib.require_device(src)
    _lib.require_device(plan_dev)
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise TypeError("src must be a contiguous uint8 tensor")
    out_w, out_h = int(input_size[0]), int(input_size[1])
    out = torch.empty((n, 3, out_h, out_w), dtype=torch.float32, device=src.device)
    if n == 0:
        return out
    with torch.cuda.device(src.device):
        _lib.launch("pp_frontend_crop_resize_multi", src, plan_dev, n, n_blocks, lds_bytes, out_w, out_h, out)
    return out


def scale_box(image: torch.Tensor, bbox, image_size: Tuple[int, int], kps: np.ndarray):
    """Reference dataset.py:71-90 for one box: returns (crop (3, h, w) f32 in [0,1] on the GPU, kps)
    with the keypoints moved into the crop's pixel frame (kps is modified in place, like the
    reference; the keypoint rescale uses the UN-rounded box, dataset.py:87-89)."""
    crop = crop_resize(image, [bbox], image_size)[0]
    kps[:, 0] = (kps[:, 0] - bbox[0]) / bbox[2] * image_size[0]
    kps[:, 1] = (kps[:, 1] - bbox[1]) / bbox[3] * image_size[1]
    return crop, kps
