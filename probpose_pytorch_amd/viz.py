"""Counterpart of the reference's ``probpose/viz.py``, and of the drawing its ``inference.py`` does, on the GPU.

Everything upstream of a picture already lives on the device (crops, maps, decoded keypoints, NMS-kept poses), so the
pictures are made there too, by the two launches of csrc/pp_viz.hip:

  pp_viz_render     overlay_heatmap_on_image, draw_keypoints and render: one pass over the image bytes
  pp_viz_colorize   colorize: heat maps as RGBA pictures, one workgroup a map

Every function takes numpy arrays (numpy out: one upload, one download) or device tensors (device out, no host
synchronisation; ``out=`` names a preallocated result, which graph capture needs).  There is no CPU fallback: without
a GPU the calls raise ``_lib.HipExtensionError``; shape, dtype and range errors raise ValueError / TypeError before
that.  The style arguments (colormap, colors, skeleton, ...) are host values; their small device tables are cached by
content.  ``image_index`` may be a host array (checked against the batch here) or a device tensor (not read back: an
instance whose index is outside the batch is not drawn).

Rules (restated in tests/viz_reference.py, the gauge this module is tested against, and in include/probpose_hip.h):

* value of map k at an image pixel: the map's own element when the map has the image's size (the reference's case),
  else bilinear under the codecs' ``(input - 1) / (heatmap - 1)`` convention, in float64, rounded to float32:
  ``u = px * (w - 1) / (W - 1)`` (0 when W == 1), ``x0 = min(floor(u), w - 1)``, ``x1 = min(x0 + 1, w - 1)``,
  ``fx = u - x0``, the same in y, ``(a00 (1 - fx) + a01 fx)(1 - fy) + (a10 (1 - fx) + a11 fx) fy``.  A non-finite
  neighbour contaminates the result even with weight 0 (inf * 0 = NaN), as the formula does;
* colour: matplotlib's ``Colormap.__call__`` on a float32 array: ``xa = v * 256`` in float32, NaN -> (0, 0, 0),
  ``xa < 0`` -> row 0, ``xa >= 256`` -> row 255, else row ``trunc(xa)`` of the colormap's float64 [256, 3] table;
* overlay: a value below float32(0.01) adds nothing; the colours are summed over k ascending in float64 from 0.0,
  multiplied by 255.0, saturated at 255, truncated, and added to the image byte with saturation at 255.  The reference
  wraps in both places (``.astype(np.uint8)`` of a sum above 255, and ``image + heat`` in uint8); this does not;
* a float32 [B, 3, H, W] image in [0, 1] becomes bytes as ``trunc(min(max(v * 255 + 0.5, 0), 255))`` in float32, NaN 0;
* colorize: ``trunc(colour * 255.0)``, alpha 255, (0, 0, 0, 0) for NaN; ``normalize`` first divides each map by its own
  maximum in float32 (numpy's ``hm / hm.max()``: one NaN makes the map NaN, a maximum of 0 gives 0 / 0 = NaN);
* keypoints (reference inference.py:115-125): drawn unless ``prob < threshold`` (a NaN probability is drawn), at
  ``int(x), int(y)`` (truncation toward zero), only if that centre is inside the image; non-finite coordinates and
  magnitudes of 2^31 and beyond are skipped; the disc is ``dx^2 + dy^2 <= r^2 + r`` (what PIL's ellipse paints for
  r = 2, 3, 5), clipped to the image.  The reference's text labels are not drawn: that is left to the host;
* limb (i, j) of an instance: drawn if both keypoints are and their centres a, b differ; with d = b - a, e = p - a,
  t = e.d the pixel p is painted iff 4 dist^2 <= line_width^2, dist^2 = |e|^2 (t <= 0), |p - b|^2 (t >= d.d), else
  cross(e, d)^2 / d.d, evaluated in exact integers;
* painter's order, per pixel the last primitive that covers it: all limbs (instance ascending, then skeleton order),
  then all discs (instance ascending, then keypoint ascending).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib, ops
from ._buffers import CaptureCache, room as _room, upload

COLORMAPS = ("jet", "inferno")
MAX_SIDE = _lib.PP_VIZ_MAX_SIDE
COCO17_SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9),
                   (8, 10), (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))

_TABLE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "colormaps.json")
_tables = {}
_device_tables = CaptureCache(64)      # (device, content) -> device tensor: the colour tables and the style tables


def colormap_table(name: str) -> np.ndarray:
    """matplotlib's float64 [256, 3] table of ``name``, from data/colormaps.json (minted by data/make_colormaps.py)."""
    if name not in COLORMAPS:
        raise ValueError(f"colormap: {name!r} is not one of {COLORMAPS}")
    if not _tables:
        with open(_TABLE_FILE) as f:                 # text: repr() of a float64 reads back as the same float64
            z = json.load(f)
        _tables.update({k: np.ascontiguousarray(z[k], dtype=np.float64) for k in COLORMAPS})
    return _tables[name]


def _device_table(table: np.ndarray, device) -> torch.Tensor:
    return _device_tables.get((str(device), table.dtype.str, table.tobytes()),
                              lambda: torch.from_numpy(table).to(device))


def _dtype(a) -> str:
    return str(a.dtype).replace("torch.", "") if isinstance(a, torch.Tensor) else a.dtype.name


def _placement(named, out):
    """(named with array-likes as numpy arrays, on_device).  Device tensors or host arrays, never both."""
    named = [(n, a if isinstance(a, torch.Tensor) else np.asarray(a)) for n, a in named]
    dev = [isinstance(a, torch.Tensor) and a.is_cuda for _, a in named]
    names = " / ".join(n for n, _ in named)
    if any(dev) and not all(dev):
        raise ValueError(f"{names}: either all device tensors or all host arrays")
    if not any(dev):
        for n, a in named:
            if isinstance(a, torch.Tensor):
                raise TypeError(f"{n}: a host tensor; pass a numpy array or a device tensor")
        if out is not None:
            raise ValueError("out: only with device tensors (numpy in gives numpy out)")
    return named, all(dev)


def _check_out(out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
        raise ValueError(f"out: expected a tensor on {device}")
    if out.dtype != torch.uint8:
        raise TypeError(f"out: expected uint8, got {out.dtype}")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"out: expected a contiguous {tuple(shape)} tensor, got {tuple(out.shape)}")
    return out


def _rgb_rows(value, rows: int, name: str) -> np.ndarray:
    """One RGB triple or [rows, 3] -> int64 [rows, 3] of bytes."""
    c = np.asarray(value)
    if c.dtype.kind not in "iu":
        raise TypeError(f"{name}: expected integers 0..255, got {c.dtype.name}")
    if c.shape == (3,):
        c = np.broadcast_to(c, (rows, 3))
    if c.shape != (rows, 3):
        raise ValueError(f"{name}: expected one RGB triple or [{rows}, 3], got {c.shape}")
    if c.size and (c.min() < 0 or c.max() > 255):
        raise ValueError(f"{name}: values outside 0..255")
    return c.astype(np.int64)


def _style_table(K, colors, skeleton, limb_colors) -> tuple:
    """(int32 table: K packed colours r | g << 8 | b << 16, then L limbs (i, j, colour); L)."""
    pack = lambda c: c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16               # noqa: E731
    kp = _rgb_rows(colors, K, "colors")
    if skeleton is None:
        if limb_colors is not None:
            raise ValueError("limb_colors: needs a skeleton")
        return pack(kp).astype(np.int32), 0
    sk = np.asarray(skeleton)
    if sk.size == 0:
        sk = sk.reshape(0, 2).astype(np.int64)
    if sk.dtype.kind not in "iu":
        raise TypeError(f"skeleton: expected pairs of keypoint indices, got {sk.dtype.name}")
    if sk.ndim != 2 or sk.shape[1] != 2:
        raise ValueError(f"skeleton: expected [L, 2], got {sk.shape}")
    if sk.size and (sk.min() < 0 or sk.max() >= K):
        raise ValueError(f"skeleton: a keypoint index outside 0..{K - 1}")
    sk = sk.astype(np.int64)
    L = sk.shape[0]
    lc = kp[sk[:, 0]] if limb_colors is None else _rgb_rows(limb_colors, L, "limb_colors")
    limbs = np.concatenate([sk, pack(lc)[:, None]], axis=1).reshape(-1)
    return np.concatenate([pack(kp), limbs]).astype(np.int32), L


def _int_in(value, lo: int, hi: int, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name}: expected an int, got {type(value).__name__}")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name}: {value} is outside {lo}..{hi}")
    return int(value)


def _instance_order(image_index, N: int, B: int):
    """Checks ``image_index``; returns ``make(device, keep)`` -> (inst int32 [N]: the instances ordered by image,
    stable; img_off int32 [B + 1]: where each image's instances start in inst), both on the device."""
    if image_index is None:
        if N != B:
            raise ValueError(f"image_index: {N} instances on {B} images need an image_index")
        return lambda device, keep: (torch.arange(N, dtype=torch.int32, device=device),
                                     torch.arange(B + 1, dtype=torch.int32, device=device))
    on_device = isinstance(image_index, torch.Tensor) and image_index.is_cuda
    idx = image_index if on_device else np.asarray(image_index)
    if tuple(idx.shape) != (N,):
        raise ValueError(f"image_index: expected [{N}], got {tuple(idx.shape)}")
    if on_device:
        if idx.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"image_index: expected int32 or int64, got {idx.dtype}")

        def make(device, keep):
            ordered, inst = torch.sort(idx.to(torch.int64), stable=True)
            off = torch.searchsorted(ordered, torch.arange(B + 1, dtype=torch.int64, device=device))
            return inst.to(torch.int32), off.to(torch.int32)
        return make
    if idx.dtype.kind not in "iu":
        raise TypeError(f"image_index: expected integers, got {idx.dtype.name}")
    if N and (idx.min() < 0 or idx.max() >= B):
        raise ValueError(f"image_index: an index outside 0..{B - 1}")
    inst = np.argsort(idx, kind="stable").astype(np.int32)
    off = np.searchsorted(idx[inst], np.arange(B + 1)).astype(np.int32)
    return lambda device, keep: (upload(inst, device, keep), upload(off, device, keep))


def render(image, heatmap=None, keypoints=None, probabilities=None, *, colormap: str = "jet",
           threshold: float = 0.9, radius: int = 5, colors=(255, 0, 0), skeleton=None, limb_colors=None,
           line_width: int = 2, image_index=None, out=None):
    """``draw_keypoints(overlay_heatmap_on_image(image, heatmap), keypoints, probabilities, ...)`` in one pass: each
    image byte is read once and written once.  With ``heatmap`` None nothing is overlaid, with ``keypoints`` None
    nothing is drawn.  Returns uint8 [B, H, W, 3] ([H, W, 3] for an unbatched image).  ``out`` may be the uint8 image
    itself (in place)."""
    if (keypoints is None) != (probabilities is None):
        raise ValueError("keypoints / probabilities: give both or neither")
    named = [("image", image)] + ([("heatmap", heatmap)] if heatmap is not None else []) \
        + ([("keypoints", keypoints), ("probabilities", probabilities)] if keypoints is not None else [])
    named, on_device = _placement(named, out)
    arrays = dict(named)
    image = arrays["image"]

    # ---- the image -------------------------------------------------------------------------------------------------
    dt, shape = _dtype(image), tuple(image.shape)
    batched = len(shape) == 4
    if dt == "uint8":
        if len(shape) not in (3, 4) or shape[-1] != 3:
            raise ValueError(f"image: expected uint8 [H, W, 3] or [B, H, W, 3], got {shape}")
        B, H, W = (shape[0] if batched else 1), shape[-3], shape[-2]
    elif dt == "float32":
        if len(shape) != 4 or shape[1] != 3:
            raise ValueError(f"image: a float32 image is [B, 3, H, W], got {shape}")
        B, H, W = shape[0], shape[2], shape[3]
    else:
        raise TypeError(f"image: expected uint8 (HWC) or float32 ([B, 3, H, W] in [0, 1]), got {dt}")
    if min(B, H, W) <= 0:
        raise ValueError(f"image: an empty image, {shape}")
    if max(H, W) > MAX_SIDE:
        raise ValueError(f"image: {H} x {W} is larger than {MAX_SIDE} a side")

    # ---- the maps --------------------------------------------------------------------------------------------------
    lut = None
    if heatmap is not None:
        lut = colormap_table(colormap)
        heatmap = arrays["heatmap"]
        hshape = tuple(heatmap.shape)
        if _dtype(heatmap) != "float32":
            raise TypeError(f"heatmap: expected float32, got {_dtype(heatmap)}")
        if len(hshape) != (4 if batched else 3) or (batched and hshape[0] != B):
            raise ValueError(f"heatmap: expected {'[%d, K, h, w]' % B if batched else '[K, h, w]'}, got {hshape}")
        if min(hshape) <= 0:
            raise ValueError(f"heatmap: an empty dimension, {hshape}")
        if max(hshape[-2:]) > MAX_SIDE:
            raise ValueError(f"heatmap: {hshape[-2]} x {hshape[-1]} maps are larger than {MAX_SIDE} a side")
    elif colormap not in COLORMAPS:
        raise ValueError(f"colormap: {colormap!r} is not one of {COLORMAPS}")

    # ---- the poses -------------------------------------------------------------------------------------------------
    draw = None
    if keypoints is not None:
        keypoints, probabilities = arrays["keypoints"], arrays["probabilities"]
        kshape = tuple(keypoints.shape)
        if len(kshape) != 3 or kshape[2] != 2 or kshape[1] == 0:
            raise ValueError(f"keypoints: expected [N, K, 2] with K > 0, got {kshape}")
        N, K = kshape[:2]
        if tuple(probabilities.shape) != (N, K):
            raise ValueError(f"probabilities: expected [{N}, {K}], got {tuple(probabilities.shape)}")
        for n, a in (("keypoints", keypoints), ("probabilities", probabilities)):
            if _dtype(a) not in ("float32", "float64"):
                raise TypeError(f"{n}: expected float32 or float64, got {_dtype(a)}")
        if not isinstance(threshold, (int, float, np.floating, np.integer)) or np.isnan(threshold):
            raise ValueError(f"threshold: {threshold!r} is not a number")
        radius = _int_in(radius, 0, MAX_SIDE, "radius")
        line_width = _int_in(line_width, 1, MAX_SIDE, "line_width")
        style, L = _style_table(K, colors, skeleton, limb_colors)
        if N * max(K, L) >= 1 << 31:
            raise ValueError(f"keypoints: {N} instances of {K} keypoints and {L} limbs are too many")
        draw = (N, K, style, L, _instance_order(image_index, N, B))

    # ---- device ----------------------------------------------------------------------------------------------------
    if not on_device:
        _lib.require_device()
    device = image.device if on_device else torch.device("cuda", torch.cuda.current_device())
    keep = []
    oshape = (B, H, W, 3) if batched else (H, W, 3)
    result = _check_out(out, oshape, device) if on_device else None
    with torch.cuda.device(device):
        d_image = upload(image, device, keep)
        d_heat = d_lut = None
        if heatmap is not None:
            d_heat = upload(heatmap, device, keep)
            d_heat = d_heat if batched else d_heat[None]
            d_lut = _device_table(lut, device)
        d_draw = None
        if draw:
            N, K, style, L, order = draw
            inst, off = order(device, keep)
            d_draw = (_room(upload(keypoints, device, keep, torch.float64)),
                      _room(upload(probabilities, device, keep, torch.float64)), _room(inst), off,
                      _device_table(style, device), N, K, L, float(threshold), radius, line_width)
        if result is None:
            result = torch.empty(oshape, dtype=torch.uint8, device=device)
        ops.viz_render(d_image, result.view(B, H, W, 3), d_heat, d_lut, d_draw)
    return result if on_device else result.cpu().numpy()


def overlay_heatmap_on_image(image, heatmap, colormap: str = "jet", *, out=None):
    """The reference's ``overlay_heatmap_on_image``: image uint8 [H, W, 3] with heatmap float32 [K, h, w] -> uint8
    [H, W, 3]; also batched, [B, H, W, 3] (or float32 [B, 3, H, W] in [0, 1]) with [B, K, h, w].  Saturates where the
    reference wraps (module docstring); maps of another size than the image are upsampled bilinearly."""
    if heatmap is None:
        raise ValueError("heatmap: None")
    return render(image, heatmap, colormap=colormap, out=out)


def draw_keypoints(image, keypoints, probabilities, *, threshold: float = 0.9, radius: int = 5, colors=(255, 0, 0),
                   skeleton=None, limb_colors=None, line_width: int = 2, image_index=None, out=None):
    """The drawing loop of the reference's inference.py:115-125 without its text labels, plus limbs: image uint8
    [B, H, W, 3] or [H, W, 3], keypoints [N, K, 2], probabilities [N, K], ``image_index`` int [N] (default
    ``arange(B)``: instance n on image n) says which image each instance is drawn on, so several people can land on
    one frame.  ``colors``: one RGB triple or [K, 3]; ``skeleton``: (i, j) pairs; ``limb_colors``: a triple or [L, 3],
    by default the colour of keypoint i."""
    if keypoints is None or probabilities is None:
        raise ValueError("keypoints / probabilities: None")
    if not isinstance(image, torch.Tensor):
        image = np.asarray(image)
    if _dtype(image) != "uint8":
        raise TypeError(f"image: expected uint8 [B, H, W, 3] or [H, W, 3], got {_dtype(image)}")
    return render(image, None, keypoints, probabilities, threshold=threshold, radius=radius, colors=colors,
                  skeleton=skeleton, limb_colors=limb_colors, line_width=line_width, image_index=image_index, out=out)


def colorize(heatmaps, colormap: str = "inferno", normalize: bool = False, *, out=None):
    """float32 [..., h, w] -> uint8 [..., h, w, 4]: the reference CLI's ``(cm.inferno(hm) * 255).astype(np.uint8)``,
    with ``normalize`` its ``hm / hm.max()`` per map first."""
    lut = colormap_table(colormap)
    (_, maps), = _placement([("heatmaps", heatmaps)], out)[0]
    on_device = isinstance(maps, torch.Tensor)
    shape = tuple(maps.shape)
    if _dtype(maps) != "float32":
        raise TypeError(f"heatmaps: expected float32, got {_dtype(maps)}")
    if len(shape) < 2 or shape[-1] <= 0 or shape[-2] <= 0:
        raise ValueError(f"heatmaps: expected [..., h, w] with h, w > 0, got {shape}")
    if shape[-1] * shape[-2] >= 1 << 29:
        raise ValueError(f"heatmaps: {shape[-2]} x {shape[-1]} maps are too large")
    if not on_device:
        _lib.require_device()
    device = maps.device if on_device else torch.device("cuda", torch.cuda.current_device())
    result = _check_out(out, shape + (4,), device) if on_device else None
    keep = []
    with torch.cuda.device(device):
        d_maps = upload(maps, device, keep)
        if result is None:
            result = torch.empty(shape + (4,), dtype=torch.uint8, device=device)
        if d_maps.numel():
            ops.viz_colorize(d_maps, _device_table(lut, device), result, normalize)
    return result if on_device else result.cpu().numpy()
