"""TEST INFRASTRUCTURE: the forms of the crop + LANCZOS front end (csrc/pp_frontend.hip) and the cases that reach them.

A box's *form* is the code path ``crop_resize_kernel`` takes for it: ``(rb, "staged" | "direct", need_h, need_v,
launch LDS > 64 KB)``.  Two host functions choose it: ``fe_prepare`` per box (crop size, output size, the LDS budgets)
and ``fe_rb_max`` from the number of boxes in the launch.  This module holds

* ``read_plan`` / ``form_of``: a plan built by the library, decoded (the header slots are the ``H_*`` enum of
  pp_frontend.hip, named here and nowhere else in the tests);
* ``CASES``: the literal table of frames, output sizes and boxes, each with the exact set of forms its boxes must take
  (tests/test_frontend_forms.py holds the library's plans to it, tests/test_frontend_forms_gpu.py runs them);
* ``apply_plan``: the plan executed in numpy block by block as the kernel organises it, so the host side (tables, block
  table, spans, rb) is tested without a GPU and a GPU mismatch is then known to be device code;
* ``read_extent``: the lowest and highest byte of the source buffer the horizontal pass (the only one that reads it)
  may touch for a box, derived from the kernel's load expressions.

The direct pass with a copy in BOTH directions was first thought to need a 1024-px-wide crop more than ~8700 rows high
and was to be left out.  It does not: the direct pass is taken when temporary rows + coefficient table + source-row
buffer exceed 128 KB, and with need_h == need_v == 0 all three grow with the crop's width alone (6 rows of 3 w bytes,
9 ints per column, 8 rows of 3 w + 4 bytes), so an identity crop 1700 px wide or more is direct at any height.
``direct-copy-both`` (1800 px wide, 16 rows) covers it.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np

from oracle import frontend_oracle as fo

# ---- pp_frontend.hip's constants, by name ---------------------------------------------------------------------------
FE_HDR, FE_SRC_WORDS, FE_SRC_ROWS = 16, 8, 8
(H_X0, H_Y0, H_CW, H_CH, H_KSH, H_KSV, H_COEF_OFF, H_SRC_OFF, H_OFF_BH, H_OFF_KH, H_OFF_BV, H_OFF_KV, H_NEED_H, H_NEED_V,
 H_RB, H_STAGED) = range(FE_HDR)
SRC_PAD = 4                                     # PP_FRONTEND_SRC_PAD
HALF = 1 << (fo.PRECISION_BITS - 1)


def fe_rb_max(n_boxes: int, out_h: int) -> int:
    """pp_frontend.hip fe_rb_max: output rows per workgroup before a box's LDS need lowers it."""
    rb = 32
    while rb > 1 and n_boxes * ((out_h + rb - 1) // rb) < 1024:
        rb >>= 1
    return rb


def frame(h: int, w: int, seed: int) -> np.ndarray:
    """Seeded (h, w, 3) uint8 test frame: noise, the upper half mixed with a smooth pattern."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = ((np.sin(xx / 17.0) + np.cos(yy / 23.0)) * 60 + 128).clip(0, 255).astype(np.uint8)
    base[: h // 2] = (base[: h // 2] // 4 + smooth[: h // 2, :, None] * 3 // 4).astype(np.uint8)
    return base


# ---- building and reading plans -------------------------------------------------------------------------------------
def build_plan(lib, boxes_xyxy, size, sources=None, src_bytes=0):
    """The library's plan for integer boxes: (host int32 words, n_blocks, lds_bytes).  sources [n, 4] int64: the
    multi-source builder."""
    boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
    n, bp = boxes.shape[0], boxes.ctypes.data_as(C.c_void_p)
    nb, lds = C.c_int(0), C.c_longlong(0)
    if sources is None:
        nbytes = lib.pp_frontend_plan_bytes(n, bp, size[0], size[1])
        assert nbytes > 0, lib.pp_last_error()
        host = np.zeros(nbytes // 4, dtype=np.int32)
        rc = lib.pp_frontend_plan_build(n, bp, size[0], size[1], host.ctypes.data_as(C.c_void_p), C.byref(nb),
                                        C.byref(lds))
    else:
        src = np.ascontiguousarray(sources, dtype=np.int64).reshape(n, 4)
        nbytes = lib.pp_frontend_multi_plan_bytes(n, bp, size[0], size[1])
        assert nbytes > 0, lib.pp_last_error()
        host = np.zeros(nbytes // 4, dtype=np.int32)
        rc = lib.pp_frontend_multi_plan_build(n, bp, src.ctypes.data_as(C.c_void_p), int(src_bytes), size[0], size[1],
                                              host.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(lds))
    assert rc == 0, lib.pp_last_error()
    return host, int(nb.value), int(lds.value)


def read_plan(host, n, multi, n_blocks=None, lds_bytes=None):
    """Decode a plan of n >= 1 boxes.  Returns a namespace: ``boxes`` (per box x0, y0, cw, ch, ksh, ksv, need_h, need_v,
    rb, staged, coef_off, src_off, the tables bh [out_w, 2], kh [out_w, ksh], bv [out_h, 2], kv [out_h, ksv] and, for
    multi, ``src`` = (byte offset, width, height, row stride)), ``blocks`` [n_blocks, 2] = (box, first output row),
    ``out_w``, ``out_h``, ``n_blocks`` and ``lds_bytes`` (what the build returned, when given)."""
    host = np.ascontiguousarray(host, dtype=np.int32)
    hdr = host[:n * FE_HDR].reshape(n, FE_HDR)
    pos = n * FE_HDR
    records = None
    if multi:
        records = host[pos:pos + n * FE_SRC_WORDS].view(np.int64).reshape(n, 4)
        pos += n * FE_SRC_WORDS
    first = int(hdr[0, H_OFF_BH])             # the tables follow the block table, box 0's bounds first
    if first < pos or (first - pos) % 2:
        raise ValueError(f"block table of {first - pos} words")
    nb = (first - pos) // 2
    if n_blocks is not None and nb != n_blocks:
        raise ValueError(f"the build returned {n_blocks} blocks, the plan holds {nb}")
    out_w = int(hdr[0, H_OFF_KH] - hdr[0, H_OFF_BH]) // 2
    out_h = int(hdr[0, H_OFF_KV] - hdr[0, H_OFF_BV]) // 2
    boxes = []
    for c in range(n):
        h = [int(v) for v in hdr[c]]
        ksh, ksv = h[H_KSH], h[H_KSV]
        boxes.append(SimpleNamespace(
            index=c, x0=h[H_X0], y0=h[H_Y0], cw=h[H_CW], ch=h[H_CH], ksh=ksh, ksv=ksv, need_h=bool(h[H_NEED_H]),
            need_v=bool(h[H_NEED_V]), rb=h[H_RB], staged=bool(h[H_STAGED]), coef_off=h[H_COEF_OFF],
            src_off=h[H_SRC_OFF],
            bh=host[h[H_OFF_BH]:h[H_OFF_BH] + 2 * out_w].reshape(out_w, 2),
            kh=host[h[H_OFF_KH]:h[H_OFF_KH] + ksh * out_w].reshape(out_w, ksh),
            bv=host[h[H_OFF_BV]:h[H_OFF_BV] + 2 * out_h].reshape(out_h, 2),
            kv=host[h[H_OFF_KV]:h[H_OFF_KV] + ksv * out_h].reshape(out_h, ksv),
            src=tuple(int(v) for v in records[c]) if multi else None))
    return SimpleNamespace(n=n, multi=bool(multi), boxes=boxes, records=records, blocks=host[pos:first].reshape(nb, 2),
                           out_w=out_w, out_h=out_h, n_blocks=nb, lds_bytes=lds_bytes)


def form_of(box_plan, lds_bytes) -> Tuple[int, str, bool, bool, bool]:
    return (box_plan.rb, "staged" if box_plan.staged else "direct", box_plan.need_h, box_plan.need_v,
            lds_bytes > 65536)


# ---- the plan executed in numpy, block by block ---------------------------------------------------------------------
def _region(src: np.ndarray, record) -> np.ndarray:
    off, sw, sh, stride = record
    if off < 0 or off + (sh - 1) * stride + 3 * sw > src.size:
        raise ValueError(f"region {record} leaves the {src.size}-byte buffer")
    return np.lib.stride_tricks.as_strided(src[off:], shape=(sh, sw, 3), strides=(stride, 3, 1), writeable=False)


def _dense(bounds, kk, in_size):
    """[out, in_size] float64 matrix of a bounds / coefficient table (taps x < xmax only, as the kernel loops).  The
    products and sums stay below 2^53, so float64 matmul is exact integer arithmetic."""
    m = np.zeros((bounds.shape[0], in_size), dtype=np.float64)
    for o, (lo, cnt) in enumerate(bounds):
        if lo < 0 or cnt < 0 or lo + cnt > in_size:
            raise ValueError(f"output {o}: taps [{lo}, {lo + cnt}) outside [0, {in_size})")
        m[o, lo:lo + cnt] = kk[o, :cnt]
    return m


def _clip8(acc):
    return np.clip((acc.astype(np.int64) + HALF) >> fo.PRECISION_BITS, 0, 255).astype(np.uint8)


def apply_plan(host, n, frame_or_sources, out_w, out_h) -> np.ndarray:
    """(n, 3, out_h, out_w) float32: the plan run block by block.  frame_or_sources: the (H, W, 3) uint8 frame of a
    single-frame plan, or the flat packed uint8 source buffer of a multi-source plan.  Raises ValueError when a block
    reads a temporary row outside its [0, span)."""
    src = np.asarray(frame_or_sources)
    p = read_plan(host, n, src.ndim == 1)
    if (p.out_w, p.out_h) != (out_w, out_h):
        raise ValueError(f"the plan is for {p.out_w}x{p.out_h}")
    out = np.full((n, 3, out_h, out_w), np.nan, dtype=np.float32)
    cur, crop, mat_h = -1, None, None
    for c, r0 in ((int(a), int(b)) for a, b in p.blocks):
        b = p.boxes[c]
        if c != cur:
            image = _region(src, b.src) if p.multi else src
            crop = fo.crop_zero_pad(image, (b.x0, b.y0, b.x0 + b.cw, b.y0 + b.ch))     # zeros outside the frame
            mat_h = _dense(b.bh, b.kh, b.cw) if b.need_h else None
            cur = c
        r1 = min(out_h, r0 + b.rb)
        s0, s1 = int(b.bv[r0, 0]), int(b.bv[r1 - 1, 0] + b.bv[r1 - 1, 1])
        span = s1 - s0
        if not 0 <= s0 < s1 <= b.ch:
            raise ValueError(f"box {c} block {r0}: source rows [{s0}, {s1}) outside the crop's {b.ch}")
        tmp = np.zeros(span * out_w * 3, dtype=np.uint8)                # the block's LDS rows, and not a byte more
        t = tmp.reshape(span, out_w, 3)
        rows = crop[s0:s1]
        if b.need_h:
            flat = rows.astype(np.float64).transpose(1, 0, 2).reshape(b.cw, span * 3)
            t[:] = _clip8(mat_h @ flat).reshape(out_w, span, 3).transpose(1, 0, 2)      # [out_w, cw] @ [cw, span * 3]
        else:
            t[:] = rows                                                  # cw == out_w
        lo, cnt = b.bv[r0:r1, 0].astype(np.int64) - s0, b.bv[r0:r1, 1].astype(np.int64)
        if b.need_v:
            if (lo < 0).any() or (lo + cnt > span).any():
                raise ValueError(f"box {c} block {r0}: the vertical pass reads temporary rows outside [0, {span})")
            bounds = np.stack([lo, cnt], 1)
            res = _clip8(_dense(bounds, b.kv[r0:r1], span) @ t.reshape(span, -1).astype(np.float64)).reshape(-1, out_w, 3)
        else:
            idx = np.arange(r0, r1) - s0
            if (idx < 0).any() or (idx >= span).any():
                raise ValueError(f"box {c} block {r0}: the vertical copy reads temporary rows outside [0, {span})")
            res = t[idx]
        out[c, :, r0:r1, :] = (res.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(2, 0, 1)
    return out


# ---- what the horizontal pass may read ------------------------------------------------------------------------------
def read_extent(box_plan, frame_w, frame_h, stride, multi_record=None) -> Optional[Tuple[int, int]]:
    """(lowest byte offset read, highest byte offset read) in the source buffer for this box, None when the box reads
    nothing.  From the kernel's code.  Rows: crop rows [bv[0].min, bv[-1].min + bv[-1].count) (the union of the blocks'
    [s0, s1)) at frame row y0 + row, when inside the frame.  Staged: per row the dwords d < (3 cw + 3) >> 2 at row
    byte o = 3 x0 + 4 d, whole when 0 <= o and o + 4 <= 3 img_w, else those of its bytes inside [0, 3 img_w).  Direct
    with need_h: a 4-byte load at 3 ix for every tap inside the frame, 3 single bytes for the last pixel of the last
    row; direct copy: the 3 bytes of every crop pixel inside the frame.  multi_record (byte offset, width, height,
    stride) replaces the frame arguments, as the kernel does."""
    b, base = box_plan, 0
    if multi_record is not None:
        base, frame_w, frame_h, stride = (int(v) for v in multi_record)
    first, last = int(b.bv[0, 0]), int(b.bv[-1, 0] + b.bv[-1, 1])
    iy = np.arange(b.y0 + first, b.y0 + last, dtype=np.int64)
    iy = iy[(iy >= 0) & (iy < frame_h)]
    if iy.size == 0:
        return None
    rowbytes = 3 * frame_w
    if b.staged:
        o = 3 * b.x0 + 4 * np.arange((3 * b.cw + 3) >> 2, dtype=np.int64)
        whole = (o >= 0) & (o + 4 <= rowbytes)
        byte = (o[~whole, None] + np.arange(4)).reshape(-1)
        byte = byte[(byte >= 0) & (byte < rowbytes)]
        los = np.concatenate([o[whole], byte])
        his = np.concatenate([o[whole] + 3, byte])
        if los.size == 0:
            return None
        row_lo = np.full(iy.shape, los.min())
        row_hi = np.full(iy.shape, his.max())
    else:
        if b.need_h:
            taps = np.concatenate([b.x0 + lo + np.arange(cnt, dtype=np.int64) for lo, cnt in b.bh])
        else:
            taps = b.x0 + np.arange(b.cw, dtype=np.int64)
        taps = taps[(taps >= 0) & (taps < frame_w)]
        if taps.size == 0:
            return None
        row_lo = np.full(iy.shape, 3 * taps.min())
        width = 4 if b.need_h else 3
        row_hi = np.full(iy.shape, 3 * taps.max() + width - 1)
        if b.need_h and taps.max() == frame_w - 1:
            # the last row reads its last pixel bytewise; its other taps load 4 bytes
            inner = taps[taps < frame_w - 1]
            last_hi = max(3 * (frame_w - 1) + 2, 3 * int(inner.max()) + 3 if inner.size else 0)
            row_hi[iy == frame_h - 1] = last_hi
    return int((base + iy * stride + row_lo).min()), int((base + iy * stride + row_hi).max())


# ---- the cases ------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    id: str
    frame: Tuple[int, int]              # (h, w) of the frame, seeded with `seed`
    seed: int
    out: Tuple[int, int]                # (w, h) of the crops
    boxes: Callable[[], list]           # [x, y, w, h] floats
    forms: frozenset                    # exactly the forms (rb, path, need_h, need_v, launch LDS > 64 KB) of its boxes
    rb_max: int                         # fe_rb_max of the launch
    second: Optional[Tuple[int, int]] = None   # "multi: mixed": the odd boxes read a second frame of this (h, w)


def _seeded(seed, n, xr, yr, wh):
    def make():
        rng = np.random.default_rng(seed)
        return [(float(rng.uniform(*xr)), float(rng.uniform(*yr)), float(rng.uniform(*wh)), float(rng.uniform(*wh)))
                for _ in range(n)]
    return make


def _lit(*boxes):
    return lambda: [tuple(float(v) for v in b) for b in boxes]


def _workload(n):
    return _seeded(64, n, (-50, 600), (-50, 440), (8, 500))


def _partial(n):
    return _seeded(250, n, (-20, 110), (-20, 80), (1, 160))


S, D, T, F = "staged", "direct", True, False


def _forms(*f):
    return frozenset(f)


# The forms are the library's plans, written out (tests/test_frontend_forms.py::test_cases_reach_their_forms fails when
# a threshold of fe_prepare / fe_rb_max moves a box: repair the case then, not the assertion).  partial-9 has out_h =
# 250, a multiple of its rb = 2, so partial-9-odd (out_h = 251) supplies the partial last block at rb 2.
CASES = (
    Case("direct-hv", (41, 2801), 11, (192, 32), _lit((0, 0, 2800, 40), (1, 1, 2800, 40)),
         _forms((1, D, T, T, F)), 1),
    # taps left and right of the frame; the last row's last pixel inside the crop
    Case("direct-hv-margins", (41, 2801), 12, (64, 24), _lit((-300, -8, 3000, 48), (-100, -3, 3100, 50)),
         _forms((1, D, T, T, F)), 1, second=(37, 2799)),
    Case("direct-h-only-rb2", (33, 2801), 13, (48, 32), _lit(*[(x, 0, 2800, 32) for x in range(-32, 32)]),
         _forms((2, D, T, F, F)), 2),
    Case("direct-copy-h-big-lds", (64, 1024), 14, (1024, 16), _lit((0, 0, 1024, 64)),
         _forms((1, D, F, T, T)), 1),
    # the crop leaves the frame above and below
    Case("staged-big-lds", (480, 640), 15, (192, 256), _lit((0, -1760, 192, 4000)),
         _forms((1, S, F, T, T)), 1),
    Case("staged-copy-both-big", (16, 1024), 16, (1024, 16), _lit((0, 0, 1024, 16)),
         _forms((1, S, F, F, T)), 1),
    # identity crops too wide for the staged pass's tables; the second leaves the frame on the left and below
    Case("direct-copy-both", (19, 1801), 23, (1800, 16), _lit((1, 2, 1800, 16), (-3, 5, 1800, 16)),
         _forms((1, D, F, F, F)), 1),
    Case("rb-lowered", (480, 640), 17, (192, 256),
         _lit(*[(i, -1260, 192, 3000) if i % 2 == 0 else (i, -760, 400, 2000) for i in range(128)]),
         _forms((4, S, F, T, T), (8, S, T, T, T)), 32),       # the launch's LDS is the rb-8 boxes': 81440 B
    Case("workload-64", (480, 641), 18, (192, 256), _workload(64), _forms((16, S, T, T, F)), 16, second=(355, 517)),
    Case("workload-128", (480, 641), 18, (192, 256), _workload(128),
         _forms((32, S, T, T, F), (32, S, T, F, F)), 32),       # two boxes round to 256 rows: horizontal only
    Case("partial-9", (97, 131), 19, (12, 250), _partial(9), _forms((2, S, T, T, F)), 2),
    Case("partial-9-odd", (97, 131), 19, (12, 251), _partial(9), _forms((2, S, T, T, F)), 2),
    Case("partial-17", (97, 131), 19, (12, 250), _partial(17), _forms((4, S, T, T, F)), 4, second=(61, 93)),
    Case("partial-32", (97, 131), 19, (12, 250), _partial(32), _forms((8, S, T, T, F)), 8),
    Case("partial-64", (97, 131), 19, (12, 250), _partial(64),
         _forms((16, S, T, T, F), (16, S, F, T, F)), 16),       # one box rounds to 12 columns: vertical only
    Case("partial-128", (97, 131), 19, (12, 250), _partial(128),
         _forms((32, S, T, T, F), (32, S, F, T, F)), 32),
    # out smaller than any kernel; (130, 96, 1, 1) is the frame's last pixel
    Case("tiny-out-1x1", (97, 131), 20, (1, 1), _lit((3, 4, 50, 60), (0, 0, 1, 1), (130, 96, 1, 1)),
         _forms((1, S, T, T, F), (1, S, F, F, F)), 1),
    Case("tiny-out-3x2", (97, 131), 20, (3, 2), _lit((3, 4, 50, 60), (0, 0, 1, 1), (130, 96, 1, 1)),
         _forms((1, S, T, T, F)), 1),
    # img_h == 1: every row is the last row
    Case("one-row-frame-1x37", (1, 37), 21, (8, 8), _lit((0, 0, 37, 1), (-2, -2, 41, 5)), _forms((1, S, T, T, F)), 1),
    Case("one-row-frame-37x1", (37, 1), 22, (8, 8), _lit((0, 0, 1, 37), (-2, -2, 41, 5)), _forms((1, S, T, T, F)), 1),
)
CASE_IDS = tuple(c.id for c in CASES)


# Boxes of the further GPU tests; test_frontend_forms.py::test_further_boxes_reach_their_forms pins their forms.
# A 300x401 (h, w) frame: the first four staged, the last direct; (400, 299, 1, 1) and the last one include the last
# pixel of the last row.
VIEW_SIZE = (192, 256)
VIEW_BOXES = ((20.0, 30.0, 150.0, 220.0), (380.0, 280.0, 40.0, 40.0), (400.0, 299.0, 1.0, 1.0), (0.0, 0.0, 401.0, 300.0),
              (-5.0, 250.0, 2900.0, 60.0))
# Left of, right of, above and below a 97x131 (h, w) frame: four staged, four direct.
OUTSIDE_SIZE = (96, 32)
OUTSIDE_BOXES = ((-500.0, 10.0, 300.0, 40.0), (200.0, 10.0, 300.0, 40.0), (10.0, -300.0, 100.0, 200.0),
                 (10.0, 97.0, 100.0, 200.0), (-4000.0, 5.0, 2900.0, 60.0), (131.0, 5.0, 2900.0, 60.0),
                 (-10.0, -80.0, 2900.0, 60.0), (-10.0, 97.0, 2900.0, 60.0))


@functools.lru_cache(maxsize=None)
def case_frame(case_id: str, which: int) -> np.ndarray:
    """The case's frame (which = 0) or its second frame (1), read-only."""
    case = CASES[CASE_IDS.index(case_id)]
    h, w = case.frame if which == 0 else case.second
    img = frame(h, w, case.seed + 100 * which)
    img.setflags(write=False)
    return img


def case_regions(case: Case):
    """Per box the frame it reads through the multi-source entry: the case's frame, or for the odd boxes of a
    "multi: mixed" case the second frame."""
    return [case_frame(case.id, which) for which in case_region_index(case)]


def case_region_index(case: Case):
    """Per box 0 (the case's frame) or 1 (the second frame)."""
    return [1 if case.second and i % 2 else 0 for i in range(len(case.boxes()))]


def pack(regions, fill=True):
    """Every box its own copy of its frame in one packed buffer: (flat uint8 buffer, sources [n, 4] int64).
    fill=False: only the layout, (buffer size in bytes, sources)."""
    from probpose_pytorch_amd.dataset import YOLOPoseDataset
    offs, total = YOLOPoseDataset.pack_layout([r.shape[:2] for r in regions])
    sources = np.array([[off, r.shape[1], r.shape[0], 3 * r.shape[1]] for off, r in zip(offs, regions)], dtype=np.int64)
    if not fill:
        return total, sources
    packed = np.full(total, 0xA5, dtype=np.uint8)          # the gaps and the padding are never part of a result
    for r, off in zip(regions, offs):
        packed[off:off + r.size] = r.reshape(-1)
    return packed, sources


@functools.lru_cache(maxsize=None)
def pillow_reference(case_id: str, multi: bool = False):
    """Pillow's crops of the case, one (3, h, w) float32 array per box, computed once per session and never written
    to.  multi: each box on the frame case_regions gives it."""
    case = CASES[CASE_IDS.index(case_id)]

    def pil(region, b):
        ref = fo.scale_box_pil(region, b, case.out)
        ref.setflags(write=False)
        return ref

    if not multi:
        return tuple(pil(case_frame(case_id, 0), b) for b in case.boxes())
    single = pillow_reference(case_id)
    if not case.second:
        return single
    return tuple(pil(case_frame(case_id, 1), b) if which else single[i]
                 for i, (b, which) in enumerate(zip(case.boxes(), case_region_index(case))))


def first_difference(got: np.ndarray, want: np.ndarray):
    """(channel, y, x), got, want at the first element where two (3, h, w) arrays differ (NaN counts), or None."""
    bad = np.argwhere(~(got == want))
    if bad.size == 0:
        return None
    c, y, x = (int(v) for v in bad[0])
    return (c, y, x), float(got[c, y, x]), float(want[c, y, x])
