"""Every form of the crop + LANCZOS front end, on the host (no GPU): the library's plans put the cases of
tests/frontend_forms.py into the forms the table names; the plans' block tables, spans and LDS offsets hold their
invariants; the plans executed in numpy block by block equal Pillow bit for bit; the bytes the kernel's load
expressions may touch lie inside the source buffer; a many-box (threaded) plan carries its refusals back.
Single-frame and multi-source builders alike.  tests/test_frontend_forms_gpu.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

from tests import frontend_forms as ff


def _boxes(case):
    from probpose_pytorch_amd.frontend import round_boxes
    return round_boxes(case.boxes())


def _plans(lib, case):
    """[(multi, decoded plan, host words, sources or None, source bytes)] for the case: single frame, multi-source."""
    boxes = _boxes(case)
    total, sources = ff.pack(ff.case_regions(case), fill=False)
    res = []
    for src in (None, sources):
        host, nb, lds = ff.build_plan(lib, boxes, case.out, src, total)
        res.append((src is not None, ff.read_plan(host, len(boxes), src is not None, nb, lds), host, src, total))
    return res


CASE = pytest.mark.parametrize("case", ff.CASES, ids=ff.CASE_IDS)


def test_cases_reach_their_forms(built_lib):
    staged, direct, T, F = "staged", "direct", True, False
    for multi in (False, True):
        seen = set()        # (rb, path, need_h, need_v, big LDS, partial last block, rb below fe_rb_max)
        for case in ff.CASES:
            p = _plans(built_lib, case)[int(multi)][1]
            out_w, out_h = case.out
            assert (p.out_w, p.out_h) == (out_w, out_h) and p.n == len(case.boxes())
            assert ff.fe_rb_max(p.n, out_h) == case.rb_max, case.id
            forms = {ff.form_of(b, p.lds_bytes) for b in p.boxes}
            assert forms == set(case.forms), (case.id, multi, sorted(forms))
            seen |= {ff.form_of(b, p.lds_bytes) + (out_h % b.rb != 0, b.rb < case.rb_max) for b in p.boxes}
        for path, dirs in ((staged, ((T, T), (T, F), (F, T), (F, F))), (direct, ((T, T), (T, F), (F, T), (F, F)))):
            for nh, nv in dirs:
                assert any(s[1:4] == (path, nh, nv) for s in seen), (multi, path, nh, nv)
            assert any(s[1] == path and s[4] for s in seen), (multi, path, "LDS > 64 KB")
        for rb in (1, 2, 4, 8, 16, 32):
            assert any(s[0] == rb for s in seen), (multi, rb)
            assert rb == 1 or any(s[0] == rb and s[5] for s in seen), (multi, rb, "partial last block")
        assert any(s[6] for s in seen), (multi, "rb below fe_rb_max")


@CASE
def test_plan_invariants(built_lib, case):
    out_w, out_h = case.out
    for multi, p, host, sources, total in _plans(built_lib, case):
        assert 0 < p.lds_bytes <= 152 * 1024
        if multi:
            assert np.array_equal(p.records, sources)
        want = [(c, r0) for c, b in enumerate(p.boxes) for r0 in range(0, out_h, b.rb)]
        assert [tuple(int(v) for v in e) for e in p.blocks] == want            # each (box, r0) once, in order
        for b in p.boxes:
            bv = b.bv.astype(np.int64)
            for r0 in range(0, out_h, b.rb):
                r1 = min(out_h, r0 + b.rb)
                span = int(bv[r1 - 1, 0] + bv[r1 - 1, 1] - bv[r0, 0])
                assert 0 < span and ((span * out_w * 3 + 15) & ~15) <= b.coef_off, (case.id, b.index, r0)
                # every row of the block reads inside the block's rows (bounds are monotone in Pillow's tables)
                assert (bv[r0:r1, 0] >= bv[r0, 0]).all() and (bv[r0:r1].sum(1) <= bv[r1 - 1].sum()).all()
            assert b.coef_off % 16 == 0 and b.coef_off <= p.lds_bytes
            if b.staged:
                assert b.src_off % 16 == 0 and b.src_off >= b.coef_off + 4 * out_w * (b.ksh + 2)
                assert b.src_off + ff.FE_SRC_ROWS * (((3 * b.cw + 3) & ~3) + 4) <= p.lds_bytes
            for bounds, size in ((b.bh, b.cw), (bv, b.ch)):
                assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 0).all(), (case.id, b.index)
                assert (bounds[:, 0] + bounds[:, 1] <= size).all(), (case.id, b.index)
            assert (b.bh[:, 1] <= b.ksh).all() and (bv[:, 1] <= b.ksv).all()
            assert b.need_h == (b.cw != out_w) and b.need_v == (b.ch != out_h)


@CASE
def test_apply_plan_equals_pillow(built_lib, case):
    out_w, out_h = case.out
    regions = ff.case_regions(case)
    (_, ps, host_s, _, _), (_, pm, host_m, _, _) = _plans(built_lib, case)
    packed, _ = ff.pack(regions)
    for multi, p, host, src in ((False, ps, host_s, ff.case_frame(case.id, 0)), (True, pm, host_m, packed)):
        got = ff.apply_plan(host, p.n, src, out_w, out_h)
        for i, want in enumerate(ff.pillow_reference(case.id, multi)):
            assert np.array_equal(got[i], want), (case.id, multi, i, ff.form_of(p.boxes[i], p.lds_bytes),
                                                  ff.first_difference(got[i], want))


def test_apply_plan_refuses_a_row_outside_the_block(built_lib):
    """apply_plan's own check: a block whose vertical bounds reach past its span is refused, not computed."""
    case = ff.CASES[ff.CASE_IDS.index("partial-17")]
    host, nb, lds = ff.build_plan(built_lib, _boxes(case), case.out)
    p = ff.read_plan(host, 17, False, nb, lds)
    r = p.boxes[3].rb - 2                                  # a row inside a block: reach one row past the block's last
    p.boxes[3].bv[r, 1] = p.boxes[3].bv[p.boxes[3].rb - 1].sum() - p.boxes[3].bv[r, 0] + 1     # (a view of host)
    with pytest.raises(ValueError, match="outside"):
        ff.apply_plan(host, 17, ff.case_frame(case.id, 0), *case.out)


def _inside(extent, lo, hi, what):
    if extent is not None:
        assert lo <= extent[0] <= extent[1] < hi, (what, extent, (lo, hi))


@CASE
def test_read_extents_stay_inside_the_buffer(built_lib, case):
    h, w = case.frame
    (_, ps, _, _, _), (_, pm, _, sources, total) = _plans(built_lib, case)
    for b in ps.boxes:
        _inside(ff.read_extent(b, w, h, 3 * w), 0, 3 * w * h, (case.id, b.index))
    for b, (off, sw, sh, stride) in zip(pm.boxes, sources):
        end = int(off + (sh - 1) * stride + 3 * sw)
        assert end + ff.SRC_PAD <= total
        _inside(ff.read_extent(b, 0, 0, 0, multi_record=b.src), int(off), end + ff.SRC_PAD, (case.id, b.index, "multi"))
    # every case reads something: an extent of None for all boxes would make the above vacuous
    assert any(ff.read_extent(b, w, h, 3 * w) is not None for b in ps.boxes)


def test_further_boxes_reach_their_forms(built_lib):
    """The boxes of the GPU file's strided-view and outside-the-frame tests take the passes those tests are about."""
    from probpose_pytorch_amd.frontend import round_boxes
    for boxes, size, want in ((ff.VIEW_BOXES, ff.VIEW_SIZE, [True] * 4 + [False]),
                              (ff.OUTSIDE_BOXES, ff.OUTSIDE_SIZE, [True] * 4 + [False] * 4)):
        host, nb, lds = ff.build_plan(built_lib, round_boxes(boxes), size)
        assert [b.staged for b in ff.read_plan(host, len(boxes), False, nb, lds).boxes] == want


STRIDED_BOXES = [(0, 0, 401, 300), (380, 280, 40, 40), (400, 299, 1, 1), (-5, 250, 2900, 60), (0, 0, 2900, 300)]


def test_read_extents_of_a_row_strided_view(built_lib):
    """The left 401 columns of a 512-wide, 300-row buffer: nothing past the view's last pixel, staged and direct."""
    w, h, stride = 401, 300, 3 * 512
    boxes = np.array([[x, y, x + bw, y + bh] for x, y, bw, bh in STRIDED_BOXES], dtype=np.int32)
    host, nb, lds = ff.build_plan(built_lib, boxes, (192, 256))
    p = ff.read_plan(host, len(boxes), False, nb, lds)
    assert {b.staged for b in p.boxes} == {True, False}
    for b in p.boxes:
        e = ff.read_extent(b, w, h, stride)
        _inside(e, 0, (h - 1) * stride + 3 * w, b.index)
    assert ff.read_extent(p.boxes[2], w, h, stride) == ((h - 1) * stride + 3 * (w - 1), (h - 1) * stride + 3 * w - 1)
    assert ff.read_extent(p.boxes[4], w, h, stride)[1] == (h - 1) * stride + 3 * w - 1     # direct, the last pixel


# ---- refusals inside a many-box plan ---------------------------------------------------------------------------------
def _good64():
    rng = np.random.default_rng(37)
    x, y = rng.integers(-20, 500, 64), rng.integers(-20, 400, 64)
    return np.stack([x, y, x + rng.integers(8, 300, 64), y + rng.integers(8, 300, 64)], 1).astype(np.int32)


EMPTY, TALL = (10, 10, 10, 50), (0, 0, 192, 102400)


def _refused(lib, boxes, sources=None, src_bytes=0):
    """(plan_bytes' value and message, plan_build's status and message) for a 192x256 plan of the boxes."""
    bp = boxes.ctypes.data_as(C.c_void_p)
    good = _good64()
    words = lib.pp_frontend_multi_plan_bytes(64, good.ctypes.data_as(C.c_void_p), 192, 256) // 4
    host = np.zeros(words, dtype=np.int32)                 # a refused build writes nothing; this is room to spare
    nb, lds = C.c_int(0), C.c_longlong(0)
    if sources is None:
        size = lib.pp_frontend_plan_bytes(64, bp, 192, 256)
        size_msg = lib.pp_last_error()
        rc = lib.pp_frontend_plan_build(64, bp, 192, 256, host.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(lds))
    else:
        size = lib.pp_frontend_multi_plan_bytes(64, bp, 192, 256)
        size_msg = lib.pp_last_error()
        rc = lib.pp_frontend_multi_plan_build(64, bp, sources.ctypes.data_as(C.c_void_p), src_bytes, 192, 256,
                                              host.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(lds))
    return size, size_msg, rc, lib.pp_last_error()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_refusals_in_a_many_box_plan(built_lib, multi):
    good = _good64()
    sources = np.tile(np.array([[0, 640, 480, 3 * 640]], dtype=np.int64), (64, 1)) if multi else None
    src_bytes = 3 * 640 * 480 + 4
    size, _, rc, _ = _refused(built_lib, good, sources, src_bytes)
    assert size > 0 and rc == 0, built_lib.pp_last_error()               # the 64 good boxes are accepted
    for bad, texts in (({37: EMPTY}, (b"empty box",)), ({37: TALL}, (b"LDS",)),
                       ({5: EMPTY, 37: TALL}, (b"empty box", b"LDS")), ({5: TALL, 37: EMPTY}, (b"empty box", b"LDS"))):
        boxes = good.copy()
        for i, b in bad.items():
            boxes[i] = b
        size, size_msg, rc, msg = _refused(built_lib, boxes, sources, src_bytes)
        assert size < 0 and any(t in size_msg for t in texts), (bad, size, size_msg)
        assert rc != 0 and any(t in msg for t in texts), (bad, rc, msg)


def test_refused_source_records_in_a_many_box_plan(built_lib):
    good = _good64()
    sources = np.tile(np.array([[0, 640, 480, 3 * 640]], dtype=np.int64), (64, 1))
    sources[:, 0] = np.arange(64) * 16
    src_bytes = int(sources[-1, 0]) + 3 * 640 * 480 + 4
    assert _refused(built_lib, good, sources, src_bytes)[2] == 0, built_lib.pp_last_error()
    bad = sources.copy()
    bad[37, 0] += 2
    rc, msg = _refused(built_lib, good, bad, src_bytes + 64)[2:]
    assert rc != 0 and b"source 37 " in msg and b"misaligned" in msg, msg
    bad = sources.copy()
    bad[41, 0] = sources[-1, 0] + 4
    rc, msg = _refused(built_lib, good, bad, src_bytes)[2:]
    assert rc != 0 and b"source 41 " in msg and b"past the end" in msg, msg
