"""Every form of crop_resize_kernel (csrc/pp_frontend.hip) on the device, against Pillow itself, bit for bit.

The cases and the forms they reach are tests/frontend_forms.py's (held to the library's plans on the host by
tests/test_frontend_forms.py): the direct and the staged horizontal pass with a pass or a copy in either direction,
row blocks of 1 to 32 output rows with and without a partial last block, launches above 64 KB of LDS, rb lowered below
fe_rb_max, frames whose rows sit at every byte alignment, through ``crop_resize``, through the multi-source kernel and
through the bare C entry with a guarded output.  Integer arithmetic against Pillow: equality is exact, nothing is
measured."""
import numpy as np
import pytest
import torch

from oracle import frontend_oracle as fo
from tests import frontend_forms as ff

pytestmark = pytest.mark.gpu

CASE = pytest.mark.parametrize("case", ff.CASES, ids=ff.CASE_IDS)
GUARD = 4099


def _assert_boxes_equal(got, refs, plan, what):
    """got (n, 3, h, w) on the host == refs box by box; on failure the box, its form and the first difference."""
    assert got.shape[0] == len(refs) and got.dtype == np.float32
    for i, want in enumerate(refs):
        if not np.array_equal(got[i], want):
            b = plan.boxes[i]
            form = ff.form_of(b, plan.lds_bytes)
            pytest.fail(f"{what}: box {i} (x0 {b.x0}, y0 {b.y0}, {b.cw}x{b.ch}) of form {form}: first difference "
                        f"(channel, y, x), got, want = {ff.first_difference(got[i], want)}")


def _decoded(plan):
    return ff.read_plan(plan.host, plan.n, False, plan.n_blocks, plan.lds_bytes)


@CASE
def test_crop_resize_equals_pillow(built_lib, case):
    from probpose_pytorch_amd import frontend
    frame = torch.from_numpy(ff.case_frame(case.id, 0).copy()).cuda()
    plan = frontend.FrontendPlan(frontend.round_boxes(case.boxes()), case.out, frame.device)
    got = frontend.crop_resize(frame, None, case.out, plan=plan)
    assert torch.equal(got, frontend.crop_resize(frame, case.boxes(), case.out))      # boxes given == plan given
    _assert_boxes_equal(got.cpu().numpy(), ff.pillow_reference(case.id), _decoded(plan), case.id)


@CASE
def test_multi_source_equals_single_frame_and_pillow(built_lib, case):
    from probpose_pytorch_amd import frontend
    boxes = frontend.round_boxes(case.boxes())
    regions = ff.case_regions(case)
    packed, sources = ff.pack(regions)
    host = np.zeros(frontend.multi_plan_bytes(boxes, case.out) // 4, dtype=np.int32)
    n_blocks, lds = frontend.multi_plan_build(boxes, sources, packed.size, case.out, host.ctypes.data)
    got = frontend.crop_resize_multi(torch.from_numpy(packed).cuda(), torch.from_numpy(host).cuda(), len(boxes),
                                     n_blocks, lds, case.out)
    single = frontend.crop_resize(torch.from_numpy(ff.case_frame(case.id, 0).copy()).cuda(), case.boxes(), case.out)
    same = torch.tensor([which == 0 for which in ff.case_region_index(case)], device=got.device)
    assert bool(same.any()) and (case.second is None) == bool(same.all())
    assert torch.equal(got[same], single[same]), case.id
    _assert_boxes_equal(got.cpu().numpy(), ff.pillow_reference(case.id, True),
                        ff.read_plan(host, len(boxes), True, n_blocks, lds), case.id + " (multi-source)")


@CASE
def test_bare_entry_writes_every_element_and_no_other(built_lib, case):
    """pp_frontend_crop_resize itself on a NaN-filled output with NaN guards on both sides."""
    from probpose_pytorch_amd import _lib, frontend
    frame = torch.from_numpy(ff.case_frame(case.id, 0).copy()).cuda()
    plan = frontend.FrontendPlan(frontend.round_boxes(case.boxes()), case.out, frame.device)
    numel = plan.n * 3 * plan.out_h * plan.out_w
    buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=torch.float32, device=frame.device)
    out = buf[GUARD:GUARD + numel]
    _lib.launch("pp_frontend_crop_resize", frame, int(frame.shape[1]), int(frame.shape[0]), int(frame.stride(0)),
                plan.dev, plan.n, plan.n_blocks, plan.lds_bytes, plan.out_w, plan.out_h, out)
    torch.cuda.synchronize()
    assert bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + numel:].isnan().all()), "a guard element was written"
    unwritten = out.isnan().nonzero()
    assert unwritten.numel() == 0, f"{unwritten.numel()} elements unwritten, the first at flat index {int(unwritten[0])}"
    _assert_boxes_equal(out.view(plan.n, 3, plan.out_h, plan.out_w).cpu().numpy(), ff.pillow_reference(case.id),
                        _decoded(plan), case.id + " (bare entry)")


def test_plan_reuse_across_frames(built_lib):
    """One FrontendPlan on two frames of different sizes; the boxes leave the smaller one."""
    from probpose_pytorch_amd import frontend
    boxes = [(-10.0, -5.0, 150.0, 120.0), (80.0, 60.0, 90.0, 100.0), (120.0, 90.0, 190.0, 200.0), (0.0, 0.0, 131.0, 97.0),
             (130.0, 96.0, 1.0, 1.0), (5.5, 6.5, 51.0, 40.0)]
    size = (48, 64)
    plan = None
    for h, w, seed in ((97, 131, 31), (240, 321, 32)):
        img = ff.frame(h, w, seed)
        dev = torch.from_numpy(img).cuda()
        if plan is None:
            plan = frontend.FrontendPlan(frontend.round_boxes(boxes), size, dev.device)
        got = frontend.crop_resize(dev, None, size, plan=plan).cpu().numpy()
        _assert_boxes_equal(got, [fo.scale_box_pil(img, b, size) for b in boxes], _decoded(plan), f"{w}x{h} frame")


def test_channel_strided_and_flipped_frames(built_lib, monkeypatch):
    from probpose_pytorch_amd import frontend
    img = ff.frame(300, 401, 33)
    dev = torch.from_numpy(img).cuda()
    size = ff.VIEW_SIZE
    boxes = ff.VIEW_BOXES                  # staged and direct; two include the last pixel of the view's last row
    plan = frontend.FrontendPlan(frontend.round_boxes(boxes), size, dev.device)

    def check(view, array, what):
        got = frontend.crop_resize(view, None, size, plan=plan).cpu().numpy()
        _assert_boxes_equal(got, [fo.scale_box_pil(array, b, size) for b in boxes], _decoded(plan), what)

    bgr = dev.flip(-1)                                                       # BGR order of the same frame
    check(bgr, np.ascontiguousarray(img[:, :, ::-1]), "BGR view")
    chw = dev.permute(2, 0, 1).contiguous().permute(1, 2, 0)                 # (H, W, 3) view of a (3, H, W) tensor:
    # crop_resize materialises it with .contiguous()
    assert chw.stride(2) != 1 and chw.shape == dev.shape
    check(chw, img, "channel-strided view")
    # a row-strided view is read in place: the left 401 columns of a 512-wide buffer, whose own last byte is the view's
    flat = torch.full(((300 - 1) * 512 * 3 + 401 * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (300, 401, 3), (512 * 3, 3, 1))
    view.copy_(dev)
    assert view.stride(0) == 1536 and view.data_ptr() == flat.data_ptr()
    seen = []
    launch = frontend._lib.launch
    monkeypatch.setattr(frontend._lib, "launch",
                        lambda name, image, *a: (seen.append(image.data_ptr()), launch(name, image, *a))[1])
    check(view, img, "row-strided view")
    assert seen == [flat.data_ptr()]                                         # no copy was made


def test_box_wholly_outside_the_frame(built_lib):
    """Left, right, above and below the 97x131 frame, staged and direct (tests/test_frontend_forms.py holds the boxes
    to those forms): Pillow's zero padding, so exactly 0.0."""
    from probpose_pytorch_amd import frontend
    img = ff.frame(97, 131, 34)
    dev = torch.from_numpy(img).cuda()
    size = ff.OUTSIDE_SIZE
    plan = frontend.FrontendPlan(frontend.round_boxes(ff.OUTSIDE_BOXES), size, dev.device)
    got = frontend.crop_resize(dev, None, size, plan=plan)
    assert got.shape == (8, 3, 32, 96)
    for i, b in enumerate(ff.OUTSIDE_BOXES):
        assert not fo.scale_box_pil(img, b, size).any(), b                   # the oracle agrees: all zeros
        assert bool((got[i] == 0).all()), (b, ff.form_of(_decoded(plan).boxes[i], plan.lds_bytes))
