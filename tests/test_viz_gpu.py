"""probpose.viz on the GPU against tests/viz_reference.py, byte for byte: the overlay at the maps' own size (both
instances of the kernel, the golden case, saturation), on special values, upsampled and on a float CHW image; colorize
with and without normalisation; discs, limbs, their order, many instances on one image and more primitives than the
LDS list holds; render; no host synchronisation and graph capture; the command line's pictures.  Guard bytes sit around
every output and the inputs must keep their bytes."""
import os

import numpy as np
import pytest
import torch

from tests import viz_reference as VR

pytestmark = pytest.mark.gpu

GUARD = 4096                          # bytes on either side of an output that must keep their value
SENTINEL = 0xA5


def _guarded(shape, offset=0):
    count = int(np.prod(shape))
    buf = torch.full((count + 2 * GUARD + offset,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + count].view(*shape)


def _guards_intact(buf, shape, offset=0):
    count, got = int(np.prod(shape)), buf.cpu().numpy()
    return (got[:GUARD + offset] == SENTINEL).all() and (got[GUARD + offset + count:] == SENTINEL).all()


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _unchanged(pairs):
    return all(d.cpu().numpy().tobytes() == np.ascontiguousarray(h).tobytes() for d, h in pairs)


def _check_overlay(viz, images, maps, name, offsets=(0, 1)):
    """Device in, device out with ``out=`` (at both alignments) and numpy in, numpy out, against the restatement."""
    lut = VR.table(name)
    want = np.stack([VR.overlay(im, hm, lut) for im, hm in zip(images, maps)])
    d_im, d_hm = _dev(images, maps)
    for offset in offsets:
        buf, out = _guarded(want.shape, offset)
        got = viz.overlay_heatmap_on_image(d_im, d_hm, name, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), (name, offset)
        assert _guards_intact(buf, want.shape, offset)
    assert _unchanged([(d_im, images), (d_hm, maps)])
    return want


# ---- overlay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 5, 7), (3, 5, 24, 20), (2, 20, 33, 65)], ids=str)
def test_overlay_same_size(built_lib, golden_dir, shape):
    """(1,3,5,7): a last group of 3 pixels; (3,5,24,20): the golden's case, dword loads and stores; (2,20,33,65): an
    odd pixel count a batch image (the byte instance), 20 overlapping maps on bright images: both saturations."""
    from probpose_pytorch_amd import viz
    B, K, H, W = shape
    for name in ("jet", "inferno"):
        if shape == VR.GOLDEN_SHAPE:
            images, maps = VR.golden_inputs(name)
        else:
            rng = np.random.default_rng(sum(shape))
            images = rng.integers(180, 256, (B, H, W, 3), dtype=np.uint8)
            images[rng.random((B, H, W)) < 0.3] = 0
            maps = rng.random(shape, dtype=np.float32)
            maps[rng.random(shape) < 0.4] *= np.float32(0.02)
        want = _check_overlay(viz, images, maps, name)
        if shape == VR.GOLDEN_SHAPE:
            assert np.array_equal(want, np.load(os.path.join(golden_dir, "viz.npz"))[name])
        if K == 20:
            assert (want == 255).mean() > 0.2 and (want < 255).any()
    # numpy in, numpy out; the unbatched form of the reference; in place
    got = viz.overlay_heatmap_on_image(images, maps, name)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(viz.overlay_heatmap_on_image(images[0], maps[0], name), want[0])
    d_im, d_hm = _dev(images, maps)
    assert viz.overlay_heatmap_on_image(d_im, d_hm, name, out=d_im) is d_im and np.array_equal(d_im.cpu().numpy(), want)


def _special_maps():
    t = np.float32(0.01)
    bins = (np.array([0, 1, 2, 3, 64, 127, 128, 129, 200, 254, 255, 256], dtype=np.float32) / np.float32(256))
    vals = np.concatenate([
        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.0, 1.5, 1e30, -0.5, -1e30, np.inf, -np.inf, np.nan, t,
                  np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], dtype=np.float32),
        bins, np.nextafter(bins, np.float32(-1)), np.nextafter(bins, np.float32(2))]).astype(np.float32)
    return vals


@pytest.mark.parametrize("name", ["jet", "inferno"])
def test_overlay_special_values(built_lib, name):
    from probpose_pytorch_amd import viz
    vals = _special_maps()
    n = vals.size
    maps = np.zeros((2, 2, 4, n), dtype=np.float32)
    maps[0, 0, :, :], maps[0, 1, 1, :] = vals, vals[::-1]          # alone, and summed with another special value
    maps[1, 1, 2, :] = vals
    images = np.random.default_rng(3).integers(0, 200, (2, 4, n, 3), dtype=np.uint8)
    want = _check_overlay(viz, images, maps, name)
    assert (want != images).any()


@pytest.mark.parametrize("sizes", [((1, 1), (3, 3)), ((4, 6), (13, 17)), ((96, 96), (97, 96)), ((8, 8), (1, 5))],
                         ids=str)
def test_overlay_upsampled(built_lib, sizes):
    """(96,96) -> (97,96): equal in one axis only, so the bilinear path with fx = 0 everywhere; (4,6) -> (13,17) also
    holds an inf and a NaN, which contaminate the pixels whose taps they are, as the formula does."""
    from probpose_pytorch_amd import viz
    (h, w), (H, W) = sizes
    rng = np.random.default_rng(h + W)
    maps = rng.random((2, 3, h, w), dtype=np.float32)
    if (h, w) == (4, 6):
        maps[0, 1, 2, 3], maps[1, 0, 0, 0], maps[1, 2, 3, 5] = np.inf, np.nan, -np.inf
    images = rng.integers(0, 128, (2, H, W, 3), dtype=np.uint8)
    want = _check_overlay(viz, images, maps, "jet")
    assert (want != images).any()


def test_overlay_float_chw_image(built_lib):
    from probpose_pytorch_amd import viz
    j = np.arange(256, dtype=np.float32)
    edges = ((j + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    vals = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2)),
                           np.array([0.0, 1.0, -1.0, 2.0, np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)])
    H, W = 3, vals.size // 3 + 1
    x = np.resize(vals, (2, 3, H, W)).astype(np.float32)
    x[1] = np.roll(x[1], 5, axis=-1)
    maps = np.random.default_rng(9).random((2, 2, H, W), dtype=np.float32) * np.float32(0.2)
    lut = VR.table("inferno")
    want = np.stack([VR.overlay(im, hm, lut) for im, hm in zip(x, maps)])
    d_x, d_hm = _dev(x, maps)
    buf, out = _guarded(want.shape)
    viz.overlay_heatmap_on_image(d_x, d_hm, "inferno", out=out)
    assert np.array_equal(out.cpu().numpy(), want) and _guards_intact(buf, want.shape)
    assert _unchanged([(d_x, x), (d_hm, maps)])
    assert np.array_equal(viz.render(d_x).cpu().numpy(), np.stack([VR.image_bytes(im) for im in x]))   # conversion alone
    assert np.array_equal(viz.overlay_heatmap_on_image(x, maps, "inferno"), want)


# ---- colorize --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 20, 96, 96)], ids=str)
def test_colorize(built_lib, shape, normalize):
    from probpose_pytorch_amd import viz
    rng = np.random.default_rng(sum(shape))
    maps = (rng.random(shape, dtype=np.float32) * np.float32(0.8)).astype(np.float32)
    flat = maps.reshape(-1, shape[-2], shape[-1])
    if flat.shape[0] >= 6:
        flat[1] = 0.0                                            # maximum 0: 0 / 0
        flat[2, -1, -1] = np.nan                                 # one NaN: the whole map when normalising
        flat[3] = 0.37                                           # all equal
        flat[4] = -flat[4]                                       # all negative
        flat[5, 0, :_special_maps().size] = _special_maps()[:shape[-1]]
    for name in ("inferno", "jet"):
        want = VR.colorize(maps, VR.table(name), normalize)
        d_maps, = _dev(maps)
        for offset in (0, 1):
            buf, out = _guarded(want.shape, offset)
            got = viz.colorize(d_maps, name, normalize, out=out)
            assert got is out and np.array_equal(got.cpu().numpy(), want), (name, offset)
            assert _guards_intact(buf, want.shape, offset)
        assert _unchanged([(d_maps, maps)])
    got = viz.colorize(maps[0], name, normalize)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want[0])
    assert viz.colorize(d_maps[:0], name, normalize).shape == (0,) + shape[1:] + (4,)


# ---- drawing ---------------------------------------------------------------------------------------------------------
def _check_draw(viz, images, kp, pr, **kw):
    want = VR.draw(images, kp, pr, **kw)
    d_im, d_kp, d_pr = _dev(images, kp, pr)
    dkw = dict(kw)
    if isinstance(dkw.get("image_index"), np.ndarray):
        dkw["image_index"] = torch.from_numpy(dkw["image_index"]).cuda()
    for offset in (0, 1):
        buf, out = _guarded(want.shape, offset)
        viz.draw_keypoints(d_im, d_kp, d_pr, out=out, **dkw)
        assert np.array_equal(out.cpu().numpy(), want), offset
        assert _guards_intact(buf, want.shape, offset)
    assert _unchanged([(d_im, images), (d_kp, kp), (d_pr, pr)])
    assert np.array_equal(viz.draw_keypoints(images, kp, pr, **kw), want)              # numpy in, host image_index
    return want


@pytest.mark.parametrize("radius", range(1, 9))
def test_draw_discs(built_lib, radius):
    from probpose_pytorch_amd import viz
    H, W, thr = 21, 30, 0.9
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (7, H - 1), (W - 1, 9), (-1, 5), (W, 5), (5, -1), (5, H),
           (-0.5, 10.2), (-1.0, 12), (W - 0.5, 14.9), (np.nan, 3), (3, np.inf), (-np.inf, 3), (3e9, 3), (3, -3e9),
           (12.9, 10.9), (15, 10), (18, 10), (21, 10)]
    kp = np.array(pts, dtype=np.float64).reshape(-1, 1, 2)
    pr = np.ones((len(pts), 1))
    pr[-3:, 0] = [thr, np.nextafter(thr, 0), np.nan]            # drawn, not drawn, drawn
    images = np.random.default_rng(radius).integers(0, 255, (1, H, W, 3), dtype=np.uint8)
    index = np.zeros(len(pts), dtype=np.int64)
    want = _check_draw(viz, images, kp, pr, threshold=thr, radius=radius, colors=(255, 0, 0), image_index=index)
    red = (want[0] == (255, 0, 0)).all(-1)
    assert red[10, 15] and red[10, 21] and red[0, 0] and red[H - 1, W - 1] and red[10, 0]
    assert radius > 2 or not red[10, 18]                         # below the threshold: only its neighbours' discs reach it
    # float32 keypoints and probabilities give the same picture (their conversion to float64 is exact)
    kp32, pr32 = np.nan_to_num(kp, nan=5.0, posinf=5.0, neginf=5.0).astype(np.float32), pr.astype(np.float32)
    _check_draw(viz, images, kp32, pr32, threshold=float(np.float32(thr)), radius=radius, image_index=index)


def test_draw_many_keypoints_and_none(built_lib):
    from probpose_pytorch_amd import viz
    rng = np.random.default_rng(133)
    H, W, K = 40, 52, 133
    images = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    kp = rng.uniform(-3, 55, (2, K, 2))
    pr = rng.uniform(0.5, 1.0, (2, K))
    colors = rng.integers(0, 256, (K, 3), dtype=np.uint8)
    want = _check_draw(viz, images, kp, pr, threshold=0.7, radius=2, colors=colors)
    assert (want != images).any()
    # N = 0: a copy of the images
    got = viz.draw_keypoints(images, np.zeros((0, K, 2)), np.zeros((0, K)), image_index=np.zeros(0, dtype=np.int64))
    assert np.array_equal(got, images)
    d_im, = _dev(images)
    got = viz.draw_keypoints(d_im, torch.zeros(0, K, 2, device="cuda"), torch.zeros(0, K, device="cuda"),
                             image_index=torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert np.array_equal(got.cpu().numpy(), images)


@pytest.mark.parametrize("width", [1, 2, 3])
def test_draw_limbs(built_lib, width):
    """Horizontal, vertical, both diagonals, a zero-length limb and one with a skipped end; two instances whose limbs
    and discs cross (limbs under discs, later over earlier), three instances on image 1 of a batch of two."""
    from probpose_pytorch_amd import viz
    H, W = 33, 47
    a = [(3, 4), (30, 4), (30, 25), (3, 25), (16, 4), (16.7, 4.2), (40, 30), (-5, 10)]
    b = [(8, 2), (8, 30), (44, 16), (2, 16), (20, 20), (20, 20), (25, 25), (26, 28)]
    c = [(10, 10), (12, 31), (44, 2), (1, 31), (0, 0), (46, 32), (22, 18), (23, 19)]
    kp = np.array([a, b, c], dtype=np.float64)
    pr = np.ones((3, 8))
    pr[2, 6] = 0.1
    skeleton = [(0, 1), (1, 2), (0, 2), (1, 3), (4, 5), (6, 7), (3, 0), (2, 6), (7, 4)]
    images = np.random.default_rng(width).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    colors = np.random.default_rng(5).integers(0, 256, (8, 3), dtype=np.uint8)
    limb_colors = np.random.default_rng(6).integers(0, 256, (len(skeleton), 3), dtype=np.uint8)
    index = np.array([1, 1, 1], dtype=np.int64)
    for lc in (None, limb_colors, (0, 0, 255)):
        want = _check_draw(viz, images, kp, pr, radius=2, colors=colors, skeleton=skeleton, limb_colors=lc,
                           line_width=width, image_index=index)
        assert np.array_equal(want[0], images[0]) and (want[1] != images[1]).any()
    for fault in ("discs_under_limbs", "r2"):
        assert not np.array_equal(VR.draw(images, kp, pr, radius=2, colors=colors, skeleton=skeleton,
                                          limb_colors=(0, 0, 255), line_width=width, image_index=index,
                                          fault=fault), want)
    # instances out of order on the images, and an image without instances
    images3 = np.concatenate([images, images[:1]])
    _check_draw(viz, images3, kp, pr, radius=3, colors=colors, skeleton=skeleton, line_width=width,
                image_index=np.array([2, 0, 2], dtype=np.int64))


@pytest.mark.parametrize("H", [1, 3])
def test_draw_longest_limb(built_lib, H):
    """An 8191-pixel limb on an 8192-wide strip: the largest products of the integer distance test."""
    from probpose_pytorch_amd import viz
    W = 8192
    images = np.zeros((1, H, W, 3), dtype=np.uint8)
    kp = np.array([[[0.0, 0.0], [W - 1.0, H - 1.0]]])
    for width in (1, 3):
        want = _check_draw(viz, images, kp, np.ones((1, 2)), radius=1, colors=(0, 255, 0), skeleton=[(0, 1)],
                           limb_colors=(255, 255, 255), line_width=width)
        white = (want[0] == 255).all(-1)
        assert white[:, 2:W - 2].any(axis=0).all() and white.sum() < 4 * W and not white[0, 0]    # the end discs are green


def test_draw_more_primitives_than_the_list_holds(built_lib):
    """10 instances of 133 keypoints on a 32 x 32 image: 1330 discs and 1320 limbs on one tile, more than the 1024
    entries of the LDS list: the list is resolved and refilled, in order, and nothing is dropped."""
    from probpose_pytorch_amd import viz
    rng = np.random.default_rng(1024)
    N, K, H, W = 10, 133, 32, 32
    kp = rng.uniform(0, 32, (N, K, 2))
    pr = np.ones((N, K))
    colors = rng.integers(0, 256, (K, 3), dtype=np.uint8)
    skeleton = [(k, k + 1) for k in range(K - 1)]
    images = np.zeros((2, H, W, 3), dtype=np.uint8)
    index = np.array([1] * N, dtype=np.int64)
    want = _check_draw(viz, images, kp, pr, radius=1, colors=colors, skeleton=skeleton, line_width=1, image_index=index)
    # the last instance's discs are on top: its centres show their own colours
    last = kp[-1].astype(np.int64)
    assert all((want[1, y, x] == colors[k]).all() for k, (x, y) in enumerate(last) if k == K - 1)
    assert not want[0].any()


def _pose_scene(B=2, K=17, H=64, W=48, h=16, w=12, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    maps = rng.random((B, K, h, w), dtype=np.float32) * np.float32(0.3)
    kp = rng.uniform(0, 1, (B + 1, K, 2)) * (W, H)
    pr = rng.uniform(0.8, 1.0, (B + 1, K))
    index = np.array([0, 1, 1][:B + 1], dtype=np.int64)
    return images, maps, kp, pr, index


def test_render_is_draw_of_overlay(built_lib):
    from probpose_pytorch_amd import viz
    images, maps, kp, pr, index = _pose_scene()
    kw = dict(threshold=0.85, radius=3, skeleton=viz.COCO17_SKELETON, line_width=2, image_index=index)
    want = VR.render(images, maps, VR.table("jet"), kp, pr, **kw)
    d_im, d_hm, d_kp, d_pr = _dev(images, maps, kp, pr)
    buf, out = _guarded(want.shape)
    viz.render(d_im, d_hm, d_kp, d_pr, out=out, **kw)
    assert np.array_equal(out.cpu().numpy(), want) and _guards_intact(buf, want.shape)
    two = viz.draw_keypoints(viz.overlay_heatmap_on_image(d_im, d_hm), d_kp, d_pr, **kw)
    assert torch.equal(two, out)
    assert np.array_equal(viz.render(images, maps, kp, pr, **kw), want)
    assert _unchanged([(d_im, images), (d_hm, maps), (d_kp, kp), (d_pr, pr)])
    assert (want != images).any() and (want != VR.overlay(images[0], maps[0], VR.table("jet"))[None]).any()


# ---- no host synchronisation, graph capture ----------------------------------------------------------------------------
def _device_calls(viz, d, outs):
    viz.overlay_heatmap_on_image(d["im"], d["hm"], "jet", out=outs[0])
    viz.colorize(d["hm"], "inferno", True, out=outs[1])
    viz.draw_keypoints(d["im"][:1].expand(3, -1, -1, -1).contiguous(), d["kp"], d["pr"], radius=3,
                       skeleton=viz.COCO17_SKELETON, out=outs[2])
    viz.render(d["im"], d["hm"], d["kp"], d["pr"], radius=3, skeleton=viz.COCO17_SKELETON, image_index=d["index"],
               out=outs[3])


def _device_scene():
    images, maps, kp, pr, index = _pose_scene(seed=4)
    lut_j, lut_i = VR.table("jet"), VR.table("inferno")
    kw = dict(radius=3, skeleton=((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7),
                                  (6, 8), (7, 9), (8, 10), (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6)))
    want = [np.stack([VR.overlay(im, hm, lut_j) for im, hm in zip(images, maps)]), VR.colorize(maps, lut_i, True),
            VR.draw(np.stack([images[0]] * 3), kp, pr, **kw), VR.render(images, maps, lut_j, kp, pr, image_index=index,
                                                                        **kw)]
    d = dict(zip(("im", "hm", "kp", "pr", "index"), _dev(images, maps, kp, pr, index)))
    return d, want


def test_device_calls_make_no_host_sync(built_lib):
    from probpose_pytorch_amd import viz
    d, want = _device_scene()
    outs = [torch.zeros(w.shape, dtype=torch.uint8, device="cuda") for w in want]
    _device_calls(viz, d, outs)                                 # the warm-up call: the colour and style tables
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _device_calls(viz, d, outs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), w)


def test_device_calls_are_capturable(built_lib):
    """One linear capture of the four calls with ``out=``, replayed twice, on new input values the second time."""
    from probpose_pytorch_amd import viz
    d, want = _device_scene()
    d["index"] = None                                           # default placement: instance n on image n
    d["kp"], d["pr"] = d["kp"][:2].contiguous(), d["pr"][:2].contiguous()
    d3 = dict(d, kp=torch.cat([d["kp"], d["kp"][:1]]), pr=torch.cat([d["pr"], d["pr"][:1]]))
    outs = [torch.zeros(w.shape, dtype=torch.uint8, device="cuda") for w in want]

    def calls():
        viz.overlay_heatmap_on_image(d["im"], d["hm"], "jet", out=outs[0])
        viz.colorize(d["hm"], "inferno", True, out=outs[1])
        viz.draw_keypoints(d["im"][:1].expand(3, -1, -1, -1).contiguous(), d3["kp"], d3["pr"], radius=3,
                           skeleton=viz.COCO17_SKELETON, out=outs[2])
        viz.render(d["im"], d["hm"], d["kp"], d["pr"], radius=3, skeleton=viz.COCO17_SKELETON, out=outs[3])

    calls()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e)
    assert np.array_equal(outs[0].cpu().numpy(), want[0]) and np.array_equal(outs[1].cpu().numpy(), want[1])
    d["hm"].mul_(0.5)                                           # the graph reads the inputs where they are
    halved = d["hm"].cpu().numpy()
    g.replay()
    torch.cuda.synchronize()
    lut = VR.table("jet")
    images = d["im"].cpu().numpy()
    assert np.array_equal(outs[0].cpu().numpy(), np.stack([VR.overlay(im, hm, lut) for im, hm in zip(images, halved)]))
    assert np.array_equal(outs[1].cpu().numpy(), VR.colorize(halved, VR.table("inferno"), True))


# ---- command line ----------------------------------------------------------------------------------------------------
def _png(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path))


def test_cli_render_single_image(built_lib, tmp_path):
    from probpose_pytorch_amd import inference, viz
    from probpose_pytorch_amd.synthetic import synthetic_crops
    preds = inference.main(["--output", str(tmp_path), "--render", "--normalize", "--render-threshold", "0.2",
                            "--input_size", "48,64", "--num_keypoints", "17"])
    x = synthetic_crops(1, 64, 48, seed=1234)
    kp, pr = np.asarray(preds[0][0], dtype=np.float64)[:1], np.asarray(preds[1], dtype=np.float64).reshape(-1, 17)[:1]
    crop = VR.image_bytes(x[0].numpy())
    want = viz.draw_keypoints(crop, kp, pr, threshold=0.2, radius=5, colors=(255, 0, 0))
    assert np.array_equal(_png(tmp_path / "output_image.png"), want)
    assert np.array_equal(want, VR.draw(crop[None], kp, pr, threshold=0.2)[0])
    print("drawn keypoints:", int((pr >= 0.2).sum()), "pixels changed:", int((want != crop).any(-1).sum()))
    # the .npy dumps stay; the PNGs are colorize of the raw maps (the dumps are normalised on the host unless max is 0)
    for i in range(17):
        assert (tmp_path / f"heatmap_{i}.npy").exists()
        rgba = _png(tmp_path / f"heatmap_{i}.png")
        assert rgba.shape == (16, 12, 4) and rgba.dtype == np.uint8
        dumped = np.load(tmp_path / f"heatmap_{i}.npy")
        if dumped.max() > 0:
            assert np.array_equal(rgba, viz.colorize(dumped, "inferno", True))
            assert np.array_equal(rgba, VR.colorize(dumped, VR.table("inferno"), True))


def test_cli_render_boxes_with_nms(built_lib, tmp_path):
    from probpose_pytorch_amd import inference, viz
    boxes = "4,6,60,80,0.9;4,6,60,80,0.7;70,10,50,90,0.8"
    out = inference.main(["--output", str(tmp_path), "--render", "--render-threshold", "0.2", "--boxes", boxes,
                          "--nms", "hard", "--input_size", "48,64", "--num_keypoints", "17"])
    keep = out[3].keep.cpu().numpy()
    assert keep.sum() < 3                                       # the twin boxes: one of the two poses is suppressed
    frame = np.random.default_rng(1234).integers(0, 256, (101, 121, 3), dtype=np.uint8)
    kp, pr = out[2][keep], np.asarray(out[1][1], dtype=np.float64).reshape(-1, 17)[keep]
    kw = dict(threshold=0.2, skeleton=viz.COCO17_SKELETON, image_index=np.zeros(int(keep.sum()), dtype=np.int64))
    want = viz.draw_keypoints(frame, kp, pr, **kw)
    assert np.array_equal(_png(tmp_path / "output_image.png"), want)
    assert np.array_equal(want, VR.draw(frame[None], kp, pr, **kw)[0])
    assert not (tmp_path / "heatmap_0.png").exists()
