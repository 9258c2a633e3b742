"""CPU tests of probpose.viz: the numpy restatement (tests/viz_reference.py) is pinned on the reference's
overlay_heatmap_on_image (tests/golden/viz.npz), on the installed matplotlib and on PIL; it rejects a planted fault of
each kind; the committed colour tables are matplotlib's; argument errors of the module raise without a device."""
import os

import numpy as np
import pytest

from tests import viz_reference as VR


@pytest.mark.parametrize("name", ["jet", "inferno"])
def test_restatement_equals_the_reference(golden_dir, name):
    gold = np.load(os.path.join(golden_dir, "viz.npz"))
    assert int(gold["seed"]) == VR.GOLDEN_SEED
    images, maps = VR.golden_inputs(name)
    lut = VR.table(name)
    got = np.stack([VR.overlay(im, hm, lut) for im, hm in zip(images, maps)])
    assert got.dtype == np.uint8 and np.array_equal(got, gold[name])
    assert (got != images).mean() > 0.3                          # the overlay is visible: not a copy of the image


def _special_values():
    rng = np.random.default_rng(7)
    bins = np.arange(0, 257, dtype=np.float32) / np.float32(256)
    v = np.concatenate([bins, np.nextafter(bins, np.float32(-1)), np.nextafter(bins, np.float32(2)),
                        rng.random(4096, dtype=np.float32) * np.float32(1.2) - np.float32(0.1),
                        np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, 1.5, -0.5, np.inf, -np.inf, np.nan, 0.01],
                                 dtype=np.float32)])
    return v.reshape(-1, 1)


@pytest.mark.parametrize("name", ["jet", "inferno"])
def test_colour_rule_and_tables_equal_matplotlib(name):
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps[name]
    v = _special_values()
    with np.errstate(invalid="ignore"):
        want = cmap(v)
    lut = VR.table(name)
    assert np.array_equal(VR.colours(v, lut), want[..., :3])
    assert np.array_equal(want[..., 3] == 0, np.isnan(v))        # alpha: 1, and 0 for NaN
    # the committed file is matplotlib's table, bit for bit; the package reads the same file
    from probpose_pytorch_amd import viz
    assert lut.dtype == np.float64 and lut.shape == (256, 3)
    assert np.array_equal(lut, cmap._lut[:256, :3])
    assert np.array_equal(viz.colormap_table(name), lut)
    # colorize is the reference CLI's (cm.inferno(hm) * 255).astype(np.uint8), also after hm / hm.max()
    for normalize in (False, True):
        hm = v[np.isfinite(v)][:4400].reshape(1, 400, 11) if normalize else v.reshape(2, -1, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            src = (hm / hm.max()) if normalize else hm
            assert src.dtype == np.float32
            assert np.array_equal(VR.colorize(hm, lut, normalize), (cmap(src) * 255).astype(np.uint8))


def test_colorize_normalize_edge_maps():
    lut = VR.table("inferno")
    maps = np.zeros((3, 4, 5), dtype=np.float32)                 # maximum 0: 0 / 0 = NaN everywhere
    maps[1] = 0.25                                               # all equal: everything becomes 1.0, the last row
    maps[2] = np.linspace(0, 1, 20, dtype=np.float32).reshape(4, 5)
    maps[2, 1, 1] = np.nan                                       # one NaN makes the whole map NaN
    got = VR.colorize(maps, lut, normalize=True)
    assert not got[0].any() and not got[2].any()
    assert np.array_equal(got[1], np.broadcast_to(np.append((lut[255] * 255).astype(np.uint8), 255), (4, 5, 4)))


@pytest.mark.parametrize("r", [2, 3, 5])
def test_disc_rule_equals_pil_ellipse(r):
    """dx^2 + dy^2 <= r^2 + r is what Pillow's ImageDraw.ellipse((x - r, y - r, x + r, y + r)) paints for r = 2, 3, 5
    (the reference uses 5).  For r = 1 and r = 8 the rule and Pillow 12.2 differ in 4 pixels each; that is stated here,
    not asserted, since it is Pillow's rasteriser and not a rule of this project."""
    PIL_Image = pytest.importorskip("PIL.Image")
    from PIL import ImageDraw
    H, W, x, y = 23, 27, 12, 10
    im = PIL_Image.new("RGB", (W, H))
    ImageDraw.Draw(im).ellipse((x - r, y - r, x + r, y + r), fill=(255, 0, 0))
    assert np.array_equal(np.asarray(im)[..., 0] == 255, VR.disc_mask(H, W, x, y, r))
    # through draw(), clipped at a corner
    im = PIL_Image.new("RGB", (W, H))
    ImageDraw.Draw(im).ellipse((-r, H - 1 - r, r, H - 1 + r), fill=(255, 0, 0))
    got = VR.draw(np.zeros((1, H, W, 3), np.uint8), [[[0.9, H - 0.5]]], [[1.0]], radius=r)
    assert np.array_equal(got[0], np.asarray(im))


def _fault_scene():
    rng = np.random.default_rng(11)
    image = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
    heat = rng.random((6, 12, 16), dtype=np.float32)
    heat[2, 3, 3] = VR.THRESHOLD
    heat[:2, 3, 3] = 0.0
    heat[3:, 3, 3] = 0.0
    return image, heat


@pytest.mark.parametrize("fault", ["descending_k", "le_threshold", "wrap"])
def test_overlay_planted_faults_are_seen(fault):
    image, heat = _fault_scene()
    lut = VR.table("jet")
    if fault == "descending_k":
        # a table on which the order of the float64 sum reaches a byte: a = the double below 1, b = c = 2^-55 (a quarter
        # of the spacing at a).  Ascending: (a + b) + c = a, and a * 255 < 255 truncates to 254.  Descending: c + b =
        # 2^-54 is half the spacing, and a + 2^-54 ties to even, 1.0: 255.
        lut = np.zeros((256, 3))
        lut[10], lut[20] = np.nextafter(1.0, 0.0), 2.0 ** -55
        image = np.zeros((1, 1, 3), np.uint8)
        heat = np.array([10.5, 20.5, 20.5], dtype=np.float32).reshape(3, 1, 1) / np.float32(256)
        assert VR.overlay(image, heat, lut).tolist() == [[[254] * 3]]
    good, bad = VR.overlay(image, heat, lut), VR.overlay(image, heat, lut, fault=fault)
    assert not np.array_equal(good, bad)
    if fault == "le_threshold":
        assert (good != bad).any(axis=-1).sum() == 1 and (good[3, 3] != bad[3, 3]).any()


@pytest.mark.parametrize("fault", ["r2", "discs_under_limbs"])
def test_draw_planted_faults_are_seen(fault):
    image = np.zeros((1, 20, 20, 3), np.uint8)
    kp = np.array([[[4.0, 4.0], [15.0, 15.0]]])
    kw = dict(radius=3, colors=[(255, 0, 0), (0, 255, 0)], skeleton=[(0, 1)], limb_colors=(0, 0, 255), line_width=3)
    good, bad = VR.draw(image, kp, np.ones((1, 2)), **kw), VR.draw(image, kp, np.ones((1, 2)), fault=fault, **kw)
    assert not np.array_equal(good, bad)
    assert tuple(good[0, 4, 4]) == (255, 0, 0) and tuple(good[0, 10, 10]) == (0, 0, 255)


def test_limb_rule_small_cases():
    # width 1: 4 d^2 <= 1 keeps the pixels on the segment only; a zero-length limb paints nothing
    assert np.array_equal(np.argwhere(VR.limb_mask(5, 7, (1, 2), (5, 2), 1)), [[2, x] for x in range(1, 6)])
    m = VR.limb_mask(7, 7, (1, 1), (5, 5), 2)                     # width 2: distance <= 1, round caps
    assert m[1, 1] and m[0, 1] and m[1, 0] and not m[0, 0] and m[3, 4] and m[4, 3] and not m[2, 4]
    img = VR.draw(np.zeros((1, 5, 5, 3), np.uint8), [[[2.0, 2.0], [2.5, 2.9]]], [[1.0, 1.0]], radius=0,
                  skeleton=[(0, 1)], limb_colors=(0, 0, 255), line_width=3)
    assert img.sum() == 255 and tuple(img[0, 2, 2]) == (255, 0, 0)


def test_keypoint_rule_small_cases():
    H, W = 6, 8
    assert VR.centre((-0.5, 0.0), 1.0, 0.9, H, W) == (0, 0)      # int() truncates toward zero
    assert VR.centre((-1.0, 0.0), 1.0, 0.9, H, W) is None
    assert VR.centre((W - 0.5, H - 0.5), 0.9, 0.9, H, W) == (W - 1, H - 1)
    assert VR.centre((1.0, 1.0), np.nextafter(0.9, 0), 0.9, H, W) is None
    assert VR.centre((1.0, 1.0), np.nan, 0.9, H, W) == (1, 1)    # a NaN probability is not below the threshold
    for bad in (np.nan, np.inf, -np.inf, 3e9, -3e9):
        assert VR.centre((bad, 1.0), 1.0, 0.9, H, W) is None and VR.centre((1.0, bad), 1.0, 0.9, H, W) is None


def test_float_image_conversion():
    x = np.array([0.0, 1.0, -1.0, 2.0, np.nan, 0.5 / 255, 254.5 / 255], dtype=np.float32)
    x = np.stack([x, x, x]).reshape(3, 1, -1)
    assert VR.image_bytes(x)[0, :, 0].tolist()[:5] == [0, 255, 0, 255, 0]


def test_module_is_aliased():
    import probpose
    import probpose.viz
    import probpose_pytorch_amd.viz
    assert probpose.viz is probpose_pytorch_amd.viz
    assert callable(probpose.viz.overlay_heatmap_on_image)


def test_argument_validation_needs_no_device():
    import torch
    from probpose_pytorch_amd import _lib, viz
    img = np.zeros((4, 6, 3), np.uint8)
    hm = np.zeros((2, 4, 6), np.float32)
    kp, pr = np.zeros((1, 3, 2), np.float32), np.ones((1, 3), np.float32)
    V, T = ValueError, TypeError
    cases = [
        (V, lambda: viz.overlay_heatmap_on_image(img, hm, "viridis")),
        (T, lambda: viz.overlay_heatmap_on_image(img.astype(np.int64), hm)),
        (T, lambda: viz.overlay_heatmap_on_image(img, hm.astype(np.float64))),
        (V, lambda: viz.overlay_heatmap_on_image(img[..., :2], hm)),
        (V, lambda: viz.overlay_heatmap_on_image(img, hm[None])),
        (V, lambda: viz.overlay_heatmap_on_image(img[None], hm)),
        (V, lambda: viz.overlay_heatmap_on_image(np.zeros((2, 4, 6, 3), np.uint8), hm[None])),
        (V, lambda: viz.overlay_heatmap_on_image(np.zeros((1, 4, 4, 6), np.float32), hm[None])),    # not [B, 3, H, W]
        (V, lambda: viz.overlay_heatmap_on_image(np.zeros((1, 8193, 3), np.uint8), hm)),
        (V, lambda: viz.overlay_heatmap_on_image(img, np.zeros((0, 4, 6), np.float32))),
        (V, lambda: viz.overlay_heatmap_on_image(img, hm, out=torch.empty(4, 6, 3, dtype=torch.uint8))),
        (T, lambda: viz.overlay_heatmap_on_image(torch.zeros(4, 6, 3, dtype=torch.uint8), hm)),     # a host tensor
        (V, lambda: viz.colorize(hm, "viridis")),
        (T, lambda: viz.colorize(hm.astype(np.float64))),
        (V, lambda: viz.colorize(np.zeros(5, np.float32))),
        (V, lambda: viz.colorize(np.zeros((2, 0, 5), np.float32))),
        (T, lambda: viz.draw_keypoints(img.astype(np.float32), kp, pr)),
        (V, lambda: viz.draw_keypoints(img, kp[..., :1], pr)),
        (V, lambda: viz.draw_keypoints(img, kp, pr[:, :2])),
        (T, lambda: viz.draw_keypoints(img, kp.astype(np.int32), pr)),
        (V, lambda: viz.draw_keypoints(img, np.zeros((2, 3, 2), np.float32), np.ones((2, 3), np.float32))),  # N != B
        (V, lambda: viz.draw_keypoints(img, kp, pr, image_index=[1])),
        (V, lambda: viz.draw_keypoints(img, kp, pr, image_index=[0, 0])),
        (T, lambda: viz.draw_keypoints(img, kp, pr, image_index=[0.0])),
        (V, lambda: viz.draw_keypoints(img, kp, pr, threshold=float("nan"))),
        (V, lambda: viz.draw_keypoints(img, kp, pr, radius=-1)),
        (T, lambda: viz.draw_keypoints(img, kp, pr, radius=2.5)),
        (V, lambda: viz.draw_keypoints(img, kp, pr, line_width=0)),
        (V, lambda: viz.draw_keypoints(img, kp, pr, colors=(255, 0))),
        (V, lambda: viz.draw_keypoints(img, kp, pr, colors=(256, 0, 0))),
        (T, lambda: viz.draw_keypoints(img, kp, pr, colors=(1.0, 0.0, 0.0))),
        (V, lambda: viz.draw_keypoints(img, kp, pr, colors=np.zeros((2, 3), np.uint8))),
        (V, lambda: viz.draw_keypoints(img, kp, pr, skeleton=[(0, 3)])),
        (V, lambda: viz.draw_keypoints(img, kp, pr, skeleton=[(0, 1, 2)])),
        (V, lambda: viz.draw_keypoints(img, kp, pr, limb_colors=(0, 0, 255))),
        (V, lambda: viz.draw_keypoints(img, kp, pr, skeleton=[(0, 1)], limb_colors=np.zeros((2, 3), np.uint8))),
        (V, lambda: viz.draw_keypoints(np.zeros((8193, 2, 3), np.uint8), kp, pr)),
        (V, lambda: viz.render(img, hm, kp, None)),
    ]
    for i, (err, call) in enumerate(cases):
        with pytest.raises(err):
            call()
            pytest.fail(f"case {i} did not raise")
    if not torch.cuda.is_available():                            # valid arguments reach the device check: no CPU path
        for call in (lambda: viz.overlay_heatmap_on_image(img, hm), lambda: viz.colorize(hm),
                     lambda: viz.draw_keypoints(img, kp, pr, skeleton=[(0, 1)]), lambda: viz.render(img, hm, kp, pr)):
            with pytest.raises(_lib.HipExtensionError):
                call()


def test_viz_cabi_refusals(built_lib):
    """pp_viz_render / pp_viz_colorize refuse on the host before any launch."""
    L = built_lib
    P = 0x10000
    ok = dict(image=P, f32=0, out=2 * P, B=1, H=4, W=4, heat=None, K=0, h=0, w=0, lut=None, kpts=None, probs=None,
              inst=None, off=None, N=0, Kp=0, style=None, Ls=0, thr=0.9, radius=5, lw=2, stream=None)

    def render(**kw):
        return L.pp_viz_render(*{**ok, **kw}.values())

    assert render(image=None) != 0 and b"null" in L.pp_last_error()
    assert render(H=0) != 0 and b"positive" in L.pp_last_error()
    assert render(W=8193) != 0 and b"larger" in L.pp_last_error()
    assert render(out=P + 4) != 0 and b"alias" in L.pp_last_error()
    assert render(f32=1, out=P) != 0 and b"alias" in L.pp_last_error()
    assert render(heat=4 * P, K=1, h=4, w=4) != 0 and b"colour table" in L.pp_last_error()
    assert render(heat=4 * P, lut=8 * P, K=0, h=4, w=4) != 0 and b"map sizes" in L.pp_last_error()
    assert render(heat=2 * P, lut=8 * P, K=1, h=4, w=4) != 0 and b"alias" in L.pp_last_error()
    draw = dict(kpts=4 * P, probs=5 * P, inst=6 * P, off=7 * P, style=8 * P, N=1, Kp=3)
    assert render(**{**draw, "probs": None}) != 0 and b"without" in L.pp_last_error()
    assert render(**{**draw, "Kp": 0}) != 0 and b"Kp=0" in L.pp_last_error()
    assert render(**draw, thr=float("nan")) != 0 and b"threshold" in L.pp_last_error()
    assert render(**draw, radius=-1) != 0 and b"radius" in L.pp_last_error()
    assert render(**draw, lw=0) != 0 and b"line_width" in L.pp_last_error()
    assert L.pp_viz_colorize(P, 2 * P, -1, 4, 4, 3 * P, 0, None) != 0 and b"M=-1" in L.pp_last_error()
    assert L.pp_viz_colorize(P, 2 * P, 1, 0, 4, 3 * P, 0, None) != 0 and b"h=0" in L.pp_last_error()
    assert L.pp_viz_colorize(P, 2 * P, 1, 4, 4, None, 0, None) != 0 and b"null" in L.pp_last_error()
    assert L.pp_viz_colorize(P, P + 16, 1, 4, 4, 3 * P, 0, None) != 0 and b"alias" in L.pp_last_error()
    assert L.pp_viz_colorize(None, None, 0, 4, 4, None, 0, None) == 0
