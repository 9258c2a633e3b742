"""Counterpart of the reference's ``probpose/inference.py`` (a ``__main__``-only CLI there).

The call sequence that defines the API contract (reference inference.py:61-112) is kept as a library
function, ``run_inference``: ``Codec(ProbMap(input_size, heatmap_size, sigmas))``, ``model(x)``,
``codec.decode(out)``; the CLI around it keeps the reference's flags.  Differences, all forced:

* weights are loaded as a ``state_dict`` with ``torch.load(..., weights_only=True)``; the reference's
  whole-module pickles (``weights_only=False``) execute code from the file and are refused unless
  ``--trust-pickle`` is given;
* ``--backbone`` defaults to the in-tree ViT: ``RadioBackbone`` needs a ``torch.hub`` download;
* the model runs in ``.eval()`` mode (the reference never calls it, i.e. runs train-mode BatchNorm);
* image I/O needs PIL; without ``--image`` a seeded synthetic crop is used;
* ``--flip-test`` averages the outputs with those of the mirrored crop (``ProbPoseModel.set_flip_test``), the way the
  accuracy of top-down estimators is usually reported; ``--flip-pairs "1-2,3-4,..."`` names the left/right keypoint
  pairs (default for 17 keypoints: COCO's 1-2, 3-4, ..., 15-16);
* ``--boxes "x,y,w,h[,score];..."`` runs the box path (``run_inference_on_boxes``) on the full-size ``--image``, and
  ``--nms {hard,soft_gaussian,soft_linear}`` / ``--nms-thr`` rescore and suppress the boxes' duplicate poses after
  decode (``posenms.PoseNMS``); both are off by default;
* ``--render`` (with ``--output``) writes the reference's pictures, made on the GPU by ``viz``: ``heatmap_{i}.png``
  (``viz.colorize`` of the first crop's maps through inferno, honouring ``--normalize``) and ``output_image.png``
  (``viz.draw_keypoints``: a red disc of radius 5 at every keypoint whose probability is at least
  ``--render-threshold``, 0.9 as in the reference; no text labels).  With ``--boxes`` the picture is the frame with
  every pose (with ``--nms``: every kept pose) at its frame coordinates, with the COCO skeleton for 17 keypoints.
  Without ``--render`` nothing changes: the ``.npy`` dumps stay;
* ``--frames DIR --boxes-json FILE --track`` runs the box path on every image file of DIR in sorted name order, as the
  frames of one video stream, with the boxes FILE gives per file name (``{name: [[x, y, w, h, score], ...]}``), and
  links the poses across the frames (``tracker.PoseTracker``; ``--match-thr``, ``--max-age``, ``--fps``; ``--smooth
  [min_cutoff,beta,d_cutoff]`` adds the One-Euro filter; ``--assign optimal`` replaces the greedy association by the
  matching of largest total weight, for at most 256 people per frame).  ``--output`` gets ``tracks.json``: per frame and kept
  detection its track id and (smoothed) keypoints; with ``--render`` also one picture per frame, drawn from those.
  ``--predict [MAX_DT]`` (with ``--smooth``) compares a pose with where its track expects it, and ``--high-thr``,
  ``--low-match-thr``, ``--birth-thr`` associate in two stages by score and gate births (``PoseTracker``'s keywords of
  the same names; off by default; a dropped pose has id -1);
* ``--propagate [VIS_THR,PAD,IOU]`` (with ``--track``) follows the people from frame to frame (``follow.PoseFollower``):
  every track proposes its person's next box from its own last pose, so FILE needs boxes for a key frame only.  A frame
  FILE names uses its boxes and the proposals that do not duplicate them (IoU <= IOU), a frame it does not name uses
  the proposals alone; each detection of ``tracks.json`` then also holds its ``"box"`` and its ``"source"``
  (``"boxes"`` or ``"track"``).  The defaults 0.3, 1.25, 0.3 are common top-down practice, not tuned on data.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from .backbone import ScratchViTBackbone
from .codec import Codec, ProbMap
from .flip import COCO17_FLIP_PAIRS, flip_permutation, parse_flip_pairs
from .head import ProbMapHead
from .model import ProbPoseModel

VARIANTS = {"vit_s": (384, 12, 12), "vit_b": (768, 12, 12), "vit_l": (1024, 24, 16), "vit_h": (1280, 32, 16)}


def default_pools(grid):
    """alt_head_kernel_sizes that reduce a (gh, gw) grid to 1x1 in three poolings (train.py:44 uses
    [(4,4),(2,2),(2,2)] for 24x24 -> here the same recipe for any grid divisible like 16x12 or 24x18)."""
    gh, gw = grid
    pools = []
    for _ in range(2):
        kh = 4 if gh % 4 == 0 and gh > 4 else (2 if gh % 2 == 0 and gh > 1 else (3 if gh % 3 == 0 and gh > 1 else 1))
        kw = 4 if gw % 4 == 0 and gw > 4 else (3 if gw % 3 == 0 and gw > 3 else (2 if gw % 2 == 0 and gw > 1 else 1))
        pools.append((kh, kw))
        gh, gw = gh // kh, gw // kw
    pools.append((gh, gw))
    return pools


def build_model(input_size, num_keypoints: int, variant: str = "vit_s", patch: int = 16):
    """input_size is [w, h] as on the reference command line; returns (model, heatmap_size [W, H])."""
    w, h = int(input_size[0]), int(input_size[1])
    C, depth, heads = VARIANTS[variant]
    grid = (h // patch, w // patch)
    backbone = ScratchViTBackbone((h, w), patch, embed_dim=C, depth=depth, num_heads=heads)
    head = ProbMapHead(C, num_keypoints, default_pools(grid), (256, 256), (4, 4), final_layer_kernel_size=1)
    return ProbPoseModel(backbone, head), (grid[1] * 4, grid[0] * 4)


def run_inference(model: ProbPoseModel, codec: Codec, image_tensor: torch.Tensor):
    """image_tensor (B,3,H,W) float32 in [0,1] on the GPU -> (raw 5-tuple, decoded predictions).
    Reference inference.py:82-107."""
    with torch.no_grad():
        output = model(image_tensor)
    return output, codec.decode(output)


def run_inference_on_boxes(model: ProbPoseModel, codec: Codec, frame: torch.Tensor, boxes_xywh, nms=None,
                           box_scores=None):
    """Whole per-frame path on the GPU: ``frame`` (H, W, 3) uint8 RGB on the device and person boxes
    [x, y, w, h] -> crops (dataset.py:71-90 semantics, frontend.crop_resize) -> forward -> decode.
    Returns (raw 5-tuple, decoded predictions, keypoints in FRAME pixels (n, K, 2) float64): the inverse of
    the keypoint rescale of dataset.py:87-89, ``kpt / input_size * box_wh + box_xy``.

    With ``nms`` (a ``posenms.PoseNMS``) a fourth value follows: the ``PoseNMSResult`` of the frame's poses, rescored
    by ``box_scores`` [n] (default: ones) times the mean confident keypoint score and suppressed by OKS, with the box
    areas w * h as the scale; the three other values are what they are without it."""
    from . import frontend
    input_size = codec.probmap.input_size
    crops = frontend.crop_resize(frame, boxes_xywh, input_size)
    output, preds = run_inference(model, codec, crops)
    b = np.asarray(boxes_xywh, dtype=np.float64).reshape(-1, 4)
    kpts = np.asarray(preds[0][0], dtype=np.float64)
    in_wh = np.asarray(input_size, dtype=np.float64)
    frame_kpts = kpts / in_wh * b[:, None, 2:4] + b[:, None, 0:2]
    if nms is None:
        return output, preds, frame_kpts
    n = b.shape[0]
    scores = np.ones(n) if box_scores is None else np.asarray(box_scores, dtype=np.float64).reshape(n)
    dev = frame.device
    result = nms(np.zeros(n, dtype=np.int64), torch.from_numpy(frame_kpts).to(dev), torch.from_numpy(scores).to(dev),
                 torch.from_numpy(b[:, 2] * b[:, 3]).to(dev),
                 kpt_scores=torch.from_numpy(np.ascontiguousarray(preds[0][1])).to(dev))
    return output, preds, frame_kpts, result


def load_image(path: Path, input_size) -> torch.Tensor:
    """Reference inference.py:74-82: RGB, LANCZOS resize to input_size [w,h], scale to [0,1]."""
    import PIL.Image
    image = PIL.Image.open(path).convert("RGB").resize(tuple(input_size), PIL.Image.LANCZOS)
    arr = np.asarray(image, dtype=np.float32) * np.float32(1.0 / 255.0)   # v2.ToDtype(float32, scale=True)
    return torch.from_numpy(arr).permute(2, 0, 1).unsqueeze(0).contiguous()


def load_weights(model: ProbPoseModel, path: Path, model_type: str, trust_pickle: bool = False):
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:  # a whole-module pickle (reference train.py:171-180)
        if not trust_pickle:
            raise RuntimeError(f"{path} is not a plain state_dict (safe loader said: {e}); whole-module pickles run "
                               "code on load -- re-save as a state_dict or pass --trust-pickle") from e
        obj = torch.load(path, map_location="cpu", weights_only=False)
    sd = obj.state_dict() if hasattr(obj, "state_dict") else obj
    target = model.head if model_type == "head" else model
    return target.load_state_dict(sd)


def resolve_flip_pairs(parser, args):
    """The flip pairs the command line asks for, or None; argument errors go through ``parser.error``."""
    if not args.flip_test:
        if args.flip_pairs is not None:
            parser.error("--flip-pairs needs --flip-test")
        return None
    if args.flip_pairs is None:
        if args.num_keypoints != 17:
            parser.error(f"--flip-test with --num_keypoints {args.num_keypoints} needs --flip-pairs (only the COCO-17 "
                         "pairs are built in)")
        return COCO17_FLIP_PAIRS
    try:
        pairs = parse_flip_pairs(args.flip_pairs)
        flip_permutation(pairs, args.num_keypoints)
    except ValueError as e:
        parser.error(f"--flip-pairs: {e}")
    return pairs


def parse_boxes(text: str):
    """"x,y,w,h[,score];..." -> (boxes [n, 4], scores [n]; a box without score gets 1)."""
    boxes, scores = [], []
    for part in text.split(";"):
        if not part.strip():
            continue
        v = [float(t) for t in part.split(",")]
        if len(v) not in (4, 5) or v[2] <= 0 or v[3] <= 0:
            raise ValueError(f"{part!r} is not x,y,w,h[,score] with positive w, h")
        boxes.append(v[:4])
        scores.append(v[4] if len(v) == 5 else 1.0)
    if not boxes:
        raise ValueError("no box given")
    return np.asarray(boxes, dtype=np.float64), np.asarray(scores, dtype=np.float64)


def load_frame(path: Path) -> torch.Tensor:
    """The image at its own size as (H, W, 3) uint8 RGB: what the box path crops from."""
    import PIL.Image
    return torch.from_numpy(np.ascontiguousarray(np.asarray(PIL.Image.open(path).convert("RGB"), dtype=np.uint8)))


def save_png(array: np.ndarray, path: Path) -> None:
    """uint8 [H, W, 3] or [H, W, 4] -> a PNG file (the one host step of --render)."""
    import PIL.Image
    PIL.Image.fromarray(array).save(path)


def build_codec(parser, args, input_size, heatmap_size, device="cuda") -> Codec:
    """The codec of the command line: ``ProbMap`` with one sigma, and the ``--calibration`` file loaded into it."""
    calibration = None
    if args.calibration is not None:
        from .calibration import HeadCalibration
        try:
            calibration = HeadCalibration.load(args.calibration, device)
        except Exception as e:      # noqa: BLE001  (whatever the file holds instead of a calibration)
            parser.error(f"--calibration: {args.calibration}: {e}")
        if calibration.K != args.num_keypoints:
            parser.error(f"--calibration: {args.calibration} holds {calibration.K} keypoints; --num_keypoints is "
                         f"{args.num_keypoints}")
    return Codec(ProbMap(input_size, heatmap_size, np.array([args.sigma] * args.num_keypoints)), calibration)


def main(argv=None):
    p = argparse.ArgumentParser(description="Inference script for ProbPose (MI355X-native path)")
    p.add_argument("--model", type=Path, default=None, help="state_dict checkpoint (omit: seeded synthetic weights)")
    p.add_argument("--model_type", type=str, default="full", choices=["head", "full"])
    p.add_argument("--image", type=Path, default=None, help="input image (omit: seeded synthetic crop)")
    p.add_argument("--output", type=Path, default=None, help="folder for heatmap .npy dumps")
    p.add_argument("--backbone", type=str, default="vit_s", choices=sorted(VARIANTS))
    p.add_argument("--input_size", type=str, default="192,256", help="w,h")
    p.add_argument("--num_keypoints", type=int, default=17)
    p.add_argument("--sigma", type=float, default=0.05, help="per-keypoint OKS sigma (inference.py:72 uses one value)")
    p.add_argument("--bf16", action="store_true", help="bf16 MFMA instead of exact-fp32 MFMA")
    p.add_argument("--normalize", action="store_true", help="divide each dumped heatmap by its maximum")
    p.add_argument("--trust-pickle", action="store_true")
    p.add_argument("--flip-test", action="store_true", help="average with the outputs of the mirrored crop")
    p.add_argument("--flip-pairs", type=str, default=None,
                   help='left/right keypoint pairs "1-2,3-4,..." (default for 17 keypoints: the COCO pairs)')
    p.add_argument("--boxes", type=str, default=None,
                   help='person boxes "x,y,w,h[,score];..." in pixels of --image at its own size: the box path')
    p.add_argument("--nms", type=str, default=None, choices=["hard", "soft_gaussian", "soft_linear"],
                   help="with --boxes: rescore the poses and suppress duplicates by OKS after decode (default: off)")
    p.add_argument("--nms-thr", type=float, default=0.9, help="OKS threshold of --nms")
    p.add_argument("--frames", type=Path, default=None,
                   help="folder of image files: the frames of one stream, in sorted name order (with --boxes-json)")
    p.add_argument("--boxes-json", type=Path, default=None,
                   help="with --frames: JSON {file name: [[x, y, w, h, score], ...]}, the person boxes of every frame")
    p.add_argument("--track", action="store_true",
                   help="with --frames: link the poses across the frames by OKS; writes tracks.json to --output")
    p.add_argument("--smooth", type=str, nargs="?", const="", default=None, metavar="MIN_CUTOFF,BETA,D_CUTOFF",
                   help="with --track: One-Euro smoothing of the tracked keypoints (no value: the defaults)")
    p.add_argument("--propagate", type=str, nargs="?", const="", default=None, metavar="VIS_THR,PAD,IOU",
                   help="with --track: crop each track's next box from its own last pose; --boxes-json then needs "
                        "boxes for key frames only (no value: 0.3,1.25,0.3)")
    p.add_argument("--match-thr", type=float, default=0.3, help="OKS a pose needs to continue a track")
    p.add_argument("--max-age", type=int, default=30, help="frames a track survives unseen")
    p.add_argument("--assign", type=str, default="greedy", choices=["greedy", "optimal"],
                   help="with --track: how poses take tracks: each in turn its best free one, or the best matching "
                        "overall (Hungarian)")
    p.add_argument("--predict", type=float, nargs="?", const=float("inf"), default=None, metavar="MAX_DT",
                   help="with --track --smooth: compare a pose with where its track's One-Euro speed expects it, "
                        "extrapolating over at most MAX_DT seconds (no value: no limit)")
    p.add_argument("--high-thr", type=float, default=None,
                   help="with --track: poses scoring at least this take tracks first; the others only continue tracks "
                        "seen in the previous frame and never start one")
    p.add_argument("--low-match-thr", type=float, default=None,
                   help="with --high-thr: OKS a pose below it needs to continue a track (default: --match-thr)")
    p.add_argument("--birth-thr", type=float, default=None,
                   help="with --track: score a pose needs to start a track (default: --high-thr)")
    p.add_argument("--fps", type=float, default=30.0, help="frame rate of --frames: the time base of --smooth")
    p.add_argument("--render", action="store_true",
                   help="with --output: also write heatmap_{i}.png and output_image.png, drawn on the GPU")
    p.add_argument("--render-threshold", type=float, default=0.9,
                   help="--render draws the keypoints whose probability is at least this")
    p.add_argument("--calibration", type=Path, default=None,
                   help="a HeadCalibration.save file: recalibrate probability, visibility and OKS in the decode")
    args = p.parse_args(argv)
    flip_pairs = resolve_flip_pairs(p, args)
    if args.calibration is not None and not args.calibration.is_file():
        p.error(f"--calibration: {args.calibration} is not a file")
    boxes = None
    if args.boxes is not None:
        try:
            boxes = parse_boxes(args.boxes)
        except ValueError as e:
            p.error(f"--boxes: {e}")
    track = _track_options(p, args)
    if args.nms is not None and boxes is None and track is None:
        p.error("--nms needs --boxes (it applies to the box path)")
    if not 0.0 < args.nms_thr <= 1.0:
        p.error(f"--nms-thr: {args.nms_thr} is outside (0, 1]")
    if args.render and args.output is None:
        p.error("--render needs --output (the folder the pictures go to)")
    if np.isnan(args.render_threshold):
        p.error("--render-threshold: not a number")
    input_size = tuple(map(int, args.input_size.split(",")))
    model, heatmap_size = build_model(input_size, args.num_keypoints, args.backbone)
    if args.model is not None:
        print("load:", load_weights(model, args.model, args.model_type, args.trust_pickle))
    else:
        from .synthetic import synthetic_model_state
        C, depth, _ = VARIANTS[args.backbone]
        model.load_state_dict(synthetic_model_state((input_size[1], input_size[0]), 16, C, depth, args.num_keypoints,
                                                    3, (256, 256), seed=0))
    model = model.to("cuda").eval()
    if args.bf16:
        model.set_compute_dtype(torch.bfloat16)
    model.set_flip_test(flip_pairs)
    codec = build_codec(p, args, input_size, heatmap_size)
    if track is not None:
        return _main_frames(args, model, codec, track)
    if boxes is not None:
        return _main_boxes(args, model, codec, boxes)
    if args.image is not None:
        x = load_image(args.image, input_size)
    else:
        from .synthetic import synthetic_crops
        x = synthetic_crops(1, input_size[1], input_size[0], seed=1234)
    print("Input image shape:", tuple(x.shape))
    x = x.to("cuda")
    output, preds = run_inference(model, codec, x)
    heatmaps = output[0][0].cpu().numpy()
    print("Output heatmap shape:", heatmaps.shape)
    if args.output is not None:
        args.output.mkdir(parents=True, exist_ok=True)
        for i, hm in enumerate(heatmaps):
            np.save(args.output / f"heatmap_{i}.npy", hm / hm.max() if args.normalize and hm.max() > 0 else hm)
        if args.render:
            from . import viz
            for i, rgba in enumerate(viz.colorize(output[0][0], "inferno", args.normalize).cpu().numpy()):
                save_png(rgba, args.output / f"heatmap_{i}.png")
            K = args.num_keypoints
            kpts = np.ascontiguousarray(np.asarray(preds[0][0], dtype=np.float64)[:1])
            probs = np.ascontiguousarray(np.asarray(preds[1], dtype=np.float64).reshape(-1, K)[:1])
            drawn = viz.render(x[:1], None, torch.from_numpy(kpts).to(x.device), torch.from_numpy(probs).to(x.device),
                               threshold=args.render_threshold)
            save_png(drawn[0].cpu().numpy(), args.output / "output_image.png")
    print("Predictions:", preds[0])
    print("Probabilities:", preds[1])
    print("Visibilities:", preds[2])
    print("OKS:", preds[3])
    print("Errors:", preds[4])
    return preds


def _main_boxes(args, model, codec, boxes):
    """The box path of the command line: full-size frame, one crop per box, optional NMS of the poses."""
    if args.image is not None:
        frame = load_frame(args.image)
    else:       # a seeded synthetic frame that holds every box
        h, w = int(np.ceil((boxes[0][:, 1] + boxes[0][:, 3]).max())) + 1, int(np.ceil((boxes[0][:, 0]
                                                                                       + boxes[0][:, 2]).max())) + 1
        frame = torch.from_numpy(np.random.default_rng(1234).integers(0, 256, (h, w, 3), dtype=np.uint8))
    print("Frame shape:", tuple(frame.shape), "boxes:", boxes[0].shape[0])
    nms = None
    if args.nms is not None:
        from .posenms import PoseNMS
        nms = PoseNMS(np.array([args.sigma] * args.num_keypoints), mode=args.nms, oks_thr=args.nms_thr)
    out = run_inference_on_boxes(model, codec, frame.to("cuda"), boxes[0], nms=nms, box_scores=boxes[1])
    print("Keypoints (frame pixels):", out[2])
    if nms is not None:
        print("Kept:", out[3].keep.cpu().numpy())
        print("Scores:", out[3].scores.cpu().numpy())
    if args.render:
        from . import viz
        K = args.num_keypoints
        shown = out[3].keep.cpu().numpy() if nms is not None else np.ones(out[2].shape[0], dtype=bool)
        kpts, probs = out[2][shown], np.asarray(out[1][1], dtype=np.float64).reshape(-1, K)[shown]
        drawn = viz.draw_keypoints(frame.numpy(), kpts, probs, threshold=args.render_threshold,
                                   skeleton=viz.COCO17_SKELETON if K == 17 else None,
                                   image_index=np.zeros(kpts.shape[0], dtype=np.int64))
        args.output.mkdir(parents=True, exist_ok=True)
        save_png(drawn, args.output / "output_image.png")
    return out


def _track_options(p, args):
    """The tracking options of the command line, checked: None without --track, else dict(files, boxes, smooth,
    propagate, stage); ``stage`` holds PoseTracker's prediction and two-stage keywords."""
    if not args.track:
        for flag, given in (("--frames", args.frames is not None), ("--boxes-json", args.boxes_json is not None),
                            ("--smooth", args.smooth is not None), ("--propagate", args.propagate is not None),
                            ("--assign", args.assign != "greedy"), ("--predict", args.predict is not None),
                            ("--high-thr", args.high_thr is not None),
                            ("--low-match-thr", args.low_match_thr is not None),
                            ("--birth-thr", args.birth_thr is not None)):
            if given:
                p.error(f"{flag} needs --track")
        return None
    if args.frames is None:
        p.error("--track needs --frames (a folder of image files)")
    if args.boxes_json is None:
        p.error("--track needs --boxes-json (the person boxes of every frame)")
    if args.image is not None or args.boxes is not None:
        p.error("--track takes its images from --frames and its boxes from --boxes-json, not --image / --boxes")
    if args.output is None:
        p.error("--track needs --output (the folder tracks.json goes to)")
    if not 0.0 <= args.match_thr < 1.0:
        p.error(f"--match-thr: {args.match_thr} is outside [0, 1)")
    if args.max_age < 0:
        p.error(f"--max-age: {args.max_age} is negative")
    if not (np.isfinite(args.fps) and args.fps > 0):
        p.error(f"--fps: {args.fps} is not a positive number")
    from .tracker import OneEuro
    smooth = None
    if args.smooth is not None:
        try:
            values = [float(v) for v in args.smooth.split(",") if v.strip()]
            if len(values) not in (0, 3):
                raise ValueError(f"{args.smooth!r} is not min_cutoff,beta,d_cutoff")
            smooth = OneEuro(*values)
        except (TypeError, ValueError) as e:
            p.error(f"--smooth: {e}")
    stage = {}
    if args.predict is not None:
        if smooth is None:
            p.error("--predict needs --smooth (the speed it moves a track by is the One-Euro filter's)")
        if not args.predict >= 0:
            p.error(f"--predict: {args.predict} is negative or not a number")
        stage.update(predict=True, predict_max_dt=None if np.isinf(args.predict) else args.predict)
    for flag, value in (("--high-thr", args.high_thr), ("--low-match-thr", args.low_match_thr),
                        ("--birth-thr", args.birth_thr)):
        if value is not None and not np.isfinite(value):
            p.error(f"{flag}: {value} is not finite")
    if args.low_match_thr is not None:
        if args.high_thr is None:
            p.error("--low-match-thr needs --high-thr")
        if not 0.0 <= args.low_match_thr < 1.0:
            p.error(f"--low-match-thr: {args.low_match_thr} is outside [0, 1)")
    stage.update(high_thr=args.high_thr, low_match_thr=args.low_match_thr, birth_thr=args.birth_thr)
    propagate = None
    if args.propagate is not None:
        try:
            values = [float(v) for v in args.propagate.split(",") if v.strip()]
            if len(values) not in (0, 3):
                raise ValueError(f"{args.propagate!r} is not vis_thr,pad,iou")
            vis_thr, pad, iou = values or (0.3, 1.25, 0.3)
            if not np.isfinite(vis_thr):
                raise ValueError(f"vis_thr: {vis_thr} is not finite")
            if not (np.isfinite(pad) and pad > 0):
                raise ValueError(f"pad: {pad} is not a positive number")
            if not 0.0 <= iou <= 1.0:
                raise ValueError(f"iou: {iou} is outside [0, 1]")
            propagate = (vis_thr, pad, iou)
        except ValueError as e:
            p.error(f"--propagate: {e}")
    if not args.frames.is_dir():
        p.error(f"--frames: {args.frames} is not a folder")
    files = sorted(f for f in args.frames.iterdir() if f.is_file())
    if not files:
        p.error(f"--frames: {args.frames} holds no file")
    try:
        table = json.loads(args.boxes_json.read_text())
        boxes = {}
        for f in files:
            rows = np.asarray(table.get(f.name, []), dtype=np.float64).reshape(-1, 5)
            if rows.size and (rows[:, 2:4] <= 0).any():
                raise ValueError(f"{f.name}: a box without positive w, h")
            boxes[f.name] = rows
    except (OSError, ValueError, AttributeError) as e:
        p.error(f"--boxes-json: {e}")
    return dict(files=files, boxes=boxes, smooth=smooth, propagate=propagate, stage=stage)


def _main_frames(args, model, codec, track):
    """--frames / --track: the box path on every frame, the tracker behind it; tracks.json and, with --render, one
    picture per frame."""
    from .tracker import PoseTracker
    K, dev = args.num_keypoints, "cuda"
    sigmas = np.array([args.sigma] * K)
    nms = None
    if args.nms is not None:
        from .posenms import PoseNMS
        nms = PoseNMS(sigmas, mode=args.nms, oks_thr=args.nms_thr)
    if track["propagate"] is not None:
        return _main_follow(args, model, codec, track, nms)
    tracker = PoseTracker(sigmas, match_thr=args.match_thr, max_age=args.max_age, smooth=track["smooth"], fps=args.fps,
                          assign=args.assign, **track["stage"])
    args.output.mkdir(parents=True, exist_ok=True)
    record = []
    for path in track["files"]:
        frame, rows = load_frame(path), track["boxes"][path.name]
        n = rows.shape[0]
        kpts, probs = torch.zeros((0, K, 2), dtype=torch.float64, device=dev), np.zeros((0, K))
        areas = scores = torch.zeros(0, dtype=torch.float64, device=dev)
        if n:
            out = run_inference_on_boxes(model, codec, frame.to(dev), rows[:, :4], nms=nms, box_scores=rows[:, 4])
            kept = out[3].keep.cpu().numpy() if nms is not None else np.ones(n, dtype=bool)
            kpts = torch.from_numpy(out[2][kept]).to(dev)
            areas = torch.from_numpy((rows[:, 2] * rows[:, 3])[kept]).to(dev)
            scores = out[3].scores[out[3].keep] if nms is not None else torch.from_numpy(rows[:, 4]).to(dev)
            probs = np.asarray(out[1][1], dtype=np.float64).reshape(-1, K)[kept]
        res = tracker.update(kpts, areas, scores)
        ids, smoothed = res.ids.cpu().numpy(), res.keypoints.cpu().numpy()
        record.append(dict(frame=path.name, detections=[dict(id=int(i), keypoints=k.tolist())
                                                        for i, k in zip(ids, smoothed)]))
        print(f"{path.name}: ids {ids.tolist()}")
        if args.render:
            from . import viz
            drawn = viz.draw_keypoints(frame.numpy(), smoothed, probs, threshold=args.render_threshold,
                                       skeleton=viz.COCO17_SKELETON if K == 17 else None,
                                       image_index=np.zeros(smoothed.shape[0], dtype=np.int64))
            save_png(drawn, args.output / f"{path.stem}_tracked.png")
    (args.output / "tracks.json").write_text(json.dumps(record))
    return record


def box_estimator(model, codec):
    """The ``estimate`` of a ``follow.PoseFollower``: ``run_inference_on_boxes`` on a (H, W, 3) uint8 device frame,
    giving the keypoints in frame pixels and their scores as device tensors."""
    def estimate(frame, boxes):
        _, preds, frame_kpts = run_inference_on_boxes(model, codec, frame, boxes)
        scores = np.ascontiguousarray(preds[0][1], dtype=np.float64)
        return torch.from_numpy(frame_kpts).to(frame.device), torch.from_numpy(scores).to(frame.device)
    return estimate


def _main_follow(args, model, codec, track, nms):
    """--propagate: the frames through a PoseFollower; the record also says which box every detection was cropped by
    and where that box came from."""
    from .follow import PoseFollower
    from .tracker import PoseTracker
    K, dev = args.num_keypoints, "cuda"
    vis_thr, pad, iou = track["propagate"]
    tracker = PoseTracker(np.array([args.sigma] * K), match_thr=args.match_thr, max_age=args.max_age, vis_thr=vis_thr,
                          smooth=track["smooth"], fps=args.fps, assign=args.assign, **track["stage"])
    follower = PoseFollower(tracker, box_estimator(model, codec), nms=nms, pad=pad, iou_thr=iou)
    args.output.mkdir(parents=True, exist_ok=True)
    record = []
    for path in track["files"]:
        frame, rows = load_frame(path), track["boxes"][path.name]
        step = follower.step(frame.to(dev), rows[:, :4], rows[:, 4], frame_size=(frame.shape[1], frame.shape[0]))
        ids, smoothed = step.tracks.ids.cpu().numpy(), step.tracks.keypoints.cpu().numpy()
        record.append(dict(frame=path.name, detections=[
            dict(id=int(i), keypoints=k.tolist(), box=b.tolist(), source="track" if s else "boxes")
            for i, k, b, s in zip(ids, smoothed, step.boxes, step.source)]))
        print(f"{path.name}: ids {ids.tolist()} from {['track' if s else 'boxes' for s in step.source]}")
        if args.render:
            from . import viz
            drawn = viz.draw_keypoints(frame.numpy(), smoothed, step.kpt_scores.cpu().numpy(),
                                       threshold=args.render_threshold,
                                       skeleton=viz.COCO17_SKELETON if K == 17 else None,
                                       image_index=np.zeros(smoothed.shape[0], dtype=np.int64))
            save_png(drawn, args.output / f"{path.stem}_tracked.png")
    (args.output / "tracks.json").write_text(json.dumps(record))
    return record


if __name__ == "__main__":
    main()
