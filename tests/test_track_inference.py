"""inference.py --frames / --boxes-json / --track: the command-line flags (CPU) and a four-frame run with seeded
synthetic weights (GPU): tracks.json holds one id per box position across the frames, --render writes one picture per
frame, and a single --image without --track gives what the library's call sequence gives, as before."""
import json

import numpy as np
import pytest
import torch

ARGS = ["--input_size", "48,64", "--num_keypoints", "17"]
BOXES = [[4.0, 6.0, 40.0, 100.0, 0.9], [50.0, 20.0, 42.0, 104.0, 0.8]]


def write_frames(folder, n=4):
    """n frames of 96 x 128 (w x h): one seeded picture, a different pixel changed in a corner of each."""
    import PIL.Image
    folder.mkdir()
    base = np.random.default_rng(9).integers(0, 256, (128, 96, 3), dtype=np.uint8)
    names = []
    for f in range(n):
        im = base.copy()
        im[127, 95 - f] = 255 - im[127, 95 - f]
        names.append(f"frame_{f:03d}.png")
        PIL.Image.fromarray(im).save(folder / names[-1])
    table = {name: BOXES if f % 2 == 0 else BOXES[::-1] for f, name in enumerate(names)}     # the order alternates
    (folder.parent / "boxes.json").write_text(json.dumps(table))
    return names, folder.parent / "boxes.json"


def test_flag_errors(tmp_path, capsys):
    from probpose_pytorch_amd import inference
    names, table = write_frames(tmp_path / "frames", 1)
    frames, out = str(tmp_path / "frames"), str(tmp_path / "out")
    (tmp_path / "bad.json").write_text(json.dumps({names[0]: [[1, 2, 3]]}))
    (tmp_path / "flat.json").write_text(json.dumps({names[0]: [[1, 2, 0, 4, 0.5]]}))
    for argv, word in ((["--track"], "--track needs --frames"),
                       (["--track", "--frames", frames], "--track needs --boxes-json"),
                       (["--frames", frames, "--boxes-json", str(table)], "--frames needs --track"),
                       (["--smooth"], "--smooth needs --track"),
                       (["--track", "--frames", frames, "--boxes-json", str(table)], "--track needs --output"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--boxes",
                         "1,2,3,4"], "not --image / --boxes"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--match-thr",
                         "1"], "--match-thr"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--max-age",
                         "-1"], "--max-age"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--fps", "0"],
                        "--fps"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--smooth",
                         "1,2"], "--smooth"),
                       (["--track", "--frames", frames, "--boxes-json", str(table), "--output", out, "--smooth",
                         "0,0.1,1"], "--smooth: min_cutoff"),
                       (["--track", "--frames", frames + "x", "--boxes-json", str(table), "--output", out],
                        "is not a folder"),
                       (["--track", "--frames", frames, "--boxes-json", str(tmp_path / "bad.json"), "--output", out],
                        "--boxes-json"),
                       (["--track", "--frames", frames, "--boxes-json", str(tmp_path / "flat.json"), "--output", out],
                        "positive w, h"),
                       (["--track", "--frames", frames, "--boxes-json", str(tmp_path / "none.json"), "--output", out],
                        "--boxes-json")):
        with pytest.raises(SystemExit):
            inference.main(argv)
        assert word in capsys.readouterr().err, argv


@pytest.mark.gpu
@pytest.mark.parametrize("render", [False, True])
def test_frames_are_tracked(tmp_path, render):
    from probpose_pytorch_amd import inference
    names, table = write_frames(tmp_path / "frames")
    out = tmp_path / "out"
    argv = ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track", "--smooth", "--output",
                   str(out), "--fps", "25"]
    record = inference.main(argv + (["--render", "--render-threshold", "0.2"] if render else []))
    saved = json.loads((out / "tracks.json").read_text())
    assert saved == record and [r["frame"] for r in saved] == names
    for f, r in enumerate(saved):
        ids = [d["id"] for d in r["detections"]]
        assert ids == ([0, 1] if f % 2 == 0 else [1, 0]), (f, ids)      # one id per box position, whatever the order
        for d, box in zip(r["detections"], BOXES if f % 2 == 0 else BOXES[::-1]):
            kp = np.asarray(d["keypoints"])
            assert kp.shape == (17, 2) and np.isfinite(kp).all()
            assert (kp >= np.array(box[:2]) - 1).all() and (kp <= np.array(box[:2]) + np.array(box[2:4]) + 1).all()
    pictures = sorted(p.name for p in out.glob("*.png"))
    assert pictures == ([n.replace(".png", "_tracked.png") for n in names] if render else [])
    if render:
        import PIL.Image
        drawn = np.asarray(PIL.Image.open(out / pictures[0]))
        source = np.asarray(PIL.Image.open(tmp_path / "frames" / names[0]))
        assert drawn.shape == source.shape and (drawn != source).any()


@pytest.mark.gpu
def test_a_single_image_without_track_is_the_library_call_sequence(tmp_path, capsys):
    """--image alone: the dumps and the returned predictions are those of build_model -> load_image -> run_inference,
    byte for byte, and nothing of the tracking path appears."""
    from probpose_pytorch_amd import Codec, ProbMap, inference
    from probpose_pytorch_amd.synthetic import synthetic_model_state
    names, _ = write_frames(tmp_path / "frames", 1)
    image, out = tmp_path / "frames" / names[0], tmp_path / "out"
    preds = inference.main(ARGS + ["--image", str(image), "--output", str(out)])
    text = capsys.readouterr().out
    assert all(w in text for w in ("Input image shape: (1, 3, 64, 48)", "Predictions:", "Errors:"))
    assert sorted(p.name for p in out.iterdir()) == sorted(f"heatmap_{i}.npy" for i in range(17))
    model, hm_size = inference.build_model((48, 64), 17, "vit_s")
    model.load_state_dict(synthetic_model_state((64, 48), 16, 384, 12, 17, 3, (256, 256), seed=0))
    model = model.to("cuda").eval()
    codec = Codec(ProbMap((48, 64), hm_size, np.array([0.05] * 17)))
    output, want = inference.run_inference(model, codec, inference.load_image(image, (48, 64)).to("cuda"))
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(preds[0], want[0]))
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(preds[1:], want[1:]))
    heat = output[0][0].cpu().numpy()
    for i in range(17):
        assert np.load(out / f"heatmap_{i}.npy").tobytes() == heat[i].tobytes()
