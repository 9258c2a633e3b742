"""inference.py --propagate: the flag's errors (CPU) and a four-frame run with seeded synthetic weights and boxes for
frame 0 only (GPU): frames 1 - 3 are followed from the tracks' own boxes, the record is that of a ``PoseFollower``
driven by hand with the same model, and without the flag the same command gives the record it gave before."""
import json

import numpy as np
import pytest

from tests.test_track_inference import ARGS, BOXES, write_frames


def key_frame_only(tmp_path):
    names, table = write_frames(tmp_path / "frames")
    table.write_text(json.dumps({names[0]: BOXES}))
    return names, table


def test_flag_errors(tmp_path, capsys):
    from probpose_pytorch_amd import inference
    names, table = write_frames(tmp_path / "frames", 1)
    base = ["--track", "--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--output",
            str(tmp_path / "out")]
    for argv, word in ((["--propagate"], "--propagate needs --track"),
                       (["--propagate", "0.3,1.25,0.3", "--smooth"], "--smooth needs --track"),
                       (["--track", "--propagate", "--frames", str(tmp_path / "frames")], "--track needs --boxes-json"),
                       (base + ["--propagate", "0.3,1.25"], "--propagate: '0.3,1.25' is not vis_thr,pad,iou"),
                       (base + ["--propagate", "a,b,c"], "--propagate"),
                       (base + ["--propagate", "nan,1.25,0.3"], "--propagate: vis_thr"),
                       (base + ["--propagate", "0.3,0,0.3"], "--propagate: pad"),
                       (base + ["--propagate", "0.3,1.25,1.5"], "--propagate: iou")):
        with pytest.raises(SystemExit):
            inference.main(argv)
        assert word in capsys.readouterr().err, argv


@pytest.mark.gpu
def test_frames_are_followed_from_the_key_frame(tmp_path):
    from probpose_pytorch_amd import Codec, PoseFollower, PoseTracker, ProbMap, inference
    from probpose_pytorch_amd.synthetic import synthetic_model_state
    names, table = key_frame_only(tmp_path)
    out = tmp_path / "out"
    argv = ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track", "--output", str(out),
                   "--fps", "25"]
    record = inference.main(argv + ["--propagate", "0,1.25,0.3", "--render", "--render-threshold", "0.2"])
    assert sorted(p.name for p in out.glob("*.png")) == [n.replace(".png", "_tracked.png") for n in names]
    assert json.loads((out / "tracks.json").read_text()) == record and [r["frame"] for r in record] == names
    assert [d["source"] for d in record[0]["detections"]] == ["boxes", "boxes"]
    assert [d["box"] for d in record[0]["detections"]] == [b[:4] for b in BOXES]
    for r in record[1:]:
        assert [d["source"] for d in r["detections"]] == ["track", "track"], r["frame"]
        for d in r["detections"]:
            assert set(d) == {"id", "keypoints", "box", "source"}
            x, y, w, h = d["box"]
            assert x >= 0 and y >= 0 and x + w <= 96 and y + h <= 128 and w >= 2 and h >= 2, d["box"]
            kp = np.asarray(d["keypoints"])
            assert kp.shape == (17, 2) and np.isfinite(kp).all()
            assert (kp >= np.array([x, y]) - 1).all() and (kp <= np.array([x + w, y + h]) + 1).all()

    # the same loop by hand
    model, hm_size = inference.build_model((48, 64), 17, "vit_s")
    model.load_state_dict(synthetic_model_state((64, 48), 16, 384, 12, 17, 3, (256, 256), seed=0))
    model = model.to("cuda").eval()
    codec = Codec(ProbMap((48, 64), hm_size, np.array([0.05] * 17)))
    tracker = PoseTracker(np.array([0.05] * 17), match_thr=0.3, max_age=30, vis_thr=0.0, fps=25.0)
    follower = PoseFollower(tracker, inference.box_estimator(model, codec), pad=1.25, iou_thr=0.3)
    for f, (name, r) in enumerate(zip(names, record)):
        frame = inference.load_frame(tmp_path / "frames" / name).to("cuda")
        rows = np.asarray(BOXES if f == 0 else np.zeros((0, 5)))
        step = follower.step(frame, rows[:, :4], rows[:, 4], frame_size=(96, 128))
        assert [d["id"] for d in r["detections"]] == step.tracks.ids.cpu().numpy().tolist()
        assert [d["box"] for d in r["detections"]] == step.boxes.tolist()
        assert [d["keypoints"] for d in r["detections"]] == step.tracks.keypoints.cpu().numpy().tolist()
        assert [d["source"] for d in r["detections"]] == ["track" if s else "boxes" for s in step.source]

    # without the flag: what the command gave before, frames 1 - 3 empty
    plain = inference.main(argv[:-4] + ["--output", str(tmp_path / "plain"), "--fps", "25"])
    assert [len(r["detections"]) for r in plain] == [2, 0, 0, 0]
    assert all(set(d) == {"id", "keypoints"} for d in plain[0]["detections"])
    assert [d["id"] for d in plain[0]["detections"]] == [0, 1]
