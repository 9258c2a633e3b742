"""The box path of inference.py with PoseNMS behind it: the command-line flags (CPU) and run_inference_on_boxes with
``nms`` against the gauge chain rescore -> nms_image on the decoded poses (GPU)."""
import numpy as np
import pytest
import torch

from tests import posenms_reference as PR


def test_parse_boxes_and_flag_errors(capsys):
    from probpose_pytorch_amd import inference
    boxes, scores = inference.parse_boxes("1,2,30,40; 5,6,7,8,0.5;")
    assert boxes.tolist() == [[1, 2, 30, 40], [5, 6, 7, 8]] and scores.tolist() == [1.0, 0.5]
    for text in ("", "1,2,3", "1,2,0,4", "1,2,3,4,5,6", "a,b,c,d"):
        with pytest.raises(ValueError):
            inference.parse_boxes(text)
    for argv, word in ((["--nms", "hard"], "--nms needs --boxes"), (["--boxes", "1,2,3"], "--boxes:"),
                       (["--boxes", "1,2,3,4", "--nms", "hard", "--nms-thr", "0"], "--nms-thr"),
                       (["--boxes", "1,2,3,4", "--nms", "harder"], "invalid choice")):
        with pytest.raises(SystemExit):
            inference.main(argv)
        assert word in capsys.readouterr().err, argv


@pytest.mark.gpu
def test_run_inference_on_boxes_with_nms_is_the_gauge_chain():
    """Five boxes: one person box given twice bit for bit and once moved by a pixel, two other boxes.  Without ``nms``
    the function returns what it always returned; with it the same three values and the NMS of the frame's poses,
    equal to the gauge's on the decoded keypoints and keypoint scores."""
    from probpose_pytorch_amd import Codec, PoseNMS, ProbMap, inference
    from probpose_pytorch_amd.synthetic import synthetic_model_state
    from tests.test_posenms_gpu import check_fixture
    model, hm_size = inference.build_model((192, 256), 17, "vit_s")
    model.load_state_dict(synthetic_model_state((256, 192), 16, 384, 12, 17, 3, (256, 256), seed=0))
    model = model.to("cuda").eval()
    sig = np.array([0.05] * 17)
    codec = Codec(ProbMap((192, 256), hm_size, sig))
    frame = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (480, 640, 3), dtype=np.uint8)).cuda()
    boxes = [(40.0, 30.0, 200.0, 380.0), (300.5, 100.25, 150.0, 300.0), (40.0, 30.0, 200.0, 380.0),
             (41.0, 30.0, 200.0, 380.0), (420.0, 60.0, 180.0, 320.0)]
    box_scores = [0.9, 0.8, 0.7, 0.95, 0.6]
    plain = inference.run_inference_on_boxes(model, codec, frame, boxes)
    assert len(plain) == 3
    nms = PoseNMS(sig, mode="hard", oks_thr=0.9, kpt_thr=0.0)
    out, preds, frame_kpts, res = inference.run_inference_on_boxes(model, codec, frame, boxes, nms=nms,
                                                                   box_scores=box_scores)
    assert torch.equal(out[0], plain[0][0]) and np.array_equal(frame_kpts, plain[2])
    assert all(np.array_equal(a, b) for a, b in zip(preds[0], plain[1][0]))
    b = np.asarray(boxes)
    scores = PR.rescore(preds[0][1], box_scores, 0.0)
    image = PR.make_image(frame_kpts, scores, b[:, 2] * b[:, 3])
    want = dict(PR.run([image], sig, "hard", 0.9), max_dets=20)
    check_fixture(dict(want, keep=np.array([True, False])), "hard", [image])     # (1) and (2); (3) is not this test's
    keep = res.keep.cpu().numpy()
    print("kept", keep, "scores", res.scores.cpu().numpy())
    assert np.array_equal(keep, want["keep"]) and res.counts.cpu().numpy().tolist() == [int(keep.sum())]
    assert res.scores.cpu().numpy().tobytes() == scores.tobytes() and res.image_ids == [0]
    first = min((0, 2), key=lambda i: -scores[i])
    assert keep[[0, 2]].sum() <= 1 and not keep[2 if first == 0 else 0]          # the twin boxes: at most the better
