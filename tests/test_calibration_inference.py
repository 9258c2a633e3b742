"""inference.py --calibration: the flag is parsed, a bad file is refused before the model is built, and the loaded
calibration reaches the codec (CPU: the codec is built on the host; GPU: the command line's predictions are the
calibrated ones)."""
import argparse

import numpy as np
import pytest
import torch

from tests import calibration_reference as cr
from tests import valmeter_reference as vr

ARGS = ["--input_size", "48,64", "--num_keypoints", "17"]


def saved_calibration(path, K=17, seed=5):
    """A calibration fitted by the gauge on a seeded state, saved as HeadCalibration.save writes it."""
    from probpose_pytorch_amd import HeadCalibration
    rng = np.random.default_rng(seed)
    state = vr.empty_state(K, 1)
    vr.update(state, [0.5], *vr.random_batch(rng, 256, K))
    blocks, table, row_of = cr.fit(state, K, 1, 100)
    cal = HeadCalibration(torch.from_numpy(table), torch.from_numpy(blocks), torch.from_numpy(row_of), 100)
    cal.save(path)
    return cal


def test_flag_errors(tmp_path, capsys):
    from probpose_pytorch_amd import inference
    (tmp_path / "junk.pt").write_bytes(b"not a calibration")
    saved_calibration(tmp_path / "three.pt", K=3)
    for argv, word in ((["--calibration", str(tmp_path / "none.pt")], "is not a file"),
                       (["--calibration"], "expected one argument")):
        with pytest.raises(SystemExit):
            inference.main(ARGS + argv)
        assert word in capsys.readouterr().err, argv
    # the two refusals of the codec's builder, on the host
    parser = argparse.ArgumentParser()
    for name, word in (("junk.pt", "--calibration"), ("three.pt", "holds 3 keypoints")):
        args = argparse.Namespace(calibration=tmp_path / name, num_keypoints=17, sigma=0.05)
        with pytest.raises(SystemExit):
            inference.build_codec(parser, args, (48, 64), (12, 16), device="cpu")
        assert word in capsys.readouterr().err, name


def test_the_flag_reaches_the_codec(tmp_path):
    from probpose_pytorch_amd import inference
    cal = saved_calibration(tmp_path / "cal.pt")
    parser = argparse.ArgumentParser()
    args = argparse.Namespace(calibration=tmp_path / "cal.pt", num_keypoints=17, sigma=0.05)
    codec = inference.build_codec(parser, args, (48, 64), (12, 16), device="cpu")
    got = codec.calibration
    assert got is not None and got.K == 17 and got.min_count == 100
    assert torch.equal(got.table, cal.table) and torch.equal(got.blocks, cal.blocks)
    assert torch.equal(got.row_of, cal.row_of)
    args.calibration = None
    assert inference.build_codec(parser, args, (48, 64), (12, 16), device="cpu").calibration is None


@pytest.mark.gpu
def test_command_line_predictions_are_calibrated(tmp_path, capsys):
    from probpose_pytorch_amd import inference
    cal = saved_calibration(tmp_path / "cal.pt")
    plain = inference.main(ARGS)
    calibrated = inference.main(ARGS + ["--calibration", str(tmp_path / "cal.pt")])
    capsys.readouterr()
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(plain[0], calibrated[0]))
    assert np.asarray(plain[4]).tobytes() == np.asarray(calibrated[4]).tobytes()
    aux = np.stack([np.asarray(plain[i], dtype=np.float32).reshape(-1, 17) for i in (1, 2, 3)])
    want = cr.apply(aux, cal.table.numpy(), cal.row_of.numpy())
    got = np.stack([np.asarray(calibrated[i], dtype=np.float32).reshape(-1, 17) for i in (1, 2, 3)])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not np.array_equal(got, aux)
