"""Drop-in import path: ``probpose.model`` / ``backbone`` / ``head`` / ``codec`` /
``heatmap`` / ``util`` / ``dataset`` / ``viz`` / ``tracker`` / ``trackeval`` / ``valmeter`` / ``calibration`` resolve
to the MI355X-native implementations in ``probpose_pytorch_amd`` (same class names, constructor signatures, parameter
names and return structures as zir-vision/ProbPose_pytorch)."""
import importlib
import sys

for _name in ("model", "backbone", "head", "codec", "heatmap", "util", "inference", "frontend", "metrics", "loss",
              "dataset", "viz", "tracker", "trackeval", "valmeter", "calibration"):
    _mod = importlib.import_module("probpose_pytorch_amd." + _name)
    sys.modules[__name__ + "." + _name] = _mod
    globals()[_name] = _mod

# the reference keeps its losses and its evaluation metrics in one file, probpose/loss.py; probpose_pytorch_amd.loss
# holds the losses (loss.py:18-712) and re-exports the metrics (loss.py:715-866) from probpose_pytorch_amd.metrics

from probpose_pytorch_amd.dataset import Augment  # noqa: E402,F401  (probpose.Augment, as probpose.dataset.Augment)
from probpose_pytorch_amd.valmeter import ValidationMeter  # noqa: E402,F401
from probpose_pytorch_amd.calibration import HeadCalibration  # noqa: E402,F401
