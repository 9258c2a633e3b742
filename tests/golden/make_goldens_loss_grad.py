"""Mint tests/golden/loss_grad.npz: the reference's own loss gradients (reference loss.py:55-143, :232-339, :360-464),
computed by torch autograd on the CPU.  cv2 is registered as an empty stub as in make_goldens_loss.py.  Run once,
from a directory outside the repository, with the path of a zir-vision/ProbPose_pytorch checkout:
    python <repo>/tests/golden/make_goldens_loss_grad.py <reference checkout>
Inputs come from the seeded generators of tests/loss_reference.py; only outputs, seeds and checksums are stored.

* ProbPoseLoss, cases G1, G2, G3, G3e of loss.npz: the gradient of each of the five losses, and of train.py's
  LOSS_WEIGHTS sum, with respect to the five predictions.  The four head gradients are stored whole.  The heatmap
  gradient (only kpt reaches it, and the weighted sum's equals kpt's) is stored for three whole maps
  (``{tag}_kpt_hm_maps``, not for G3e, whose heatmap gradient is G3's) and as per-map float64 sums of the gradient
  and of its absolute values over every map; every gradient's sha256 is kept.
* OKSHeatmapLoss over heatmap_options() x the three reductions, each with a seeded upstream gradient."""
import hashlib
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit("usage: make_goldens_loss_grad.py <path of a zir-vision/ProbPose_pytorch checkout>")
REF = os.path.abspath(sys.argv[1])

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


LR = _load("loss_reference")
LG = _load("loss_grad_reference")

sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, REF)
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
import probpose  # noqa: E402

assert all(os.path.abspath(p).startswith(REF) for p in probpose.__path__)
from probpose.codec import Codec, ProbMap  # noqa: E402
from probpose.loss import OKSHeatmapLoss, ProbPoseLoss  # noqa: E402

CASES = {"G1": ("G1", True, False, False), "G2": ("G1", False, True, True), "G3": ("G3", True, False, False),
         "G3e": ("G3", False, False, False)}
HEAD_KEYS = LG.PRED_KEYS[1:]


def hm_maps(B, K):
    """The maps stored whole: the first, the G3 map with an all-zero target, the last."""
    return sorted({0, min(K + 3, B * K - 1), B * K - 1})


def run_probpose(out, tag):
    case, freeze_error, use_kw, from_zeros = CASES[tag]
    inp = LR.case_inputs(case)
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (W, H), inp["sigmas"])), freeze_error=freeze_error)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp["gt"].items()}
    pred = tuple(torch.from_numpy(p).requires_grad_(True) for p in inp["pred"])
    kw = torch.from_numpy(inp["keypoint_weights"]) if use_kw else None
    losses = loss_fn(gt, pred, keypoint_weights=kw, learn_heatmaps_from_zeros=from_zeros)
    total = torch.sum(torch.stack([losses[k] * LG.LOSS_WEIGHTS[k] for k in LG.LOSS_WEIGHTS]))   # train.py:97-104
    maps = hm_maps(B, K)
    p = f"{tag}_"
    out[p + "hm_map_index"] = np.array(maps)
    for name, L in [*losses.items(), ("weighted", total)]:
        grads = torch.autograd.grad(L, pred, retain_graph=True, allow_unused=True)
        grads = [np.zeros(x.shape, np.float32) if g is None else g.numpy() for g, x in zip(grads, pred)]
        gh = grads[0].reshape(B * K, H, W).astype(np.float64)
        if name == "kpt":
            kpt_hm = grads[0]
            if tag != "G3e":        # G3e differs from G3 in freeze_error only: the same heatmap gradient
                out[f"{p}kpt_hm_maps"] = grads[0].reshape(B * K, H, W)[maps]
            out[f"{p}kpt_hm_sum"] = gh.sum(axis=(1, 2))
            out[f"{p}kpt_hm_abs"] = np.abs(gh).sum(axis=(1, 2))
        elif name == "weighted":
            assert np.array_equal(grads[0], kpt_hm), tag        # LOSS_WEIGHTS["kpt"] = 1
        else:
            assert not gh.any(), (tag, name)            # only the heatmap loss reaches the heatmaps
        out[f"{p}{name}_hm_sha"] = hashlib.sha256(grads[0].tobytes()).hexdigest()
        for key, g in zip(HEAD_KEYS, grads[1:]):
            out[f"{p}{name}_{key}"] = g.reshape(B, K)


def main():
    out = {}
    for tag in CASES:
        run_probpose(out, tag)
    hi = LR.heatmap_case_inputs()
    T = {k: torch.from_numpy(v) for k, v in hi.items()}
    B, K, H, W = hi["output"].shape
    for i, (ot, skip, wk, mk, sw, gw, lw) in enumerate(LR.heatmap_options()):
        m = OKSHeatmapLoss(use_target_weight=wk is not None, skip_empty_channel=skip, smoothing_weight=sw,
                           gaussian_weight=gw, loss_weight=lw, oks_type=ot)
        rng = np.random.default_rng(1000 + i)
        ups = dict(pixel=rng.normal(size=(B, K, H, W)).astype(np.float32),
                   keypoint=rng.normal(size=(B, K)).astype(np.float32), mean=np.float32(rng.normal()))
        for red, u in ups.items():
            o = T["output"].clone().requires_grad_(True)
            L = m(o, T["target"], T[wk] if wk else None, T[mk] if mk else None, per_pixel=red == "pixel",
                  per_keypoint=red == "keypoint")
            L.backward(torch.as_tensor(u))
            out[f"hm{i}_{red}_grad"] = o.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "loss_grad.npz"), upstream_seed=1000, input_sha=LR.sha(hi["output"]),
                        **out)
    print("loss_grad.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
