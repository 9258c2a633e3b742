"""Mint tests/golden/loss.npz by running the reference's own losses (reference loss.py:18-712) on the CPU: the
reference has no GPU dependency on this path.  cv2 is registered as an empty stub exactly as in make_goldens.py
(imported by the reference, unused by ProbMap's decode).  Run once, from a directory outside the repository, with the
path of a zir-vision/ProbPose_pytorch checkout:
    python <repo>/tests/golden/make_goldens_loss.py <reference checkout>
Inputs come from the seeded generators of tests/loss_reference.py (numpy only); only outputs, seeds and input
checksums are stored.  The ProbPoseLoss intermediates the reference never returns (the decoded coordinates, the OKS
and error targets, the visibility weights) are recorded by wrapping the reference objects' methods from outside."""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit("usage: make_goldens_loss.py <path of a zir-vision/ProbPose_pytorch checkout>")
REF = os.path.abspath(sys.argv[1])

import numpy as np  # noqa: E402
import torch  # noqa: E402

_spec = importlib.util.spec_from_file_location("loss_reference", os.path.join(REPO, "tests", "loss_reference.py"))
LR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LR)

sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, REF)
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
import probpose  # noqa: E402

assert all(os.path.abspath(p).startswith(REF) for p in probpose.__path__)
from probpose.codec import Codec, ProbMap  # noqa: E402
from probpose.loss import BCELoss, L1LogLoss, MSELoss, OKSHeatmapLoss, ProbPoseLoss  # noqa: E402

ACC_SEED = {"G1": 1234, "G2": 99, "G3": 7, "G3e": 8}


def run_probpose(out, tag, case, freeze_error, use_kw, from_zeros):
    inp = LR.case_inputs(case)
    B, K, H, W = inp["B"], inp["K"], inp["H"], inp["W"]
    loss_fn = ProbPoseLoss(Codec(ProbMap(inp["input_size"], (W, H), inp["sigmas"])), freeze_error=freeze_error)
    rec = {"decoded": [], "vis_w": None, "gt_oks": None, "gt_err": None}
    dec = loss_fn.codec.decode_heatmap

    def decode_heatmap(h):
        r = dec(h)
        rec["decoded"].append(np.asarray(r[0]).reshape(K, 2))
        return r
    loss_fn.codec.decode_heatmap = decode_heatmap
    for mod, key, idx in ((loss_fn.visibility_loss_module, "vis_w", 2), (loss_fn.oks_loss_module, "gt_oks", 1),
                          (loss_fn.error_loss_module, "gt_err", 1)):
        def hook(m, args, key=key, idx=idx):
            rec[key] = args[idx].detach().double().numpy().copy()
        mod.register_forward_pre_hook(hook)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp["gt"].items()}
    pred = tuple(torch.from_numpy(p) for p in inp["pred"])
    kw = torch.from_numpy(inp["keypoint_weights"]) if use_kw else None
    np.random.seed(ACC_SEED[tag])
    with torch.no_grad():
        losses, accs = loss_fn(gt, pred, keypoint_weights=kw, learn_heatmaps_from_zeros=from_zeros, compute_acc=True)
    d = np.stack(rec["decoded"][: 2 * B]).reshape(B, 2, K, 2)
    p = f"{tag}_"
    out[p + "gt_kpts"], out[p + "dt_kpts"] = d[:, 0], d[:, 1]
    out[p + "gt_hm_sha"], out[p + "dt_hm_sha"] = LR.sha(inp["gt"]["heatmaps"]), LR.sha(inp["pred"][0])
    out[p + "acc_seed"] = ACC_SEED[tag]
    for k, v in losses.items():
        out[p + "loss_" + k] = np.asarray(v.double().numpy())
    for k, v in accs.items():
        out[p + "acc_" + k] = np.asarray(v.double().numpy())
        out[p + "accdtype_" + k] = str(v.dtype)
    out[p + "vis_weight"], out[p + "gt_oks"], out[p + "gt_err"] = rec["vis_w"], rec["gt_oks"], rec["gt_err"]


def main():
    out = {}
    run_probpose(out, "G1", "G1", True, False, False)
    run_probpose(out, "G2", "G1", False, True, True)
    run_probpose(out, "G3", "G3", True, False, False)
    run_probpose(out, "G3e", "G3", False, False, False)
    # OKSHeatmapLoss over every option combination and reduction
    hi = LR.heatmap_case_inputs()
    T = {k: torch.from_numpy(v) for k, v in hi.items()}
    for i, (ot, skip, wk, mk, sw, gw, lw) in enumerate(LR.heatmap_options()):
        m = OKSHeatmapLoss(use_target_weight=wk is not None, skip_empty_channel=skip, smoothing_weight=sw,
                           gaussian_weight=gw, loss_weight=lw, oks_type=ot)
        args = (T["output"], T["target"], T[wk] if wk else None, T[mk] if mk else None)
        out[f"hm{i}_pixel"] = m(*args, per_pixel=True).numpy()
        out[f"hm{i}_keypoint"] = m(*args, per_keypoint=True).numpy()
        out[f"hm{i}_mean"] = m(*args).numpy()
    # BCELoss / MSELoss / L1LogLoss
    S = LR.small_inputs()
    t = {k: torch.from_numpy(v) for k, v in S.items()}
    for sig in (True, False):
        for red in ("mean", "sum", "none"):
            for wn in ("none", "w1", "w2"):
                m = BCELoss(use_target_weight=wn != "none", reduction=red, use_sigmoid=sig, loss_weight=1.5)
                out[f"bce_{int(sig)}_{red}_{wn}"] = m(t["x"] if sig else t["logits"], t["y"],
                                                      None if wn == "none" else t[wn]).numpy()
    out["mse_w"] = MSELoss(use_target_weight=True)(t["a"], t["b"], t["wm"]).numpy()
    out["mse_now"] = MSELoss(loss_weight=0.7)(t["a"], t["b"]).numpy()
    for D in (1, 2):
        out[f"l1log_D{D}"] = L1LogLoss(use_target_weight=True)(t[f"eo{D}"], t[f"et{D}"], t[f"wl{D}"]).numpy()
        out[f"l1log_D{D}_now"] = L1LogLoss()(t[f"eo{D}"], t[f"et{D}"]).numpy()
    np.savez_compressed(os.path.join(HERE, "loss.npz"), small_seed=77, **out)
    print("loss.npz:", len(out), "arrays;", {k: v for k, v in out.items() if k.startswith("G") and "loss_" in k})


if __name__ == "__main__":
    main()
