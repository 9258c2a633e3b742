"""``ValidationMeter``: a whole validation pass accumulated on the device and read back once.

The reference's ``train.py`` validates every 50 steps (train.py:124-168): ``loss_fn(gt, pred, compute_acc=True)`` per
batch, the five losses and five accuracies averaged on the host.  Done that way here, every batch synchronises several
times (the masks, the scalars, the PCK counts, the head tensors), and the two head accuracies are noise: loss.py:653-697
shuffles with numpy's global RNG, subsamples per batch and maximises over thresholds after the noise.

The meter keeps an integer state on the device (``pp_valmeter_update``, csrc/pp_valmeter.hip): histograms over 1024
fine bins, counts above every threshold and fixed-point sums, per head and per keypoint.  ``update`` runs the launches
``ProbPoseLoss.forward(compute_acc=True)`` runs and adds the batch without any host synchronisation; the state does not
depend on the order or the split of the batches; ``compute`` is the one synchronisation (``pp_valmeter_report`` and a
copy of a few KB).  The report holds the reference's validation numbers (train.py:146-167) and, per head and per
keypoint, what nothing else here measures: reliability tables, ECE / MCE, Brier, AUROC, the balanced accuracy at every
threshold and the best threshold, and how well the OKS head tracks the OKS the decode achieves.

``bal_acc[j]`` stands in for ``get_binary_accuracy(force_balanced=True)``.  The reference takes the smaller class whole
and subsamples the larger uniformly, so the expectation of its accuracy at one threshold is exactly
``(TP_j / n_pos + TN_j / n_neg) / 2``; its number is one noisy draw of that, maximised after the noise.

``mean_prob`` is the mean predicted probability of the whole set; train.py:145 logs the last batch's.

There is no CPU fallback: without a GPU the meter raises ``HipExtensionError``.  State layout and report fields:
include/probpose_hip.h; tests/valmeter_reference.py restates the semantics.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from . import _buffers, _lib

__all__ = ["ValidationMeter", "state_layout", "report_fields"]

BINS = _lib.PP_VALMETER_BINS
_SCALARS, _GLOBALS = 15, 18
_BINARY = ("n_pos", "n_neg", "best_bal_acc", "best_thr", "auroc", "brier", "ece", "mce", "mean_conf", "base_rate")
_OKS = ("n", "mae", "rmse", "bias", "pearson")
_ERR = ("n", "mae", "bias")
_REFERENCE = ("loss_kpt", "loss_probability", "loss_visibility", "loss_oks", "loss_error", "acc_kpt", "acc_oks",
              "acc_error")
REJECTED = ("mask", "probability", "visibility", "oks", "error")


def state_layout(K: int, J: int) -> dict:
    """name -> (word offset, shape) of every section of the state, in the header's order."""
    shapes = [("hist", (2, K, 2, BINS)), ("conf", (2, K, BINS)), ("above", (2, K, 2, J)), ("sum_p", (2, K, 2)),
              ("sum_p2", (2, K, 2)), ("oks_hist", (K, BINS)), ("oks_sx", (K, BINS)), ("oks_st", (K, BINS)),
              ("oks_sums", (K, 5)), ("err", (K, 4)), ("pck", (2, K)), ("all", (3,)), ("rejected", (5,)),
              ("scalars", (_SCALARS,))]
    out, o = {}, 0
    for name, shape in shapes:
        out[name] = (o, shape)
        o += int(np.prod(shape))
    out["words"] = (o, ())
    return out


def report_fields(J: int, E: int) -> int:
    return 2 * (len(_BINARY) + J + 3 * E) + len(_OKS) + 3 * E + len(_ERR) + 1 + _GLOBALS


def check_ece_bins(ece_bins: int) -> None:
    if ece_bins < 1 or BINS % ece_bins:
        raise ValueError(f"ece_bins must divide {BINS}, got {ece_bins}")


def head_fields(rep: np.ndarray, o: int, names, E: int, J: int = 0):
    """One head of a [K+1][F] report from column ``o``: the named scalars, ``bal_acc`` [J] where J > 0, then the
    ``reliability`` table [E][3].  Returns the dict and the column after the head."""
    d = {name: rep[:, o + i].copy() for i, name in enumerate(names)}
    o += len(names)
    if J:
        d["bal_acc"] = rep[:, o:o + J].copy()
        o += J
    d["reliability"] = rep[:, o:o + 3 * E].reshape(-1, E, 3).copy()
    return d, o + 3 * E


def parse_report(rep: np.ndarray, thresholds: np.ndarray, ece_bins: int) -> dict:
    """The [K+1][F] float64 report as a nested dict; per-row fields are arrays of K+1 (the last entry is the pool)."""
    J, E = len(thresholds), ece_bins
    out, o = {"thresholds": np.array(thresholds)}, 0
    for head in ("probability", "visibility"):
        out[head], o = head_fields(rep, o, _BINARY, E, J)
    out["oks"], o = head_fields(rep, o, _OKS, E)
    out["error"] = {name: rep[:, o + i].copy() for i, name in enumerate(_ERR)}
    o += len(_ERR)
    out["pck"] = rep[:, o].copy()
    o += 1
    g = rep[-1, o:o + _GLOBALS]
    out["reference"] = {name: float(g[i]) for i, name in enumerate(_REFERENCE)}
    out["max_heatmap"], out["mean_prob"] = float(g[8]), float(g[9])
    out["batches"], out["flagged_batches"], out["flags"] = int(g[10]), int(g[11]), int(g[12])
    out["rejected"] = {name: int(g[13 + i]) for i, name in enumerate(REJECTED)}
    return out


class ValidationMeter:
    """Whole-set validation statistics of a ``ProbPoseLoss`` model, accumulated on the device.

    ``meter.update(gt, pred)`` per batch, as ``ProbPoseLoss.forward`` takes them; ``meter.compute()`` once.  With ``gt``
    and ``pred`` on the device an update performs no host synchronisation.  A batch the loss would raise on (its flags,
    a target outside [0, 1], a non-finite loss) is counted in ``flagged_batches`` and left out of the loss means; its
    samples are counted wherever they are valid, and nothing is raised."""

    def __init__(self, loss_fn, thresholds=None, ece_bins: int = 16):
        thr = np.arange(0.1, 1.0, 0.05) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= len(thr) <= _lib.PP_VALMETER_MAX_THRESHOLDS:
            raise ValueError(f"1 to {_lib.PP_VALMETER_MAX_THRESHOLDS} thresholds, got {len(thr)}")
        check_ece_bins(ece_bins)
        self.loss_fn, self.thresholds, self.ece_bins = loss_fn, np.ascontiguousarray(thr), int(ece_bins)
        self._state = self._thr = self._K = self._device = None
        self._pinned = []           # pinned sources of the uploads that stay for the meter's life
        self._in_flight = []        # (event, operands) of the updates the stream may not have consumed yet

    # ------------------------------------------------------------------------------------------- state
    def _ensure(self, K: int, dev) -> None:
        if self._state is not None:
            if K != self._K or dev != self._device:
                raise ValueError(f"the meter holds {self._K} keypoints on {self._device}; got {K} on {dev}")
            return
        words = _lib.call("pp_valmeter_state_words", K, len(self.thresholds))
        if words < 0:
            _lib.check(int(words), "pp_valmeter_state_words")
        self._state = torch.zeros((words,), dtype=torch.int64, device=dev)
        self._thr = _buffers.upload(self.thresholds, dev, self._pinned)
        self._K, self._device = K, dev

    def device_state(self):
        """``(state, K, J)``: the int64 words on the device as ``pp_valmeter_report`` and ``pp_calib_fit`` take them."""
        if self._state is None:
            raise RuntimeError("the meter has seen no batch yet")
        return self._state, self._K, len(self.thresholds)

    @property
    def state(self) -> dict:
        """int64 device views into the state by the header's section names (``scalars``: the raw words)."""
        words, K, J = self.device_state()
        return {name: words[o:o + int(np.prod(shape))].view(shape) for name, (o, shape) in state_layout(K, J).items()
                if name != "words"}

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def _hold(self, operands) -> None:
        """Every operand stays referenced until the stream has consumed it (the rule ``metrics.pck_counts`` documents,
        without its wait): the update's operands are parked behind an event and dropped once it has completed."""
        self._in_flight = [(e, ops) for e, ops in self._in_flight if not e.query()]
        e = torch.cuda.Event()
        e.record()
        self._in_flight.append((e, operands))

    # ------------------------------------------------------------------------------------------- updates
    def _launch(self, heads, gt_oks, gt_err, masks, B, K, pck=None, map_max=None, res=None, extra=()) -> None:
        dev = heads[0].device
        self._ensure(K, dev)
        ops = [*heads, gt_oks, gt_err, *masks, pck, map_max, res, *extra]
        with torch.cuda.device(dev):
            _lib.launch("pp_valmeter_update", *heads, gt_oks, gt_err, *masks, self._thr, len(self.thresholds), pck,
                        map_max, res, B, K, self._state)
            self._hold(ops)

    def update_heads(self, prob, vis, oks, err, in_image, annotated, visibility, gt_oks, gt_err) -> None:
        """One batch of matched arrays, device tensors [B,K]: the four predictions, the three masks, the OKS and error
        targets.  No heatmaps, so no PCK, no losses and no ``max_heatmap`` from such a batch."""
        _lib.require_device(prob)
        if prob.ndim != 2:
            raise ValueError(f"update_heads takes [B,K] tensors, got {tuple(prob.shape)}")
        B, K = prob.shape
        dev = prob.device

        def as_(t, dtype, name):
            _lib.require_device(t)
            if tuple(t.shape) != (B, K):
                raise ValueError(f"{name}: expected {(B, K)}, got {tuple(t.shape)}")
            return t.detach().to(device=dev, dtype=dtype).contiguous()

        f = [as_(t, torch.float32, n) for t, n in ((prob, "prob"), (vis, "vis"), (oks, "oks"), (err, "err"),
                                                   (gt_oks, "gt_oks"), (gt_err, "gt_err"))]
        m = [as_(t, torch.int32, n) for t, n in ((in_image, "in_image"), (annotated, "annotated"),
                                                 (visibility, "visibility"))]
        if B * K == 0:
            return
        self._launch(f[:4], f[4], f[5], m, B, K)

    def _device_masks(self, gt, B, K, dev, keep) -> Tensor:
        """The three masks as one [3,B,K] int32 device tensor, the reference's ``.to(int)`` taken on the device."""
        out = []
        for key in ("in_image", "keypoints_visible", "keypoints_visibility"):
            t = gt[key]
            if not (isinstance(t, Tensor) and t.is_cuda):
                t = _buffers.upload(t, dev, keep)
            out.append(t.detach().to(device=dev).to(torch.int64).reshape(B, K).to(torch.int32))
        return torch.stack(out)

    def update(self, gt, pred, keypoint_weights=None) -> None:
        """One batch, as ``ProbPoseLoss.forward`` takes it: both decodes, ``pp_oks_heatmap_loss``,
        ``pp_probpose_loss_terms``, ``pp_heatmap_argmax`` on both stacks and ``pp_pck_counts`` -- the launches of
        ``forward(compute_acc=True)`` -- then ``pp_valmeter_update``.  Nothing comes back to the host."""
        from .metrics import _argmax_device
        loss_fn = self.loss_fn
        with torch.no_grad():
            dev, (B, K, H, W) = loss_fn._check_pred(pred)
            keep = []
            masks = self._device_masks(gt, B, K, dev, keep)
            T = loss_fn._device_terms(gt, pred, masks, keypoint_weights)
            with torch.cuda.device(dev):
                p_locs, p_vals, _ = _argmax_device(T["hm"])
                g_locs, _, _ = _argmax_device(T["gt_hm"])
                # metrics.pose_pck_accuracy(hm, gt_hm, kw > 0.5, thr=0.05) (loss.py:642-651): normalised by [H, W]
                mask = (T["kw"] > 0.5).view(torch.uint8)
                norm = _buffers.upload(np.tile(np.array([[H, W]], dtype=np.float64), (B, 1)), dev, keep)
                skip = torch.zeros((B,), dtype=torch.uint8, device=dev)
                counts = torch.empty((2, K), dtype=torch.int32, device=dev)
                _lib.launch("pp_pck_counts", p_locs, g_locs, 0, mask, norm, skip, float(np.float32(0.05)), B, K, counts,
                            None)
            self._launch(T["heads"], T["gt_oks"], T["gt_err"], list(masks), B, K, pck=counts, map_max=p_vals,
                         res=T["res"], extra=(T, p_locs, g_locs, mask, norm, skip, keep))

    # ------------------------------------------------------------------------------------------- report
    def compute(self) -> dict:
        """The one synchronisation: ``pp_valmeter_report`` and a copy of its float64 table."""
        state, K, J = self.device_state()
        E = self.ece_bins
        rep = torch.empty((K + 1, report_fields(J, E)), dtype=torch.float64, device=state.device)
        with torch.cuda.device(state.device):
            _lib.launch("pp_valmeter_report", state, self._thr, K, J, E, rep)
        host = rep.cpu().numpy()
        self._in_flight = []
        return parse_report(host, self.thresholds, E)

    @classmethod
    def run(cls, model, loader, loss_fn, **kw) -> dict:
        """A validation pass: ``model`` in eval mode under ``no_grad`` over ``loader`` (batches ``(images, gt)`` as
        ``YOLOPoseDataset.collate`` delivers them), the model's training mode restored; returns the report."""
        _lib.require_device()
        meter = cls(loss_fn, **kw)
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for images, gt in loader:
                    meter.update(gt, model(images))
        finally:
            model.train(was_training)
        return meter.compute()
