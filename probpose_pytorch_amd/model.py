"""Mirror of the reference's ``probpose/model.py``."""
import torch
from torch import Tensor, nn

from . import _lib, flip, ops
from .backbone import ScratchViTBackbone
from .head import ProbMapHead


class ProbPoseModel(nn.Module):
    """Reference model.py:4-11: ``forward(x) = head(backbone(x))``.

    When both halves are the HIP-backed modules of this package the feature map
    never leaves the channels-last token layout the ViT produces (the
    reference's permute+contiguous copy, backbone.py:40, is skipped).

    ``flip_pairs`` (keyword only; the reference has no such argument) switches flip test on: in ``.eval()`` mode
    ``forward(x)`` runs the batch and its mirror image as one batch of 2B and returns the average of the two sets of
    outputs, the second un-mirrored with the left/right keypoint channels swapped (``flip.py``, csrc/pp_flip.hip).
    Flip test is an inference-time average: in ``.train()`` mode the plain forward runs whatever ``flip_pairs`` says.
    The pairs are those of ``Augment(flip_pairs=...)``; ``set_flip_test(None)`` switches it off again."""

    def __init__(self, backbone, head, *, flip_pairs=None):
        super().__init__()
        self.backbone = backbone
        self.head = head
        self.register_buffer("_flip_perm", None, persistent=False)
        if flip_pairs is not None:
            self.set_flip_test(flip_pairs)

    def set_flip_test(self, flip_pairs):
        """(i, j) keypoint index pairs that trade places under a horizontal flip, or None for the plain forward.  The
        permutation is checked against the head's keypoint count and uploaded here, once: it is a non-persistent
        buffer (it follows ``.to(device)`` and is not part of ``state_dict()``)."""
        if flip_pairs is None:
            self.register_buffer("_flip_perm", None, persistent=False)
            return self
        K = getattr(self.head, "num_keypoints", None)
        if K is None:
            K = getattr(self.head, "out_channels", None)
        if not isinstance(K, int) or K <= 0:
            raise ValueError("ProbPoseModel.set_flip_test: the head has neither num_keypoints nor out_channels to check "
                             "the flip pairs against")
        perm = torch.from_numpy(flip.flip_permutation(flip_pairs, K))
        device = next((p.device for p in self.parameters()), torch.device("cpu"))
        self.register_buffer("_flip_perm", perm.to(device), persistent=False)
        return self

    def set_compute_dtype(self, dtype: torch.dtype):
        """torch.float32 (exact-fp32 MFMA, parity mode; default), torch.bfloat16, or torch.float8_e4m3fn:
        the ViT's qkv / fc1 / fc2 GEMMs on fp8 MFMA (e4m3 weights with per-output-channel scales, e4m3
        activations with static per-tensor scales calibrated on the first batch), everything else bf16."""
        self.backbone.set_compute_dtype(dtype)
        self.head.set_compute_dtype(torch.bfloat16 if dtype == torch.float8_e4m3fn else dtype)
        return self

    def calibrate_fp8(self, batches, margin: float = None):
        """fp8 mode only: static activation scales = margin (default 1.25) x the maximum |activation| over the given
        batches / 448.  Call after set_compute_dtype(torch.float8_e4m3fn); otherwise the first forward calibrates on
        its own batch."""
        self.backbone.model.calibrate_fp8(batches, margin)
        return self

    def forward(self, x: Tensor):
        if isinstance(self.backbone, ScratchViTBackbone) and isinstance(self.head, ProbMapHead) \
                and self.head.training and self.head.differentiable and torch.is_grad_enabled() \
                and not self.backbone.differentiable \
                and any(p.requires_grad for p in self.backbone.parameters()):
            raise RuntimeError("ProbPoseModel: the HIP ScratchViTBackbone has no backward, so its parameters would get "
                               "no gradient; call model.backbone.requires_grad_(False) to train the head on a frozen "
                               "backbone, or construct it with differentiable=True")
        perm = getattr(self, "_flip_perm", None)      # getattr: whole-module pickles from before flip test have none
        if perm is not None and not self.training:
            return self._forward_flip(x, perm)
        return self._forward_plain(x)

    def _forward_flip(self, x: Tensor, perm: Tensor):
        _lib.require_device(x)
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"ProbPoseModel: flip test takes (B,C,H,W) float32 crops, got {tuple(x.shape)} {x.dtype}")
        x = x.detach().contiguous()
        x2 = torch.empty((2 * x.shape[0], *x.shape[1:]), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ops.hflip_pair(x, x2)
        return flip.flip_merge(self._forward_plain(x2), perm)

    def _forward_plain(self, x: Tensor):
        if isinstance(self.backbone, ScratchViTBackbone) and isinstance(self.head, ProbMapHead) \
                and self.backbone.model.token_dtype == self.head.compute_dtype:
            B, _, height, width = x.shape
            tokens = self.backbone.model.forward_tokens(x)
            gh, gw = self.backbone.model.patch_embed.dynamic_feat_size((height, width))
            return self.head.forward_tokens(tokens, B, gh, gw)
        return self.head(self.backbone(x))
