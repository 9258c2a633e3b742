"""Flip test at inference: the average of a crop's outputs and the un-mirrored outputs of its mirror image.

``ProbPoseModel(backbone, head, flip_pairs=...)`` runs, in ``.eval()`` mode, ``ops.hflip_pair`` (the batch and its
mirror image as one batch of 2B), the ordinary forward at 2B, and ``flip_merge`` below (csrc/pp_flip.hip): two
launches around an unchanged forward, no host synchronisation.  The counterpart of ``Augment(flip_pairs=...)`` on the
training side; both build their permutation with ``pair_permutation``.

Convention: the merge mirrors heatmap column ``u`` to ``W - 1 - u``.  Under the codecs' ``scale_factor = (input - 1) /
(heatmap - 1)`` that is the exact mirror of flipping the input by pixel index (``x.flip(-1)``), so there is no
"shift heatmap" step.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

COCO17_FLIP_PAIRS = tuple((i, i + 1) for i in range(1, 17, 2))       # (1, 2), (3, 4), ..., (15, 16)


def pair_permutation(flip_pairs: Sequence[Tuple[int, int]], K: int, who: str) -> np.ndarray:
    """int32 [K]: ``perm[i], perm[j] = j, i`` for every pair, the identity elsewhere.  ``who`` starts the messages."""
    perm = np.arange(K, dtype=np.int32)
    seen = set()
    for i, j in flip_pairs:
        if not (0 <= i < K and 0 <= j < K):
            raise ValueError(f"{who}: flip pair ({i}, {j}) with {K} keypoints")
        if i == j or i in seen or j in seen:
            raise ValueError(f"{who}: flip pair ({i}, {j}) repeats a keypoint index")
        seen.update((i, j))
        perm[i], perm[j] = j, i
    return perm


def flip_permutation(flip_pairs: Sequence[Tuple[int, int]], K: int) -> np.ndarray:
    """int32 [K], an involution: the keypoint channel of the mirrored pass that output channel k averages with.
    Raises ValueError on an index outside 0..K-1, on pairs that share an index and on a pair (i, i)."""
    return pair_permutation([(int(i), int(j)) for i, j in flip_pairs], int(K), "flip_permutation")


def parse_flip_pairs(text: str):
    """``"1-2,3-4"`` -> ``((1, 2), (3, 4))`` (the CLI's --flip-pairs)."""
    pairs = []
    for item in text.split(","):
        a, sep, b = item.strip().partition("-")
        if not sep or not a.strip().isdigit() or not b.strip().isdigit():
            raise ValueError(f"flip pairs are written i-j,i-j,...; got {item.strip()!r}")
        pairs.append((int(a), int(b)))
    return tuple(pairs)


def _packed_aux(aux, B2: int, K: int):
    """The four (2B,K,1,1) tensors as one [4,2B,K] float32 buffer: the HeadPlan's own buffer where they are views of
    one (no copy), else one small copy."""
    n = B2 * K
    for t in aux:
        if tuple(t.shape) != (B2, K, 1, 1):
            raise ValueError(f"flip_merge: an auxiliary output of shape {tuple(t.shape)}; expected {(B2, K, 1, 1)}")
        if t.dtype != torch.float32:
            raise _lib.HipExtensionError(f"flip_merge: auxiliary outputs must be float32, got {t.dtype}")
        _lib.require_device(t)
    store = aux[0].untyped_storage().data_ptr()
    if all(t.is_contiguous() and t.untyped_storage().data_ptr() == store
           and t.data_ptr() == aux[0].data_ptr() + 4 * n * j for j, t in enumerate(aux)):
        return aux[0].as_strided((4, B2, K), (n, K, 1))
    packed = torch.empty((4, B2, K), dtype=torch.float32, device=aux[0].device)
    torch.stack([t.reshape(B2, K) for t in aux], out=packed)
    return packed


def flip_merge(outputs2, perm: torch.Tensor):
    """The head's 5-tuple at batch 2B (crops, then their mirror images) -> the 5-tuple at batch B:
    ``(heat2[b, k, y, u] + heat2[B + b, perm[k], y, W - 1 - u]) * 0.5`` and the same average, without the mirror, for
    probability, visibility, oks and error.  Shapes and dtypes as the head returns them: (B,K,H,W) and four (B,K,1,1),
    float32.  ``perm``: int32 [K] on the device, from ``flip_permutation``."""
    if len(outputs2) != 5:
        raise ValueError(f"flip_merge: expected the head's 5 outputs, got {len(outputs2)}")
    heat2, aux = outputs2[0], tuple(outputs2[1:])
    _lib.require_device(heat2)
    if heat2.dtype != torch.float32:
        raise _lib.HipExtensionError(f"flip_merge: heatmaps must be float32, got {heat2.dtype}")
    if heat2.dim() != 4 or heat2.shape[0] % 2 or heat2.shape[0] == 0:
        raise ValueError(f"flip_merge: heatmaps of shape {tuple(heat2.shape)}; expected (2B,K,H,W)")
    if not heat2.is_contiguous():
        raise ValueError("flip_merge: heatmaps must be contiguous")
    B2, K, H, W = heat2.shape
    if perm.dtype != torch.int32 or tuple(perm.shape) != (K,) or perm.device != heat2.device \
            or not perm.is_contiguous():
        raise ValueError(f"flip_merge: perm must be a contiguous int32 [{K}] tensor on {heat2.device}; got "
                         f"{perm.dtype} {tuple(perm.shape)} on {perm.device}")
    aux2 = _packed_aux(aux, B2, K)
    B = B2 // 2
    heat = torch.empty((B, K, H, W), dtype=torch.float32, device=heat2.device)
    out = torch.empty((4, B, K), dtype=torch.float32, device=heat2.device)
    with torch.cuda.device(heat2.device):
        ops.flip_merge(heat2.detach(), aux2.detach(), perm, heat, out)
    return (heat, out[0].reshape(B, K, 1, 1), out[1].reshape(B, K, 1, 1), out[2].reshape(B, K, 1, 1),
            out[3].reshape(B, K, 1, 1))
