"""TEST INFRASTRUCTURE ONLY: numpy restatement of flip test, written from its formulas, not from
csrc/pp_flip.hip or probpose_pytorch_amd/flip.py.

  pair:   out[b] = x[b];  out[B + b, c, y, u] = x[b, c, y, W - 1 - u]
  merge:  heat[b, k, y, u] = (heat2[b, k, y, u] + heat2[B + b, perm[k], y, W - 1 - u]) * 0.5
          aux[j][b, k]     = (aux2[j][b, k] + aux2[j][B + b, perm[k]]) * 0.5              j = 0 .. 3
in the dtype given (float32: one rounded add, then the exact halving; float64 for the model-level bound).

``fault`` plants a mistake in the heatmap half, for the tests that must reject one:
  "mirror_no_swap"  the mirrored pass is un-mirrored but its keypoint channels are left alone
  "swap_no_mirror"  the channels are swapped but the columns are not un-mirrored
  "no_half"         the sum is not halved
  "off_by_one"      column u is paired with W - u (the edge convention) instead of W - 1 - u
"""
from __future__ import annotations

import numpy as np


def permutation(flip_pairs, K):
    perm = list(range(K))
    for i, j in flip_pairs:
        perm[i], perm[j] = j, i
    return np.array(perm, dtype=np.int64)


def pair(x):
    x = np.asarray(x)
    return np.concatenate([x, x[..., ::-1]], axis=0)


def merge(outputs2, perm, dtype=np.float32, fault=None):
    """5 arrays at batch 2B ((2B,K,H,W) and four (2B,K,1,1)) -> 5 arrays at batch B in ``dtype``."""
    perm = np.asarray(perm, dtype=np.int64)
    heat2 = np.asarray(outputs2[0]).astype(dtype)
    B, W = heat2.shape[0] // 2, heat2.shape[-1]
    straight, second = heat2[:B], heat2[B:]
    half = dtype(0.5)
    swapped = second if fault == "mirror_no_swap" else second[:, perm]
    if fault == "swap_no_mirror":
        back = swapped
    elif fault == "off_by_one":
        cols = (W - np.arange(W)) % W                       # W - u, wrapped to stay inside the row
        back = swapped[..., cols]
    else:
        back = swapped[..., W - 1 - np.arange(W)]
    heat = straight + back
    if fault != "no_half":
        heat = heat * half
    out = [heat.astype(dtype)]
    for a in outputs2[1:]:
        a = np.asarray(a).astype(dtype)
        out.append(((a[:B] + a[B:][:, perm]) * half).astype(dtype))
    return tuple(out)


def unflip(outputs, perm):
    """The outputs of a mirrored crop, un-mirrored and swapped back (no arithmetic): what equivariance compares."""
    perm = np.asarray(perm, dtype=np.int64)
    return (np.asarray(outputs[0])[:, perm][..., ::-1],) + tuple(np.asarray(a)[:, perm] for a in outputs[1:])


def special_floats(shape, seed):
    """float32 values with -0.0, a denormal, +-inf and NaNs of two payloads among them (for bit-pattern comparisons)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    specials = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x807FFFFF],
                        dtype=np.uint32)
    n = min(flat.size, specials.size)
    flat[rng.choice(flat.size, n, replace=False)] = specials[:n]
    return x
