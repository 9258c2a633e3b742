"""The ragged pose batch of PoseNMS, PoseTracker and CocoKeypointEval, stated once: M poses, each in one group (an
image, a stream), whose ids are host bookkeeping.  first_seen and group_layout give the layout, check_pose_batch and
device_f64 check the inputs (on_device and checked_f64 are its halves: CocoKeypointEval.add_detections takes host
arrays too), visiting_order is the two stable sorts DESIGN §4.7b, §4.7c and §4.7d promise, unsorted the way back.
Apart from checked_f64's read-back, the one of a call, nothing here waits for the device."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def host_ids(ids) -> np.ndarray:
    """Group ids as a host array; a tensor of ids is read here, once."""
    return ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)


def first_seen(ids: np.ndarray):
    """(the distinct ids in the order they first appear, every id's position in that list [M] int64)."""
    if ids.dtype != object:
        uniq, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        rank = np.empty(by_first.size, dtype=np.int64)
        rank[by_first] = np.arange(by_first.size, dtype=np.int64)
        return uniq[by_first].tolist(), rank[inverse.reshape(-1)]
    index = {}
    for i in ids.tolist():
        if i not in index:
            index[i] = len(index)
    return list(index), np.fromiter((index[i] for i in ids.tolist()), dtype=np.int64, count=ids.shape[0])


def group_layout(pos: np.ndarray, names, what: str = "", limits=()):
    """(counts [n], offsets [n + 1], int64) of the groups ``names`` (a list; their number will do without limits);
    ``pos`` [M] is every detection's group.  The fullest group above a (limit, words) of ``limits`` raises, by name."""
    n = names if isinstance(names, int) else len(names)
    counts = np.bincount(pos, minlength=n).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    for limit, words in limits:
        if n and int(counts.max()) > limit:
            worst = int(counts.argmax())
            raise ValueError(f"{what} {names[worst]!r} has {int(counts[worst])} detections, more than the {limit} "
                             f"{words}")
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    return counts, offsets


def check_pose_batch(named, K: int, M=None, vis_thr=None):
    """The shapes of ``named`` = [(name, value)]: keypoints [M, K, 2|3], two [M] vectors and, optionally, [M, K]
    values per keypoint; ``M`` None takes it from the keypoints.  ``vis_thr`` needs visibilities: that fourth entry
    or a third keypoint column.  Returns (``named`` with every value a tensor or a numpy array, M)."""
    named = [(n, a if isinstance(a, torch.Tensor) else np.asarray(a)) for n, a in named]
    shape = tuple(named[0][1].shape)
    if len(shape) != 3 or (M is not None and shape[0] != M) or shape[1] != K or shape[2] not in (2, 3):
        raise ValueError(f"{named[0][0]}: expected [{'M' if M is None else M}, {K}, 2|3] (K = len(sigmas)), got "
                         f"{shape}")
    M = shape[0]
    for (n, a), want in zip(named[1:], ((M,), (M,), (M, K))):
        if tuple(a.shape) != want:
            raise ValueError(f"{n}: expected {list(want)}, got {tuple(a.shape)}")
    if vis_thr is not None and len(named) < 4 and shape[2] != 3:
        raise ValueError("vis_thr: needs visibilities, kpt_scores or a third keypoint column")
    return named, M


def on_device(named) -> bool:
    """Whether the named inputs are device tensors: all of them or none, anything else raises."""
    dev = [isinstance(a, torch.Tensor) and a.is_cuda for _, a in named]
    if any(dev) and not all(dev):
        raise ValueError(f"{' / '.join(n for n, _ in named)}: either all device tensors or all host arrays")
    return all(dev)


FINITE = (lambda t: torch.isfinite(t).all(), "non-finite values")


def checked_f64(named, rules=None) -> list:
    """The named device tensors as contiguous float64.  One boolean per input is read back, in one copy: the one
    read-back of a call.  It is FINITE's unless ``rules`` names another (test, words) for an input."""
    out = [a.detach().to(torch.float64).contiguous() for _, a in named]
    tests = [(rules or {}).get(n, FINITE) for n, _ in named]
    passed = torch.stack([test(t) for (test, _), t in zip(tests, out)]).cpu().numpy()
    for (n, _), (_, words), ok in zip(named, tests, passed):
        if not bool(ok):
            raise ValueError(f"{n}: {words}")
    return out


def device_f64(named, names=None) -> list:
    """The named inputs (tensors or numpy arrays) as contiguous float64 device tensors.  Refuses, in this order: mixed
    placement, non-float dtypes, host arrays (under ``names``, if given; no CPU fallback) and non-finite values."""
    device = on_device(named)
    for n, a in named:
        floating = a.dtype.is_floating_point if isinstance(a, torch.Tensor) else np.issubdtype(a.dtype, np.floating)
        if not floating:
            raise ValueError(f"{n}: expected a float dtype, got {a.dtype}")
    if not device:
        _lib.require_device()
        raise _lib.HipExtensionError(f"{names or ' / '.join(n for n, _ in named)}: expected tensors on the GPU "
                                     "(cuda/HIP device); there is no CPU fallback")
    return checked_f64(named)


def visibilities(tensors, vis_thr):
    """What ``vis_thr`` reads of a checked batch: the fourth input, else the third keypoint column; None without it."""
    return None if vis_thr is None else tensors[3] if len(tensors) > 3 else tensors[0][..., 2]


def visiting_order(scores: torch.Tensor, pos, up=None):
    """(perm [M], pos as a tensor).  perm is the batch group by group, every group's detections by descending score,
    equal scores in the order they were given: two stable sorts, descending score and then group.  ``pos`` [M] is a
    tensor on ``scores``' device (any device), or host data that ``up`` takes there; the upload is issued behind the
    first sort, so that the host's pinning overlaps it."""
    by_score = torch.sort(scores, descending=True, stable=True).indices
    pos = pos if up is None else up(pos)
    by_group = torch.sort(pos[by_score], stable=True).indices
    return by_score[by_group], pos


def unsorted(perm: torch.Tensor, x_s: torch.Tensor) -> torch.Tensor:
    """``x_s``, which is in visiting order, in the order the batch was given in: out[perm] = x_s."""
    out = torch.empty_like(x_s)
    out[perm] = x_s
    return out
