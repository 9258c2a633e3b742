"""Who keeps alive what the host hands to the device: the pinned staging pool, the pinned upload, and the one cache
of device buffers whose addresses a captured HIP graph may have baked in."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch


def host_array(x, name: str, dtype) -> np.ndarray:
    """``x`` (array-like or tensor) as a contiguous host array of ``dtype``; ValueError names ``name``."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    try:
        return np.ascontiguousarray(np.asarray(x), dtype=dtype)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name}: cannot be read as {np.dtype(dtype).name} ({e})") from None


def room(t: torch.Tensor) -> torch.Tensor:
    """A tensor the library can take the address of: an empty one gets one element of room."""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def upload(a, device, keep: list, dtype=None) -> torch.Tensor:
    """To the device without a synchronising copy: host data goes through a pinned tensor, which is appended to
    ``keep`` (the caller holds it until the copy has run).  A device tensor is cast and made contiguous; an empty
    input becomes an empty device tensor without a copy."""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a.to(dtype=dtype or a.dtype).contiguous()
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.numel() == 0:
        return torch.zeros(t.shape, dtype=dtype or t.dtype, device=device)
    t = t.to(dtype=dtype or t.dtype).contiguous().pin_memory()
    keep.append(t)
    return t.to(device=device, non_blocking=True)


class PinnedStaging:
    """A pool of pinned host buffers for asynchronous uploads that are rewritten every step.  A slot is
    [uint8 pinned tensor, event]: fill the tensor, issue the copy, ``slot[1].record()``."""

    def __init__(self):
        self._slots = []

    def __len__(self):
        return len(self._slots)

    def take(self, nbytes: int):
        """A slot that no earlier asynchronous copy can still be reading: one whose event has completed, or a new
        one.  Never waits."""
        for slot in self._slots:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._slots.append(slot)
        return slot


class CaptureCache:
    """Keyed cache of values that hold device memory whose ADDRESSES kernels are given.  A captured graph bakes those
    addresses in, so the rule is: an entry handed out while the current stream is capturing is marked and never
    evicted; a marked entry that has to be replaced (the caller needs a larger buffer) is retired, not freed; unmarked
    entries age out least recently used first once there are more than ``bound`` of them (None: never)."""

    def __init__(self, bound=None, capturing=torch.cuda.is_current_stream_capturing):
        self._bound, self._capturing = bound, capturing
        self._entries = OrderedDict()       # least recently used first
        self._marked = set()
        self._retired = []

    def __len__(self):
        return len(self._entries)

    def __iter__(self):
        return iter(self._entries)

    def marked(self, key) -> bool:
        return key in self._marked

    def peek(self, key):
        """The value of ``key`` or None; changes neither its age nor its mark."""
        return self._entries.get(key)

    def get(self, key, make, fits=None):
        """The value of ``key``; ``make()`` builds it when there is none, or when ``fits(value)`` is false."""
        v = self._entries.get(key)
        fresh = v is None or (fits is not None and not fits(v))
        if fresh:
            if key in self._marked:         # a captured graph still points into the old value
                self._retired.append(v)
                self._marked.discard(key)
            v = self._entries[key] = make()
        self._entries.move_to_end(key)
        if self._capturing():
            self._marked.add(key)
        if fresh and self._bound is not None:
            unmarked = [k for k in self._entries if k not in self._marked]
            for k in unmarked[:max(0, len(unmarked) - self._bound)]:
                del self._entries[k]
        return v
