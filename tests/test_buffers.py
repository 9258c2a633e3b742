"""The capture rule of _buffers.CaptureCache on CPU tensors, with the "a graph is being captured" flag injected."""
import gc
import weakref

import torch

from probpose_pytorch_amd._buffers import CaptureCache


class _Flag:
    on = False

    def __call__(self):
        return self.on


def _make(n=4):
    return lambda: torch.zeros(n)


def test_an_entry_taken_while_capturing_survives_any_number_of_insertions():
    flag = _Flag()
    c = CaptureCache(2, capturing=flag)
    flag.on = True
    t = c.get("captured", _make())
    flag.on = False
    addr = t.data_ptr()
    for i in range(50):
        c.get(i, _make())
    assert c.marked("captured") and c.peek("captured") is t and t.data_ptr() == addr
    assert c.get("captured", lambda: 1 / 0) is t
    assert len(c) == 3


def test_a_marked_entry_that_has_to_grow_leaves_its_old_tensor_alive():
    flag = _Flag()
    c = CaptureCache(2, capturing=flag)
    flag.on = True
    old = weakref.ref(c.get("ws", _make(4), lambda t: t.numel() >= 4))
    flag.on = False
    new = c.get("ws", _make(8), lambda t: t.numel() >= 8)
    assert new.numel() == 8 and not c.marked("ws")             # the new buffer has not been in a capture
    gc.collect()
    assert old() is not None and old().numel() == 4
    # an unmarked entry that has to grow is freed
    plain = weakref.ref(c.get("plain", _make(4)))
    c.get("plain", _make(8), lambda t: t.numel() >= 8)
    gc.collect()
    assert plain() is None


def test_unmarked_entries_stay_within_the_bound_and_the_least_recently_used_goes_first():
    c = CaptureCache(3, capturing=_Flag())
    for k in "abc":
        c.get(k, _make())
    c.get("a", _make())                                        # a is now the most recently used
    c.get("d", _make())
    assert list(c) == ["c", "a", "d"]
    for i in range(20):
        c.get(i, _make())
        assert len(c) <= 3
    assert list(c) == [17, 18, 19]


def test_a_hit_while_capturing_marks_the_entry():
    flag = _Flag()
    c = CaptureCache(1, capturing=flag)
    t = c.get("k", _make())
    assert not c.marked("k")
    flag.on = True
    assert c.get("k", _make()) is t and c.marked("k")
    flag.on = False
    c.get("x", _make())
    c.get("y", _make())
    assert c.peek("k") is t and list(c) == ["k", "y"]


def test_no_bound_keeps_everything():
    c = CaptureCache(capturing=_Flag())
    for i in range(100):
        c.get(i, _make())
    assert len(c) == 100
