"""_lib.call / _lib.launch: the one way the wrappers reach the C ABI.  None of this needs a GPU: the host-side checks
of the library run before any launch."""
import ctypes

import numpy as np
import pytest
import torch

NULL_DECODE = (None, None, None, None, None, 1, 17, 64, 48, None, None, 1.0, 1.0, 1.0, 1.0,
               None, None, None, None, None, None, None, None, 0, None)      # as tests/test_cabi.py


@pytest.fixture(scope="module")
def lib(built_lib):
    from probpose_pytorch_amd import _lib
    return _lib


def test_values_are_returned(lib):
    assert lib.call("pp_version") >= 100
    assert lib.call("pp_decode_workspace_bytes", 1, 17, 64, 48) == 76


def test_numpy_arrays_go_as_host_pointers(lib):
    assert lib.call("pp_ema_table_bytes", 1, np.array([5], np.int64)) == 72          # 32 + 32 + 8


def test_a_negative_size_raises_and_names_the_entry(lib):
    with pytest.raises(lib.HipExtensionError, match="pp_ema_table_bytes"):
        lib.call("pp_ema_table_bytes", 0, None)


def test_a_failed_status_raises_with_the_entry_and_the_library_text(lib):
    with pytest.raises(lib.HipExtensionError) as e:
        lib.call("pp_decode_f32", *NULL_DECODE)
    assert "pp_decode_f32" in str(e.value) and "null" in str(e.value)


@pytest.mark.parametrize("bad", [torch.zeros(1), np.zeros(1)], ids=["tensor", "ndarray"])
def test_an_address_in_an_int_slot_fails_before_the_library_is_entered(lib, bad):
    with pytest.raises(lib.HipExtensionError):
        lib.call("pp_decode_f32", *NULL_DECODE)                # leaves a known text in pp_last_error()
    before = lib.lib().pp_last_error()
    assert b"null" in before
    with pytest.raises(ctypes.ArgumentError):
        lib.call("pp_ema_table_bytes", bad, None)              # would otherwise fail inside and rewrite the text
    assert lib.lib().pp_last_error() == before


def test_launch_appends_the_current_stream(lib, monkeypatch):
    seen = []
    monkeypatch.setattr(lib, "stream_ptr", lambda: "the stream")
    monkeypatch.setattr(lib, "call", lambda name, *args: seen.append((name, args)))
    lib.launch("pp_x", 1, None)
    assert seen == [("pp_x", (1, None, "the stream"))]
