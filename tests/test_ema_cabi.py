"""CPU tests of the ModelEma boundary: pp_ema_table_build packs what it is given (checked by decoding the bytes) and
refuses bad arguments on the host, pp_ema_update refuses before any launch; none of this needs a GPU."""
import ctypes as C
import struct

import numpy as np

CHUNK = 8192
MAGIC = 0x454D4131          # "EMA1"


def _build(lib, src=(0x10000, 0x20000, 0x30000, 0x50004), dst=(0x110000, 0x120000, 0x130000, 0x150004),
           counts=(5, CHUNK, 2 * CHUNK + 7, 2), kinds=(0, 0, 0, 1), n=None, table_off=0, null=()):
    n = len(counts) if n is None else n
    src_a, dst_a = np.asarray(src, dtype=np.uint64), np.asarray(dst, dtype=np.uint64)
    counts_a, kinds_a = np.asarray(counts, dtype=np.int64), np.asarray(kinds, dtype=np.int32)
    host = np.zeros(1024, dtype=np.uint64)
    nc = C.c_int(-1)
    args = dict(src=src_a.ctypes.data, dst=dst_a.ctypes.data, counts=counts_a.ctypes.data, kinds=kinds_a.ctypes.data,
                table=host.ctypes.data + table_off)
    for k in null:
        args[k] = None
    rc = lib.pp_ema_table_build(n, args["src"], args["dst"], args["counts"], args["kinds"], args["table"],
                                C.byref(nc))
    return rc, nc.value, host


def test_table_build_packs_what_it_is_given(built_lib):
    rc, nc, host = _build(built_lib)
    assert rc == 0, built_lib.pp_last_error()
    assert nc == 1 + 1 + 3 + 1
    counts = np.array([5, CHUNK, 2 * CHUNK + 7, 2], dtype=np.int64)
    nbytes = built_lib.pp_ema_table_bytes(4, counts.ctypes.data)
    assert nbytes == 32 + 4 * 32 + 8 * nc
    raw = host.tobytes()
    magic, n_tensors, n_chunks, chunk_elems, *pad = struct.unpack_from("<I7i", raw, 0)
    assert (magic, n_tensors, n_chunks, chunk_elems, pad) == (MAGIC, 4, nc, CHUNK, [0, 0, 0, 0])
    rows = [struct.unpack_from("<QQqii", raw, 32 + 32 * i) for i in range(4)]
    assert rows == [(0x10000, 0x110000, 5, 0, 0), (0x20000, 0x120000, CHUNK, 0, 0),
                    (0x30000, 0x130000, 2 * CHUNK + 7, 0, 0), (0x50004, 0x150004, 2, 1, 0)]
    chunk_map = np.frombuffer(raw, dtype=np.int32, count=2 * nc, offset=32 + 4 * 32).reshape(nc, 2)
    assert chunk_map.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [3, 0]]
    assert not any(raw[nbytes:])                                     # nothing written past the table


def test_table_build_refuses_bad_arguments(built_lib):
    L = built_lib
    ok_src, ok_dst = (0x10000, 0x20000, 0x30000, 0x50004), (0x110000, 0x120000, 0x130000, 0x150004)
    for kwargs, word in (
            (dict(n=0), b"zero tensors"), (dict(n=-2), b"zero tensors"),
            (dict(counts=(5, -1, 7, 2)), b"count"), (dict(counts=(5, 0, 7, 2)), b"count"),
            (dict(src=(0x10000, 0, 0x30000, 0x50004)), b"null pointer"),
            (dict(dst=(0x110000, 0x120000, 0, 0x150004)), b"null pointer"),
            (dict(src=(0x10002, *ok_src[1:])), b"aligned"), (dict(dst=(0x110001, *ok_dst[1:])), b"aligned"),
            (dict(table_off=4), b"8-byte aligned"),
            (dict(kinds=(0, 2, 0, 1)), b"kind"), (dict(kinds=(0, 0, -1, 1)), b"kind"),
            (dict(null=("src",)), b"null argument"), (dict(null=("dst",)), b"null argument"),
            (dict(null=("kinds",)), b"null argument"), (dict(null=("table",)), b"null argument"),
            (dict(null=("counts",)), b"null"),
            (dict(dst=ok_src), b"overlaps"),                                             # in place: dst is src
            (dict(dst=(0x10010, *ok_dst[1:])), b"overlaps src"),                         # dst 0 inside src 0
            (dict(dst=(0x110000, 0x120000, 0x20000 - 4 * (2 * CHUNK + 7) + 4, 0x150004)), b"overlaps src"),
            (dict(dst=(0x110000, 0x110010, 0x130000, 0x150004)), b"overlaps dst"),       # dst 0 and dst 1 share words
            (dict(dst=(0x110000, 0x120000, 0x130000, 0x130000 + 4 * (2 * CHUNK + 6))), b"overlaps dst")):
        rc = _build(L, **kwargs)[0]
        assert rc != 0 and word in L.pp_last_error(), (kwargs, L.pp_last_error())
    # ranges that touch without sharing a word are fine: dst 0 ends where src 1 begins
    assert _build(L, dst=(0x20000 - 20, *ok_dst[1:]))[0] == 0, L.pp_last_error()
    counts = np.array([5, 0, 7], dtype=np.int64)
    assert L.pp_ema_table_bytes(3, counts.ctypes.data) == -1 and b"count" in L.pp_last_error()
    assert L.pp_ema_table_bytes(0, counts.ctypes.data) == -1
    assert L.pp_ema_table_bytes(3, None) == -1 and b"null" in L.pp_last_error()


def test_update_refuses_bad_arguments_without_gpu(built_lib):
    L = built_lib
    assert L.pp_ema_update(None, 4, 0.5, None) != 0 and b"null table" in L.pp_last_error()
    assert L.pp_ema_update(0x1004, 4, 0.5, None) != 0 and b"aligned" in L.pp_last_error()
    assert L.pp_ema_update(0x1000, 0, 0.5, None) != 0 and b"n_chunks" in L.pp_last_error()
    assert L.pp_ema_update(0x1000, -1, 0.5, None) != 0 and b"n_chunks" in L.pp_last_error()
    for w in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.pp_ema_update(0x1000, 4, w, None) != 0 and b"weight" in L.pp_last_error()


def test_python_binding_names_the_kinds():
    from probpose_pytorch_amd import _lib
    assert (_lib.PP_EMA_LERP_F32, _lib.PP_EMA_COPY_WORDS) == (0, 1)
    assert {"pp_ema_table_bytes", "pp_ema_table_build", "pp_ema_update"} <= set(_lib.EXPORTS)
