"""Record which pp_gemm calls the dispatcher admits: tests/golden/gemm_admission.json.

pp_gemm checks its arguments before its first HIP call, so on a machine without a GPU a refused call returns non-zero
with a message that starts with "pp_gemm:", and an admitted one reaches the runtime and fails there
("hipFuncSetAttribute...", "hipGetDevice...", "launch ...").  The pointers are fake: never run this where a GPU is
visible.  Run once, at the commit whose verdicts are to be kept:  python tests/golden/make_gemm_admission.py
tests/test_gemm_admission.py imports cases() and verdict() from here and replays the recorded matrix."""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "gemm_admission.json")

DTYPES = ("f32", "bf16", "fp8")
# N <= 256 and > 256; M, N whole and ragged against 192 / 256 / 288; N % 4 != 0; K in {256, 512, 768}
SHAPES = ((768, 576, 512), (768, 768, 768), (192, 256, 256), (300, 576, 512), (384, 200, 256), (257, 129, 256),
          (576, 1152, 512), (400, 400, 768))
EPILOGUES = ("none", "bias_gelu", "relu", "residual_f32", "rowbias_f32", "heatmap", "headmajor", "fuse_final", "out_fp8")
STRUCTURES = ("plain", "gather", "rowmap", "batch4", "splitk2")
C_ALIGN = (16, 4)
TILES = tuple(range(-1, 22))
LIVE_TILES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 18, 19, 20)


def make_args(_lib, dtype, shape, epilogue, structure, c_align):
    """One pp_gemm_args (tile left at 0) for a point of the matrix; every pointer is a fake, suitably aligned address."""
    M, N, K = shape
    a = _lib.GemmArgs()
    a.A, a.W, a.C = 0x10000, 0x20000, 0x30000 + (0 if c_align == 16 else 4)
    a.M, a.N, a.Kd, a.lda, a.ldw, a.ldc, a.batch = M, N, K, K, K, N, 1
    a.dtype = {"f32": _lib.PP_F32, "bf16": _lib.PP_BF16, "fp8": _lib.PP_FP8}[dtype]
    if dtype == "fp8":
        a.colsum = 0x40000
    if epilogue == "bias_gelu":
        a.epilogue, a.bias = _lib.EPI_BIAS | _lib.EPI_GELU, 0x50000
    elif epilogue == "relu":
        a.epilogue = _lib.EPI_RELU
    elif epilogue == "residual_f32":
        a.epilogue, a.residual = _lib.EPI_RESIDUAL | _lib.EPI_OUT_F32, 0x60000
    elif epilogue == "rowbias_f32":
        a.epilogue, a.rowbias, a.rowbias_period = _lib.EPI_ROWBIAS | _lib.EPI_OUT_F32, 0x70000, 16
    elif epilogue == "heatmap":
        a.epilogue, a.hm_K, a.hm_HW, a.hm_temperature = _lib.EPI_HEATMAP, N, 64, 0.5
    elif epilogue == "headmajor":       # N = 3 * heads * head_dim where the shape allows it (else the call is refused)
        hd = 64 if N % 192 == 0 else 8
        a.epilogue, a.hm_K, a.hm_HW = _lib.EPI_HEADMAJOR, max(1, N // (3 * hd)), hd
    elif epilogue == "fuse_final":
        a.epilogue, a.bias = _lib.EPI_FUSE_FINAL | _lib.EPI_BIAS | _lib.EPI_RELU, 0x50000
        a.final_w, a.final_b, a.hm_K, a.hm_HW, a.hm_temperature = 0x80000, 0x90000, 17, 3072, 0.5
    elif epilogue == "out_fp8":
        a.epilogue, a.out_scale = _lib.EPI_OUT_FP8, 1.0
    if structure == "gather":
        a.rowoff, a.seg_len = 0xA0000, 128
    elif structure == "rowmap":
        a.out_rowmap = 0xB0000
    elif structure == "batch4":
        a.batch, a.strideA, a.strideW, a.strideC, a.strideBias = 4, M * K, N * K, M * N, N
    elif structure == "splitk2":        # Kd is the per-split depth; the partials are plain f32
        a.splitk, a.epilogue = 2, a.epilogue | _lib.EPI_OUT_F32
        a.lda, a.ldw, a.strideA_k, a.strideW_k, a.strideC_k = 2 * K, 2 * K, K, K, M * N
    return a


def cases():
    """(key, (dtype, shape, epilogue, structure, c_align)) for every point of the matrix but the tile."""
    for c in itertools.product(DTYPES, SHAPES, EPILOGUES, STRUCTURES, C_ALIGN):
        dtype, shape, epilogue, structure, c_align = c
        yield "|".join((dtype, "x".join(map(str, shape)), epilogue, structure, "c%d" % c_align)), c


def verdict(lib, a, tile):
    """'A' (admitted: the call got as far as the HIP runtime) or 'R' (refused by pp_gemm's own checks)."""
    a.tile = tile
    rc = lib.pp_gemm(C.byref(a), None)
    msg = lib.pp_last_error()
    assert rc != 0, "pp_gemm succeeded on fake pointers: is a GPU visible?"
    if msg.startswith(b"pp_gemm:"):
        return "R"
    assert msg.startswith((b"hipFuncSetAttribute", b"hipGetDevice", b"launch ")), msg
    return "A"


def record(lib, _lib):
    return {key: "".join(verdict(lib, make_args(_lib, *c), t) for t in TILES) for key, c in cases()}


def main():
    sys.path.insert(0, REPO)
    import torch
    assert not torch.cuda.is_available(), "fake pointers: run this without a GPU"
    import __graft_entry__ as g
    g.build()
    from probpose_pytorch_amd import _lib
    verdicts = record(_lib.lib(), _lib)
    for t in LIVE_TILES:                 # the matrix must show every live form both ways
        col = [v[TILES.index(t)] for v in verdicts.values()]
        assert "A" in col and "R" in col, f"tile {t}: {col.count('A')} admitted, {col.count('R')} refused"
    doc = {"tiles": list(TILES), "verdicts": verdicts}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    n = len(verdicts) * len(TILES)
    print(f"{OUT}: {n} cases, {sum(v.count('A') for v in verdicts.values())} admitted")


if __name__ == "__main__":
    main()
