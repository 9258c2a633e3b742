"""The pp_gemm / pp_wgrad_gemm calls of ProbMapHead's layers, each stated once: what the eval plan (engine.HeadPlan),
the training path (head_train.py) and the tests that hold those calls to float64 all pass.

Pure functions of the layer dimensions (no tensors, no device) returning the keywords of ``ops.gemm``: dimensions,
pitches, strides, ``seg_len``, ``batch`` and the split-K terms.  The caller adds the operands, the gather / scatter
tables, the bias and the epilogue.  Activations are channels-last rows; M counts the rows of the layer's *input* map (a
deconvolution writes 4 M rows, one parity each); the aux buffers are [M, 4C], the four branches side by side.
"""
from __future__ import annotations

KTILE = 64         # the heatmap gradient's channel pitch is a whole number of pp_gemm K-tiles in both compute dtypes


def kpad(K: int) -> int:
    """The channel pitch of the heatmap gradient dz [M, KPAD]."""
    return -(-K // KTILE) * KTILE


def deconv(M: int, cin: int, cout: int) -> dict:
    """A stride-2 deconvolution: batch = 4 output parities of 4 taps each (pack.pack_deconv_parities, deconv_tables).
    The fused-final site is cout = 256, the identity-final site cout = K."""
    return dict(M=M, N=cout, Kd=4 * cin, lda=cin, ldw=4 * cin, ldc=cout, seg_len=cin, batch=4,
                strideW=cout * 4 * cin, strideRowoff=4 * M, strideRowmap=M)


def conv(M: int, cin: int, cout: int, k: int) -> dict:
    """A k x k stride-1 convolution over taps-major weights (the conv stack, the final layer); k = 1: a plain GEMM."""
    kw = dict(M=M, N=cout, Kd=k * k * cin, lda=cin, ldw=k * k * cin, ldc=cout)
    return dict(kw, seg_len=cin) if k > 1 else kw


def aux_stage0(M: int, C: int, branches: int = 4) -> dict:
    """The first aux stage: the branches share their input, so one GEMM writes their column blocks of [M, 4C]."""
    return dict(M=M, N=branches * C, Kd=9 * C, lda=C, ldw=9 * C, ldc=4 * C, seg_len=C)


def aux_split(stage: int) -> int:
    """The split-K factor of aux stage >= 1: few rows (16 B, then 4 B) against K = 9 C, so the taps are split over
    workgroups when the plain launch would leave most CUs idle behind 108 sequential K-tiles (S f32 partials, summed in
    the pooling).  The split is a property of the LAYER (3 for the first pooled stage, 9 from the second on), never of
    the batch size: a crop's outputs stay bit-identical whatever batch it is computed in (the partial-sum order would
    otherwise change with B).  At large batches the partials cost ~0.2 % of the step."""
    return 3 if stage == 1 else 9


def aux_stage(M: int, C: int, branches: int = 4, split: int = 1) -> dict:
    """A later aux stage: the branches' 3x3 convolutions as batch entries on their C-wide column blocks of [M, 4C] (a
    run [b0, b1): branches = b1 - b0 on operands offset by b0 * C columns).  Its data gradient has the same dimensions
    and is this descriptor too.  split > 1: partial s of [split, M, 4C] holds taps [s, s + 1) * 9 / split, no bias."""
    kw = dict(M=M, N=C, Kd=9 * C, lda=4 * C, ldw=9 * C, ldc=4 * C, seg_len=C, batch=branches, strideA=C,
              strideW=C * 9 * C, strideC=C)
    if split == 1:
        return dict(kw, strideBias=C)
    taps = 9 // split
    return dict(kw, Kd=taps * C, splitk=split, strideW_k=taps * C, strideRowoff_k=taps * M, strideC_k=M * 4 * C)


def final_dgrad(M: int, cin: int, K: int) -> dict:
    """The final 1x1 layer's data gradient: dz [M, KPAD] against the transposed weight zero-padded to [cin, KPAD]."""
    return dict(M=M, N=cin, Kd=kpad(K), lda=kpad(K), ldw=kpad(K), ldc=cin)


def deconv_dgrad(M: int, cin: int, cout: int) -> dict:
    """A 4x4 stride-2 deconvolution's data gradient: dY [4M, cout] gathered at 16 taps (pack.deconv_data_grad_table)."""
    return dict(M=M, N=cin, Kd=16 * cout, lda=cout, ldw=16 * cout, ldc=cin, seg_len=cout)


def aux0_dgrad(M: int, C: int, n_branches: int) -> dict:
    """The first aux stage's data gradient into the tokens: n_branches column blocks of dY [M, 4C] in one GEMM."""
    return dict(M=M, N=C, Kd=9 * n_branches * C, lda=4 * C, ldw=9 * n_branches * C, ldc=C, seg_len=C)


def wgrad_of(call: dict) -> dict:
    """The ``ops.wgrad`` keywords of the layer whose forward keywords are ``call``: dY has the output's pitch and stride,
    dW and dB the weight's and the bias's.  A gathered call passes no lda: pp_wgrad_gemm reads A through rowoff alone."""
    assert "splitk" not in call
    renamed = dict(ldc="ldd", strideC="strideDY", strideW="strideDW", strideBias="strideDB")
    kept = ("M", "N", "Kd", "seg_len", "batch", "strideA", "strideRowoff", "strideRowmap") + (
        () if "seg_len" in call else ("lda",))
    return {renamed.get(k, k): v for k, v in call.items() if k in renamed or k in kept}
