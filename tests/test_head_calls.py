"""head_calls' descriptors against the keyword sets the head's call sites passed when each of them typed its own:
the one place those literals survive, so that a later edit to a descriptor is a visible decision.  CPU only.

Two arguments that no kernel reads differ from what single sites passed, and are written as the descriptors have them:
the eval plan's k = 1 convolutions passed seg_len = cin beside rowoff = None (pp_gemm takes seg_len = Kd = cin when
there is no table: the same kernel parameter), and the aux stages' data gradient passed no strideBias (it has no bias).
"""
import itertools

import pytest

from probpose_pytorch_amd import head_calls as HC

MS, WIDTHS, KS, BRANCHES, SPLITS = (1, 30, 195), (64, 256), (5, 17, 133), (1, 2, 4), (1, 3, 9)


@pytest.mark.parametrize("M,cin,cout", itertools.product(MS, WIDTHS, WIDTHS + KS))
def test_deconv_forward_weight_and_data_gradient(M, cin, cout):
    assert HC.deconv(M, cin, cout) == dict(M=M, N=cout, Kd=4 * cin, lda=cin, ldw=4 * cin, ldc=cout, seg_len=cin, batch=4,
                                           strideW=cout * 4 * cin, strideRowoff=4 * M, strideRowmap=M)
    assert HC.wgrad_of(HC.deconv(M, cin, cout)) == dict(M=M, N=cout, Kd=4 * cin, ldd=cout, seg_len=cin, batch=4,
                                                        strideRowoff=4 * M, strideRowmap=M, strideDW=cout * 4 * cin)
    assert HC.deconv_dgrad(M, cin, cout) == dict(M=M, N=cin, Kd=16 * cout, lda=cout, ldw=16 * cout, ldc=cin,
                                                 seg_len=cout)


@pytest.mark.parametrize("M,cin,cout", itertools.product(MS, WIDTHS, WIDTHS + KS))
def test_conv_and_final_layer(M, cin, cout):
    for k in (3, 5):
        kk = k * k
        assert HC.conv(M, cin, cout, k) == dict(M=M, N=cout, Kd=kk * cin, lda=cin, ldw=kk * cin, ldc=cout, seg_len=cin)
    assert HC.conv(M, cin, cout, 1) == dict(M=M, N=cout, Kd=cin, lda=cin, ldw=cin, ldc=cout)
    assert HC.wgrad_of(HC.conv(M, cin, cout, 3)) == dict(M=M, N=cout, Kd=9 * cin, ldd=cout, seg_len=cin)


@pytest.mark.parametrize("M,cin,K", itertools.product(MS, WIDTHS, KS))
def test_final_layer_gradients_at_the_ktile_pitch(M, cin, K):
    assert HC.KTILE == 64
    KPAD = -(-K // 64) * 64
    assert HC.kpad(K) == KPAD and KPAD % 64 == 0 and 0 <= KPAD - K < 64
    assert HC.final_dgrad(M, cin, K) == dict(M=M, N=cin, Kd=KPAD, lda=KPAD, ldw=KPAD, ldc=cin)
    assert dict(HC.wgrad_of(HC.conv(M, cin, K, 1)), ldd=KPAD) == dict(M=M, N=K, Kd=cin, ldd=KPAD, lda=cin)


@pytest.mark.parametrize("M,C,br", itertools.product(MS, WIDTHS, BRANCHES))
def test_aux_stages(M, C, br):
    assert HC.aux_stage0(M, C) == dict(M=M, N=4 * C, Kd=9 * C, lda=C, ldw=9 * C, ldc=4 * C, seg_len=C)
    assert HC.aux_stage(M, C) == HC.aux_stage(M, C, 4, 1)
    # the weight gradients over a run of br branches
    assert HC.wgrad_of(HC.aux_stage0(M, C, br)) == dict(M=M, N=br * C, Kd=9 * C, ldd=4 * C, seg_len=C)
    assert HC.wgrad_of(HC.aux_stage(M, C, br)) == dict(M=M, N=C, Kd=9 * C, ldd=4 * C, seg_len=C, batch=br, strideDY=C,
                                                       strideA=C, strideDW=C * 9 * C, strideDB=C)
    assert HC.aux0_dgrad(M, C, br) == dict(M=M, N=C, Kd=9 * br * C, lda=4 * C, ldw=9 * br * C, ldc=C, seg_len=C)
    for split in SPLITS:
        got = HC.aux_stage(M, C, br, split)
        if split == 1:      # forward (with its bias) and data gradient
            assert got == dict(M=M, N=C, Kd=9 * C, lda=4 * C, ldw=9 * C, ldc=4 * C, seg_len=C, batch=br, strideA=C,
                               strideW=C * 9 * C, strideC=C, strideBias=C)
        else:
            taps = 9 // split
            assert got == dict(M=M, N=C, Kd=taps * C, lda=4 * C, ldw=9 * C, ldc=4 * C, seg_len=C, batch=br, strideA=C,
                               strideW=C * 9 * C, strideC=C, splitk=split, strideW_k=taps * C, strideRowoff_k=taps * M,
                               strideC_k=M * 4 * C)


def test_aux_split_is_a_property_of_the_stage():
    assert [HC.aux_split(i) for i in (1, 2, 3)] == [3, 9, 9]


def test_wgrad_of_refuses_a_split_k_descriptor():
    with pytest.raises(AssertionError):
        HC.wgrad_of(HC.aux_stage(30, 64, split=3))


def test_head_train_keeps_the_names_tests_look_up():
    from probpose_pytorch_amd import head_train
    assert head_train.KTILE == HC.KTILE and callable(head_train._aux0_dgrad_table)
