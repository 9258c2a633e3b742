"""Flip test without a GPU: the permutation and its refusals, the numpy restatement against planted faults, the host-side
refusals of pp_hflip_pair / pp_flip_merge through the C ABI, and the CLI's argument errors."""
import numpy as np
import pytest

from tests import flip_reference as FR

PAIRS20 = [(2 * i + 1, 2 * i + 2) for i in range(8)]         # keypoints 0, 17, 18, 19 have no partner


# ---- permutation ---------------------------------------------------------------------------------------------------------
def test_permutation_is_an_involution_with_fixed_points():
    from probpose_pytorch_amd.flip import COCO17_FLIP_PAIRS, flip_permutation
    perm = flip_permutation(PAIRS20, 20)
    assert perm.dtype == np.int32 and perm.shape == (20,)
    assert np.array_equal(perm[perm], np.arange(20))
    assert [k for k in range(20) if perm[k] == k] == [0, 17, 18, 19]
    assert all(perm[i] == j and perm[j] == i for i, j in PAIRS20)
    assert np.array_equal(perm, FR.permutation(PAIRS20, 20))
    assert np.array_equal(flip_permutation((), 5), np.arange(5))
    assert COCO17_FLIP_PAIRS == ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
    assert np.array_equal(flip_permutation(COCO17_FLIP_PAIRS, 17), FR.permutation(COCO17_FLIP_PAIRS, 17))


@pytest.mark.parametrize("pairs", [[(1, 20)], [(-1, 2)], [(1, 2), (2, 3)], [(1, 2), (1, 2)], [(4, 4)]])
def test_permutation_refusals(pairs):
    from probpose_pytorch_amd.flip import flip_permutation
    with pytest.raises(ValueError):
        flip_permutation(pairs, 20)


def test_permutation_agrees_with_augment():
    from probpose_pytorch_amd.dataset import Augment
    from probpose_pytorch_amd.flip import flip_permutation
    assert np.array_equal(Augment(flip_pairs=PAIRS20).permutation(20), flip_permutation(PAIRS20, 20))
    for pairs in ([(1, 20)], [(1, 2), (2, 3)], [(4, 4)]):                     # and refuses what it refuses, in its words
        with pytest.raises(ValueError, match="Augment: flip pair"):
            Augment(flip_pairs=pairs).permutation(20)


def test_parse_flip_pairs():
    from probpose_pytorch_amd.flip import parse_flip_pairs
    assert parse_flip_pairs("1-2, 3-4,15-16") == ((1, 2), (3, 4), (15, 16))
    for bad in ("1_2", "1-", "a-b", ""):
        with pytest.raises(ValueError):
            parse_flip_pairs(bad)


# ---- the restatement against planted faults ----------------------------------------------------------------------------------
def _random_outputs(B2, K, H, W, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((B2, K, H, W), dtype=np.float32),) + tuple(rng.random((B2, K, 1, 1), dtype=np.float32)
                                                                  for _ in range(4))


def test_reference_by_hand_and_planted_faults():
    B, K, H, W = 2, 5, 3, 6
    perm = FR.permutation([(1, 2)], K)
    out2 = _random_outputs(2 * B, K, H, W, 0)
    want = FR.merge(out2, perm)
    assert [w.shape for w in want] == [(B, K, H, W)] + [(B, K, 1, 1)] * 4 and all(w.dtype == np.float32 for w in want)
    # element by element from the formula
    for b in range(B):
        for k in range(K):
            for u in range(W):
                col = (out2[0][b, k, :, u] + out2[0][B + b, perm[k], :, W - 1 - u]) * np.float32(0.5)
                assert np.array_equal(want[0][b, k, :, u], col)
            for j in range(1, 5):
                assert want[j][b, k, 0, 0] == (out2[j][b, k, 0, 0] + out2[j][B + b, perm[k], 0, 0]) * np.float32(0.5)
    for fault in ("mirror_no_swap", "swap_no_mirror", "no_half", "off_by_one"):
        assert not np.array_equal(FR.merge(out2, perm, fault=fault)[0], want[0]), fault
    # the swap faults show on the paired channels only, the mirror faults everywhere
    bad = FR.merge(out2, perm, fault="mirror_no_swap")[0]
    assert np.array_equal(bad[:, [0, 3, 4]], want[0][:, [0, 3, 4]]) and not np.array_equal(bad[:, 1], want[0][:, 1])
    # merging a batch with its own flipped-and-swapped copy gives the batch back: the merge undoes the pair-flip
    x = _random_outputs(B, K, H, W, 1)
    mirrored = (x[0][:, perm][..., ::-1],) + tuple(a[:, perm] for a in x[1:])
    same = FR.merge(tuple(np.concatenate([a, m]) for a, m in zip(x, mirrored)), perm)
    assert all(np.array_equal(s, a) for s, a in zip(same, x))
    # pair: both halves
    img = FR.special_floats((2, 3, 4, 6), 2)
    p = FR.pair(img)
    assert p.shape == (4, 3, 4, 6) and np.array_equal(p[:2].view(np.uint32), img.view(np.uint32))
    assert all(np.array_equal(p[2:, :, :, u].view(np.uint32), img[:, :, :, 5 - u].view(np.uint32)) for u in range(6))


# ---- C ABI refusals ----------------------------------------------------------------------------------------------------------
def test_hflip_pair_refusals_without_gpu(built_lib):
    L = built_lib
    x, out = 0x10000, 0x80000
    assert L.pp_hflip_pair(None, out, 1, 3, 4, 8, None) != 0 and b"null" in L.pp_last_error()
    assert L.pp_hflip_pair(x, None, 1, 3, 4, 8, None) != 0 and b"null" in L.pp_last_error()
    for shape in ((0, 3, 4, 8), (1, 0, 4, 8), (1, 3, 0, 8), (1, 3, 4, 0), (-1, 3, 4, 8)):
        assert L.pp_hflip_pair(x, out, *shape, None) != 0 and b"positive" in L.pp_last_error(), shape
    assert L.pp_hflip_pair(x, out, 1 << 12, 1 << 10, 1 << 10, 8, None) != 0 and b"2^31" in L.pp_last_error()
    assert L.pp_hflip_pair(x, out, 2147483647, 2147483647, 2147483647, 2147483647, None) != 0 \
        and b"2^31" in L.pp_last_error()
    n = 1 * 3 * 4 * 8 * 4
    for alias in (x, x + n - 4, x - 2 * n + 4):                        # in place, the tail of x, the head of x
        assert L.pp_hflip_pair(x, alias, 1, 3, 4, 8, None) != 0 and b"alias" in L.pp_last_error(), alias


def test_flip_merge_refusals_without_gpu(built_lib):
    L = built_lib
    heat2, aux2, perm, heat, aux = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    good = [heat2, aux2, perm, 2, 17, 8, 12, heat, aux, None]
    for i in (0, 1, 2, 7, 8):
        args = list(good)
        args[i] = None
        assert L.pp_flip_merge(*args) != 0 and b"null" in L.pp_last_error(), i
    for i in (3, 4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[i] = v
            assert L.pp_flip_merge(*args) != 0 and b"positive" in L.pp_last_error(), (i, v)
    args = list(good)
    args[3:7] = [1 << 10, 1 << 10, 1 << 10, 4]
    assert L.pp_flip_merge(*args) != 0 and b"2^31" in L.pp_last_error()
    n = 2 * 17 * 8 * 12 * 4                                            # bytes of heat_out
    for alias in (heat2, heat2 + n, heat2 + 2 * n - 4, heat2 - n + 4):  # in place on either half, and partial overlaps
        args = list(good)
        args[7] = alias
        assert L.pp_flip_merge(*args) != 0 and b"alias" in L.pp_last_error(), alias
    for alias in (aux2, aux2 + 4 * 2 * 17 * 4):
        args = list(good)
        args[8] = alias
        assert L.pp_flip_merge(*args) != 0 and b"alias" in L.pp_last_error(), alias
    args = list(good)
    args[8] = heat                                                     # the two outputs on top of each other
    assert L.pp_flip_merge(*args) != 0 and b"alias" in L.pp_last_error()


def test_python_refusals_without_gpu():
    import torch
    from probpose_pytorch_amd import _lib
    from probpose_pytorch_amd.flip import flip_merge
    out2 = tuple(torch.from_numpy(a) for a in _random_outputs(2, 3, 2, 4, 0))
    with pytest.raises(_lib.HipExtensionError):                         # host tensors: no CPU fallback
        flip_merge(out2, torch.arange(3, dtype=torch.int32))


# ---- model surface ---------------------------------------------------------------------------------------------------------------
def _tiny_model(**kw):
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    return ProbPoseModel(ScratchViTBackbone((64, 48), 16, embed_dim=128, depth=1, num_heads=2),
                         ProbMapHead(128, 20, [(4, 3)], (64, 64), (4, 4), final_layer_kernel_size=1), **kw)


def test_model_surface_without_gpu():
    import torch
    plain, model = _tiny_model(), _tiny_model(flip_pairs=PAIRS20)
    assert list(model.state_dict()) == list(plain.state_dict())         # the permutation is not part of the checkpoint
    assert model._flip_perm.dtype == torch.int32 and np.array_equal(model._flip_perm.numpy(), FR.permutation(PAIRS20, 20))
    assert plain._flip_perm is None and plain.set_flip_test(PAIRS20) is plain and plain._flip_perm is not None
    assert plain.set_flip_test(None)._flip_perm is None
    for pairs in ([(1, 20)], [(1, 2), (2, 3)], [(4, 4)]):                # checked against the head's K when set
        with pytest.raises(ValueError):
            model.set_flip_test(pairs)
    with pytest.raises(TypeError):
        from probpose_pytorch_amd.model import ProbPoseModel
        ProbPoseModel(plain.backbone, plain.head, PAIRS20)              # keyword only: two positional arguments as ever
    assert model.eval()._flip_perm is not None and model.train()._flip_perm is not None


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--flip-test", "--num_keypoints", "20"],
                                  ["--flip-test", "--num_keypoints", "20", "--flip-pairs", "1-2,2-3"],
                                  ["--flip-test", "--flip-pairs", "3-17"],
                                  ["--flip-test", "--flip-pairs", "4-4"],
                                  ["--flip-test", "--flip-pairs", "1_2"],
                                  ["--flip-pairs", "1-2"]])
def test_cli_argument_errors(argv, capsys):
    from probpose_pytorch_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(argv)
    assert e.value.code == 2 and "flip" in capsys.readouterr().err


def test_cli_default_pairs():
    import argparse
    from probpose_pytorch_amd import inference
    from probpose_pytorch_amd.flip import COCO17_FLIP_PAIRS
    p = argparse.ArgumentParser()
    ns = argparse.Namespace(flip_test=True, flip_pairs=None, num_keypoints=17)
    assert inference.resolve_flip_pairs(p, ns) == COCO17_FLIP_PAIRS
    ns = argparse.Namespace(flip_test=True, flip_pairs="1-2,5-9", num_keypoints=20)
    assert inference.resolve_flip_pairs(p, ns) == ((1, 2), (5, 9))
    assert inference.resolve_flip_pairs(p, argparse.Namespace(flip_test=False, flip_pairs=None, num_keypoints=20)) is None
