"""Host-side refusals of the ValidationMeter entry points through the built library: they come before any launch, so no
GPU is needed."""
from tests import valmeter_reference as vr

P = 0x1000      # a non-null pointer the refusals never dereference


def _update(lib, J=18, B=4, K=17, thresholds=P, state=P, first=P, mask=P, target=P):
    return lib.pp_valmeter_update(first, P, P, P, target, P, mask, P, P, thresholds, J, None, None, None, B, K, state,
                                  None)


def test_update_refusals(built_lib):
    lib = built_lib
    for kw, word in ((dict(K=0), b"K=0"), (dict(K=-3), b"K=-3"), (dict(J=0), b"J=0"), (dict(J=65), b"J=65"),
                     (dict(B=0), b"B=0"), (dict(thresholds=None), b"thresholds not given"),
                     (dict(first=None), b"null prediction"), (dict(target=None), b"null target"),
                     (dict(mask=None), b"null mask"), (dict(state=None), b"null state")):
        assert _update(lib, **kw) != 0, kw
        assert word in lib.pp_last_error(), (kw, lib.pp_last_error())


def test_report_refusals(built_lib):
    lib = built_lib
    for args, word in (((None, P, 17, 18, 16, P, None), b"null state"), ((P, P, 17, 18, 16, None, None), b"null report"),
                       ((P, None, 17, 18, 16, P, None), b"thresholds not given"), ((P, P, 0, 18, 16, P, None), b"K=0"),
                       ((P, P, 17, 0, 16, P, None), b"J=0"), ((P, P, 17, 65, 16, P, None), b"J=65"),
                       ((P, P, 17, 18, 15, P, None), b"ece_bins=15"), ((P, P, 17, 18, 0, P, None), b"ece_bins=0")):
        assert lib.pp_valmeter_report(*args) != 0, args
        assert word in lib.pp_last_error(), (args, lib.pp_last_error())


def test_state_words_follow_the_header(built_lib):
    lib = built_lib
    for K, J in ((1, 1), (17, 18), (133, 64), (2, 7)):
        words = lib.pp_valmeter_state_words(K, J)
        assert words == K * (9 * 1024 + 4 * J + 19) + 3 + 5 + 15 == vr.state_words(K, J)
    assert lib.pp_valmeter_state_words(18, 18) - lib.pp_valmeter_state_words(17, 18) == 9 * 1024 + 4 * 18 + 19
    assert lib.pp_valmeter_state_words(17, 19) - lib.pp_valmeter_state_words(17, 18) == 4 * 17
    for K, J in ((0, 18), (17, 0), (17, 65), (-1, 1)):
        assert lib.pp_valmeter_state_words(K, J) < 0 and b"bad" in lib.pp_last_error()


def test_python_layout_matches(built_lib):
    from probpose_pytorch_amd import valmeter
    for K, J in ((1, 1), (17, 18), (133, 64)):
        lay = valmeter.state_layout(K, J)
        assert lay["words"][0] == built_lib.pp_valmeter_state_words(K, J)
        ref = vr.empty_state(K, J)
        assert [n for n in lay if n != "words"] == list(ref)
        assert all(lay[n][1] == ref[n].shape for n in ref)


def test_meter_fails_loudly_without_gpu():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from probpose_pytorch_amd import ValidationMeter, _lib
    z = torch.zeros((2, 3))
    with pytest.raises(_lib.HipExtensionError):
        ValidationMeter(None).update_heads(z, z, z, z, z, z, z, z, z)
