"""Host-side refusals of the HeadCalibration entry points through the built library: they come before any launch, so no
GPU is needed."""
import ctypes as C

P = 0x1000      # a non-null pointer the refusals never dereference


def _fit(lib, state=P, K=17, J=18, min_count=1000, blocks=P, table=P, row_of=P):
    return lib.pp_calib_fit(state, K, J, min_count, blocks, table, row_of, None)


def _apply(lib, aux_in=P, aux_out=P, B=4, K=17, table=P, row_of=P):
    return lib.pp_calib_apply(aux_in, aux_out, B, K, table, row_of, None)


def _score(lib, state=P, K=17, J=18, table=P, row_of=P, ece_bins=16, report=P):
    return lib.pp_calib_score(state, K, J, table, row_of, ece_bins, report, None)


def _refused(lib, fn, cases):
    for kw, word in cases:
        assert fn(lib, **kw) != 0, kw
        assert word in lib.pp_last_error(), (kw, lib.pp_last_error())


def test_fit_refusals(built_lib):
    _refused(built_lib, _fit, ((dict(K=0), b"K=0"), (dict(K=-3), b"K=-3"), (dict(J=0), b"J=0"), (dict(J=65), b"J=65"),
                               (dict(min_count=0), b"min_count=0"), (dict(min_count=-5), b"min_count=-5"),
                               (dict(state=None), b"null state"), (dict(blocks=None), b"null output"),
                               (dict(table=None), b"null output"), (dict(row_of=None), b"null output")))


def test_apply_refusals(built_lib):
    _refused(built_lib, _apply, ((dict(K=0), b"K=0"), (dict(B=0), b"B=0"), (dict(B=-1), b"B=-1"),
                                 (dict(B=1 << 30), b"3*B*K < 2^31"), (dict(aux_in=None), b"null aux"),
                                 (dict(aux_out=None), b"null aux"), (dict(table=None), b"null calibration"),
                                 (dict(row_of=None), b"null calibration"),
                                 # [3][4][17] floats are 816 bytes: 4 bytes apart overlaps in part, 816 apart does not
                                 (dict(aux_out=P + 4), b"overlap in part"), (dict(aux_in=P + 812), b"overlap in part")))


def test_score_refusals(built_lib):
    _refused(built_lib, _score, ((dict(K=0), b"K=0"), (dict(J=0), b"J=0"), (dict(J=65), b"J=65"),
                                 (dict(ece_bins=15), b"ece_bins=15"), (dict(ece_bins=0), b"ece_bins=0"),
                                 (dict(ece_bins=2048), b"ece_bins=2048"), (dict(state=None), b"null state"),
                                 (dict(table=None), b"null calibration"), (dict(row_of=None), b"null calibration"),
                                 (dict(report=None), b"null report")))


def test_signatures_are_bound(built_lib):
    from probpose_pytorch_amd import _lib
    for name in ("pp_calib_fit", "pp_calib_apply", "pp_calib_score"):
        assert name in _lib.EXPORTS and getattr(built_lib, name).restype is C.c_int
    assert _lib._SIGNATURES["pp_calib_fit"][1][3] is C.c_longlong       # min_count is 64-bit
