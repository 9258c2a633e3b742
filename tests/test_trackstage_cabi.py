"""CPU tests of the boundary of PoseTracker's motion prediction and two-stage association: pp_track_oks_predicted and
pp_track_assign_staged are in the header, the library and the binding with one signature; each refuses bad arguments on
the host, naming them, before anything is launched (through ctypes, with made-up device addresses that are never
dereferenced); the constructor and the command line refuse what they must.  None of this needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

DEV = dict(det_stream=0x10000, blocks=0x20000, kpts=0x30000, vis=0x40000, area=0x50000, vars=0x60000, oks=0x70000,
           off=0x80000, ids=0x90000, match_oks=0xa0000, born=0xb0000, slot_of=0xc0000, te=0xd0000, score=0xe0000,
           dropped=0xf0000)
NAN, INF = float("nan"), float("inf")


def _oks(lib, host_off=(0, 3, 3, 10), n_str=None, K=17, T=64, Dtot=None, vis_thr=0.2, t=1.0, max_dt=INF, null=(),
         no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    return lib.pp_track_oks_predicted(len(off) - 1 if n_str is None else n_str, K, T,
                                      int(off[-1]) if Dtot is None else Dtot, None if no_host else off.ctypes.data,
                                      p["det_stream"], p["blocks"], p["kpts"], p["vis"], p["area"], p["vars"], vis_thr,
                                      t, max_dt, p["oks"], None)


def _staged(lib, host_off=(0, 3, 3, 10), n_str=None, K=17, T=64, Dtot=None, match_thr=0.3, high_thr=0.5,
            low_match_thr=0.3, low_max_age=0, birth_thr=0.6, optimal=0, max_age=30, t=1.0, t_prev=0.5, null=(),
            no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    return lib.pp_track_assign_staged(len(off) - 1 if n_str is None else n_str, K, T,
                                      int(off[-1]) if Dtot is None else Dtot, None if no_host else off.ctypes.data,
                                      p["off"], p["blocks"], p["oks"], p["area"], p["score"], match_thr, high_thr,
                                      low_match_thr, low_max_age, birth_thr, optimal, max_age, t, t_prev, p["ids"],
                                      p["match_oks"], p["born"], p["slot_of"], p["te"], p["dropped"], None)


BAD_OFFSETS = ((dict(host_off=(1, 3, 10)), b"do not start at 0"),
               (dict(host_off=(0, 5, 3, 10)), b"not monotone at stream 1"),
               (dict(host_off=(0, 3, 10), Dtot=11), b"the arrays hold 11"),
               (dict(host_off=(0, 3, 10), Dtot=-1), b"Dtot"),
               (dict(host_off=(0, 3, 10), n_str=-1), b"n_str"),
               (dict(host_off=(0, 2, 4099, 4100)), b"stream 1 has 4097 detections"),
               (dict(no_host=True), b"null host offsets"),
               (dict(K=0), b"K=0"), (dict(T=0), b"max_tracks=0"), (dict(T=4097), b"max_tracks=4097"))


def test_the_predicted_oks_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in (*BAD_OFFSETS, (dict(vis_thr=NAN), b"vis_thr"),
                         (dict(t=NAN), b"t=nan is not finite"), (dict(t=INF), b"is not finite"),
                         (dict(t=-INF), b"is not finite"),
                         (dict(max_dt=-0.5), b"max_dt=-0.5 is negative"), (dict(max_dt=NAN), b"max_dt"),
                         (dict(max_dt=-INF), b"max_dt"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("det_stream", "blocks", "kpts", "area", "vars", "oks")]):
        rc = _oks(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_oks_predicted" in L.pp_last_error(), (
            kwargs, L.pp_last_error())
    # what launches nothing returns 0; the checks run even then
    assert _oks(L, host_off=(0,)) == 0 and _oks(L, host_off=(0, 0, 0), max_dt=0.0) == 0, L.pp_last_error()
    assert _oks(L, host_off=(0,), null=("vis",), vis_thr=NAN) == 0, L.pp_last_error()
    assert _oks(L, host_off=(0,), max_dt=-1.0) != 0 and b"max_dt" in L.pp_last_error()
    assert _oks(L, host_off=(0,), t=NAN) != 0 and b"t=" in L.pp_last_error()


def test_the_staged_assign_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in (*BAD_OFFSETS,
                         (dict(match_thr=1.0), b"match_thr"), (dict(match_thr=NAN), b"match_thr"),
                         (dict(max_age=-1), b"max_age=-1"),
                         (dict(t=0.5, t_prev=0.5), b"te <= 0"), (dict(t=NAN), b"te <= 0"), (dict(t=INF), b"te <= 0"),
                         (dict(high_thr=NAN), b"high_thr is not a number"),
                         (dict(birth_thr=NAN), b"birth_thr is not a number"),
                         (dict(low_match_thr=NAN), b"low_match_thr"), (dict(low_match_thr=1.0), b"low_match_thr=1"),
                         (dict(low_match_thr=-0.1), b"low_match_thr=-0.1 is outside [0, 1)"),
                         (dict(low_max_age=-1), b"low_max_age=-1"),
                         (dict(optimal=2), b"optimal=2"), (dict(optimal=-1), b"optimal=-1"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("off", "blocks", "oks", "area", "score", "ids", "match_oks", "born", "slot_of",
                                     "te", "dropped")],
                         # the limits of the optimal stages
                         (dict(optimal=1, T=257), b"max_tracks=257 is above PP_TRACK_OPT_MAX = 256"),
                         (dict(optimal=1, host_off=(0, 2, 259, 300)),
                          b"stream 1 has 257 detections, more than PP_TRACK_OPT_MAX"),
                         (dict(optimal=1, host_off=(0, 257), T=256), b"stream 0 has 257 detections")):
        rc = _staged(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_assign_staged" in L.pp_last_error(), (
            kwargs, L.pp_last_error())
    # greedy stages take what pp_track_assign takes; -inf thresholds are the single-stage rule and are allowed
    for kwargs in (dict(), dict(T=257), dict(host_off=(0, 257)), dict(optimal=1, T=256),
                   dict(high_thr=-INF, birth_thr=-INF), dict(high_thr=INF), dict(low_match_thr=0.0, low_max_age=7),
                   dict(t_prev=-INF)):
        assert _staged(L, **{"host_off": (0,), **kwargs}, n_str=0, Dtot=0) == 0, (kwargs, L.pp_last_error())
    assert _staged(L, host_off=(0,), low_max_age=-3) != 0 and b"low_max_age=-3" in L.pp_last_error()
    assert _staged(L, host_off=(0,), optimal=1, T=300) != 0 and b"PP_TRACK_OPT_MAX" in L.pp_last_error()


def _c_types(decl):
    """The ctypes of a C declaration's parameters, by the header's conventions."""
    out = []
    for param in decl.split(","):
        param = param.strip()
        out.append(C.c_void_p if "*" in param else {"int": C.c_int, "double": C.c_double,
                                                    "long long": C.c_longlong}[param.rsplit(" ", 1)[0]])
    return out


def test_header_export_and_binding_agree(built_lib):
    from probpose_pytorch_amd import _lib
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    for name in ("pp_track_oks_predicted", "pp_track_assign_staged"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in the header"
        res, args = _lib._SIGNATURES[name]
        assert res is C.c_int and args == _c_types(" ".join(m.group(1).split())), name
        assert name in _lib.EXPORTS and getattr(built_lib, name).argtypes == args
    # the predicted entry is pp_track_oks plus (t, max_dt) before the output
    oks, pred = _lib._SIGNATURES["pp_track_oks"][1], _lib._SIGNATURES["pp_track_oks_predicted"][1]
    assert pred == oks[:-2] + [C.c_double, C.c_double] + oks[-2:]
    # the staged entry is pp_track_assign plus score, four thresholds, the flag and dropped
    assign, staged = _lib._SIGNATURES["pp_track_assign"][1], _lib._SIGNATURES["pp_track_assign_staged"][1]
    assert len(staged) == len(assign) + 7 and staged[:9] == assign[:9] and staged[-1] is C.c_void_p


def test_the_constructor_refuses_what_it_must():
    from probpose_pytorch_amd import OneEuro, PoseTracker
    sig, euro = np.full(3, 0.05), OneEuro()
    for kwargs, word in ((dict(predict=True), "predict: needs smooth"),
                         (dict(predict_max_dt=0.1, smooth=euro), "predict_max_dt"),
                         (dict(predict=True, smooth=euro, predict_max_dt=-0.1), "predict_max_dt"),
                         (dict(predict=True, smooth=euro, predict_max_dt=NAN), "predict_max_dt"),
                         (dict(predict=True, smooth=euro, predict_max_dt=INF), "predict_max_dt"),
                         (dict(low_match_thr=0.2), "low_match_thr: given without high_thr"),
                         (dict(low_max_age=1), "low_max_age: given without high_thr"),
                         (dict(birth_thr=0.5, low_max_age=1), "low_max_age"),
                         (dict(birth_thr=0.5, low_match_thr=0.1), "low_match_thr"),
                         (dict(high_thr=NAN), "high_thr"), (dict(high_thr=INF), "high_thr"),
                         (dict(high_thr=-INF), "high_thr"), (dict(birth_thr=NAN), "birth_thr"),
                         (dict(birth_thr=INF), "birth_thr"), (dict(high_thr=0.5, low_match_thr=NAN), "low_match_thr"),
                         (dict(high_thr=0.5, low_match_thr=1.0), "low_match_thr: 1.0 is outside"),
                         (dict(high_thr=0.5, low_match_thr=-0.1), "low_match_thr"),
                         (dict(high_thr=0.5, low_max_age=-1), "low_max_age")):
        with pytest.raises(ValueError, match=word):
            PoseTracker(sig, **kwargs)
    tr = PoseTracker(sig)
    assert (tr.predict, tr.high_thr, tr.birth_thr, tr.low_max_age) == (False, None, None, 0)
    tr = PoseTracker(sig, match_thr=0.4, high_thr=0.5)
    assert (tr.high_thr, tr.birth_thr, tr.low_match_thr, tr.low_max_age) == (0.5, 0.5, 0.4, 0)
    tr = PoseTracker(sig, birth_thr=0.6)
    assert tr.high_thr is None and tr.birth_thr == 0.6
    tr = PoseTracker(sig, smooth=euro, predict=True, predict_max_dt=0, high_thr=0.5, low_match_thr=0.0, low_max_age=3,
                     birth_thr=0.2, assign="optimal")
    assert (tr.predict, tr.predict_max_dt, tr.low_match_thr, tr.low_max_age, tr.birth_thr) == (True, 0.0, 0.0, 3, 0.2)
    assert PoseTracker(sig, smooth=euro, predict=True).predict_max_dt == INF
    with pytest.raises(TypeError):
        PoseTracker(sig, 0.3, 30, 64, None, euro, 30.0, "greedy", True)         # keyword-only


def test_the_flags(capsys):
    from probpose_pytorch_amd import inference
    for flags, word in ((["--predict"], "--predict needs --track"), (["--high-thr", "0.5"], "--high-thr needs --track"),
                        (["--low-match-thr", "0.2"], "--low-match-thr needs --track"),
                        (["--birth-thr", "0.6"], "--birth-thr needs --track"),
                        (["--track", "--predict", "0.1", "--high-thr", "0.5", "--low-match-thr", "0.2", "--birth-thr",
                          "0.6"], "error: --track needs --frames"),
                        (["--high-thr", "high"], "--high-thr")):
        with pytest.raises(SystemExit):
            inference.main(flags)
        assert word in capsys.readouterr().err, flags


def test_the_flags_are_checked_with_the_frames_given(tmp_path, capsys):
    from probpose_pytorch_amd import inference
    frames = tmp_path / "frames"
    frames.mkdir()
    (tmp_path / "boxes.json").write_text("{}")
    base = ["--track", "--frames", str(frames), "--boxes-json", str(tmp_path / "boxes.json"), "--output",
            str(tmp_path / "out")]
    for flags, word in ((["--predict"], "--predict needs --smooth"),
                        (["--smooth", "--predict", "-1"], "--predict: -1.0 is negative"),
                        (["--low-match-thr", "0.2"], "--low-match-thr needs --high-thr"),
                        (["--high-thr", "0.5", "--low-match-thr", "1.5"], "--low-match-thr: 1.5 is outside"),
                        (["--high-thr", "nan"], "--high-thr: nan is not finite"),
                        (["--birth-thr", "inf"], "--birth-thr: inf is not finite"),
                        (["--smooth", "--predict", "0.1", "--high-thr", "0.5", "--birth-thr", "0.6"],
                         "holds no file")):          # everything accepted: the empty folder is what is refused
        with pytest.raises(SystemExit):
            inference.main(base + flags)
        assert word in capsys.readouterr().err, flags
