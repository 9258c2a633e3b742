"""CPU tests of the PoseTracker boundary: pp_track_oks, pp_track_assign and pp_track_filter refuse bad arguments on the
host, with a message, before anything is launched, and return 0 for what launches nothing; the Python layer validates
without a GPU and raises ``HipExtensionError`` only where a device is really needed.  None of this needs a GPU: the
device pointers are never dereferenced on the host, so made-up addresses stand in for them."""
import numpy as np
import pytest
import torch

DEV = dict(det_stream=0x10000, blocks=0x20000, kpts=0x30000, vis=0x40000, area=0x50000, vars=0x60000, oks=0x70000,
           off=0x80000, ids=0x90000, match_oks=0xa0000, born=0xb0000, slot_of=0xc0000, te=0xd0000, out=0xe0000)


def _ptrs(null):
    p = dict(DEV)
    for k in null:
        p[k] = None
    return p


def _oks(lib, host_off=(0, 3, 3, 10), n_str=None, K=17, T=64, Dtot=None, vis_thr=0.2, null=(), no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    p = _ptrs(null)
    return lib.pp_track_oks(len(off) - 1 if n_str is None else n_str, K, T, int(off[-1]) if Dtot is None else Dtot,
                            None if no_host else off.ctypes.data, p["det_stream"], p["blocks"], p["kpts"], p["vis"],
                            p["area"], p["vars"], vis_thr, p["oks"], None)


def _assign(lib, host_off=(0, 3, 3, 10), n_str=None, K=17, T=64, Dtot=None, match_thr=0.3, max_age=30, t=1.0,
            t_prev=0.5, null=(), no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    p = _ptrs(null)
    return lib.pp_track_assign(len(off) - 1 if n_str is None else n_str, K, T, int(off[-1]) if Dtot is None else Dtot,
                               None if no_host else off.ctypes.data, p["off"], p["blocks"], p["oks"], p["area"],
                               match_thr, max_age, t, t_prev, p["ids"], p["match_oks"], p["born"], p["slot_of"],
                               p["te"], None)


def _filter(lib, K=17, T=64, Dtot=10, vis_thr=0.2, smooth=1, consts=(1.0, 0.05, 1.0), null=()):
    p = _ptrs(null)
    return lib.pp_track_filter(K, T, Dtot, p["det_stream"], p["blocks"], p["kpts"], p["vis"], vis_thr, p["slot_of"],
                               p["born"], p["te"], smooth, *consts, p["out"], None)


BAD_OFFSETS = ((dict(host_off=(1, 3, 10)), b"do not start at 0"),
               (dict(host_off=(0, 5, 3, 10)), b"not monotone at stream 1"),
               (dict(host_off=(0, 3, 10), Dtot=11), b"the arrays hold 11"),
               (dict(host_off=(0, 3, 10), Dtot=-1), b"Dtot"),
               (dict(host_off=(0, 3, 10), n_str=-1), b"n_str"),
               (dict(host_off=(0, 2, 4099, 4100)), b"stream 1 has 4097 detections"),
               (dict(no_host=True), b"null host offsets"),
               (dict(K=0), b"K=0"), (dict(K=-3), b"K=-3"),
               (dict(T=0), b"max_tracks=0"), (dict(T=4097), b"max_tracks=4097"))


def test_oks_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in (*BAD_OFFSETS, (dict(vis_thr=float("nan")), b"vis_thr"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("det_stream", "blocks", "kpts", "area", "vars", "oks")]):
        rc = _oks(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_oks" in L.pp_last_error(), (kwargs,
                                                                                              L.pp_last_error())
    assert _oks(L, host_off=(0,), K=0) != 0 and b"K=0" in L.pp_last_error()     # checked even when nothing would launch


def test_assign_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in (*BAD_OFFSETS,
                         (dict(match_thr=1.0), b"match_thr"), (dict(match_thr=-0.1), b"match_thr"),
                         (dict(match_thr=float("nan")), b"match_thr"),
                         (dict(max_age=-1), b"max_age=-1"),
                         (dict(t=0.5, t_prev=0.5), b"te <= 0"), (dict(t=0.4, t_prev=0.5), b"te <= 0"),
                         (dict(t=float("nan")), b"te <= 0"), (dict(t=float("inf")), b"te <= 0"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("off", "blocks", "oks", "area", "ids", "match_oks", "born", "slot_of", "te")]):
        rc = _assign(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_assign" in L.pp_last_error(), (kwargs,
                                                                                                 L.pp_last_error())
    assert _assign(L, host_off=(0,), match_thr=2.0) != 0 and b"match_thr" in L.pp_last_error()


def test_filter_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in ((dict(K=0), b"K=0"), (dict(T=0), b"max_tracks=0"), (dict(T=5000), b"max_tracks=5000"),
                         (dict(Dtot=-2), b"Dtot"), (dict(vis_thr=float("nan")), b"vis_thr"),
                         (dict(consts=(0.0, 0.05, 1.0)), b"min_cutoff"), (dict(consts=(1.0, -0.1, 1.0)), b"beta"),
                         (dict(consts=(1.0, 0.05, float("inf"))), b"d_cutoff"),
                         (dict(consts=(float("nan"), 0.05, 1.0)), b"min_cutoff"),
                         *[(dict(null=(k,)), b"null argument")
                           for k in ("det_stream", "blocks", "kpts", "slot_of", "born", "te", "out")]):
        rc = _filter(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_filter" in L.pp_last_error(), (kwargs,
                                                                                                 L.pp_last_error())


def test_what_launches_nothing_returns_zero(built_lib):
    L = built_lib
    assert _oks(L, host_off=(0,)) == 0, L.pp_last_error()                       # no stream
    assert _oks(L, host_off=(0, 0, 0)) == 0, L.pp_last_error()                  # streams without detections
    assert _oks(L, host_off=(0,), null=("vis",), vis_thr=float("nan")) == 0, L.pp_last_error()
    assert _assign(L, host_off=(0,), t_prev=float("-inf")) == 0, L.pp_last_error()      # the first call's t_prev
    assert _assign(L, host_off=(0,), match_thr=0.0, max_age=0) == 0, L.pp_last_error()
    assert _filter(L, Dtot=0) == 0, L.pp_last_error()
    assert _filter(L, Dtot=0, smooth=0, consts=(0.0, -1.0, 0.0), null=("vis",)) == 0, L.pp_last_error()


def test_state_bytes_is_the_python_layout(built_lib):
    from probpose_pytorch_amd import tracker
    L = built_lib
    for T, K in ((1, 1), (16, 17), (65, 17), (130, 1), (4096, 133), (3, 5)):
        lay = tracker.state_layout(T, K)
        assert L.pp_track_state_bytes(T, K) == lay["bytes"] and lay["bytes"] % 8 == 0
        assert all(at % 8 == 0 for name, (at, _, _) in ((n, v) for n, v in lay.items() if n != "bytes"))
    assert lay["id"][0] == 0 and lay["age"][1] == np.int32 and lay["init"][2] == (3, 5)
    assert L.pp_track_state_bytes(0, 17) < 0 and b"max_tracks=0" in L.pp_last_error()
    assert L.pp_track_state_bytes(4097, 17) < 0 and L.pp_track_state_bytes(16, 0) < 0


def test_constants_and_exports():
    from probpose_pytorch_amd import _lib
    assert _lib.PP_TRACK_MAX_TRACKS >= 256 and _lib.PP_TRACK_MAX_TRACKS == 64 * 64 and _lib.PP_TRACK_MAX_DETS == 4096
    assert {"pp_track_state_bytes", "pp_track_oks", "pp_track_assign", "pp_track_filter"} <= set(_lib.EXPORTS)
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    assert f"#define PP_TRACK_MAX_TRACKS {_lib.PP_TRACK_MAX_TRACKS}\n" in header
    assert f"#define PP_TRACK_MAX_DETS {_lib.PP_TRACK_MAX_DETS}\n" in header
    import probpose
    import probpose_pytorch_amd as pkg
    assert {"PoseTracker", "OneEuro"} <= set(pkg.__all__)
    assert pkg.PoseTracker.__module__ == "probpose_pytorch_amd.tracker" and pkg.OneEuro is probpose.tracker.OneEuro
    assert probpose.tracker.PoseTracker is pkg.PoseTracker


def test_one_euro_is_validated():
    from probpose_pytorch_amd import OneEuro
    e = OneEuro()
    assert (e.min_cutoff, e.beta, e.d_cutoff) == (1.0, 0.05, 1.0) and "beta=0.05" in repr(e)
    assert OneEuro(beta=0).beta == 0.0
    for kwargs, word in ((dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=-1.0), "min_cutoff"),
                         (dict(d_cutoff=0.0), "d_cutoff"), (dict(beta=-0.01), "beta"),
                         (dict(min_cutoff=float("nan")), "min_cutoff"), (dict(beta=float("inf")), "beta"),
                         (dict(d_cutoff=float("inf")), "d_cutoff")):
        with pytest.raises(ValueError, match=word):
            OneEuro(**kwargs)


def test_constructor_and_update_validate_without_a_gpu():
    from probpose_pytorch_amd import OneEuro, PoseTracker, _lib
    K = 3
    sig = np.full(K, 0.05)
    for kwargs, word in ((dict(match_thr=1.0), "match_thr"), (dict(match_thr=-0.1), "match_thr"),
                         (dict(max_age=-1), "max_age"), (dict(max_tracks=0), "max_tracks"),
                         (dict(max_tracks=_lib.PP_TRACK_MAX_TRACKS + 1), "max_tracks"),
                         (dict(vis_thr=float("nan")), "vis_thr"), (dict(smooth=(1.0, 0.05, 1.0)), "smooth"),
                         (dict(fps=0.0), "fps")):
        with pytest.raises(ValueError, match=word):
            PoseTracker(sig, **kwargs)
    with pytest.raises(ValueError, match="sigmas"):
        PoseTracker([])
    tr = PoseTracker(sig, smooth=OneEuro(), max_tracks=_lib.PP_TRACK_MAX_TRACKS, match_thr=0.0, max_age=0)
    kp, ones = np.zeros((5, K, 2)), np.ones(5)
    with pytest.raises(ValueError, match="keypoints: expected"):
        tr.update(kp[:, :2], ones, ones)
    with pytest.raises(ValueError, match="keypoints: expected"):
        tr.update(np.zeros((5, K, 4)), ones, ones)
    with pytest.raises(ValueError, match=r"areas: expected \[5\]"):
        tr.update(kp, ones[:4], ones)
    with pytest.raises(ValueError, match=r"scores: expected \[5\]"):
        tr.update(kp, ones, np.ones((5, 1)))
    with pytest.raises(ValueError, match=r"kpt_scores: expected \[5, 3\]"):
        tr.update(kp, ones, ones, np.ones((5, 2)))
    with pytest.raises(ValueError, match=r"stream_ids: expected \[5\]"):
        tr.update(kp, ones, ones, stream_ids=[0, 1])
    with pytest.raises(ValueError, match="stream_ids: stream 7 is not in streams"):
        tr.update(kp, ones, ones, stream_ids=[0, 0, 7, 1, 1], streams=[0, 1])
    with pytest.raises(ValueError, match="scores: expected a float dtype"):
        tr.update(kp, ones, ones.astype(np.int64))
    with pytest.raises(ValueError, match="areas: expected a float dtype"):
        tr.update(torch.zeros((5, K, 2)), torch.ones(5, dtype=torch.int32), torch.ones(5))
    with pytest.raises(ValueError, match="vis_thr: needs visibilities"):
        PoseTracker(sig, vis_thr=0.2).update(kp, ones, ones)
    with pytest.raises(ValueError, match="t: "):
        tr.update(kp, ones, ones, t=float("nan"))
    M = _lib.PP_TRACK_MAX_DETS + 1
    with pytest.raises(ValueError, match=f"stream_ids: stream 'cam' has {M} detections"):
        tr.update(np.zeros((M, K, 2)), np.ones(M), np.ones(M), stream_ids=["cam"] * M)
    # a well-formed call on host arrays: the device is really needed now
    with pytest.raises(_lib.HipExtensionError):
        tr.update(kp, ones, ones)
    with pytest.raises(KeyError):
        tr.tracks(0)
    assert tr.overflow.shape == (0,) and tr.overflow.dtype == torch.int64
    tr.reset()
    tr.reset("never seen")
