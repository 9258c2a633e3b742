"""CPU tests of the track-driven boxes' boundary: pp_track_boxes refuses bad arguments on the host, with a message that
names the argument, before anything is launched; ``PoseTracker.propose_boxes`` and ``PoseFollower`` validate without a
GPU and raise ``HipExtensionError`` only where a device is really needed.  Made-up addresses stand in for the device
pointers: the host never dereferences them."""
import numpy as np
import pytest

DEV = dict(blocks=0x10000, frame_wh=0x20000, sup_off=0x30000, sup_boxes=0x40000, boxes=0x50000, ids=0x60000,
           scores=0x70000, status=0x80000)
INF, NAN = float("inf"), float("nan")


def _boxes(lib, n_str=2, K=17, T=8, t=1.0, use_vis=1, vis_thr=0.3, smooth=1, extrapolate=1, max_dt=INF, max_age=0,
           min_keypoints=3, pad=1.25, min_side=2.0, aspect=0.0, iou_thr=0.3, host_off=(0, 1, 3), null=()):
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    off = None if host_off is None else np.asarray(host_off, dtype=np.int64)
    return lib.pp_track_boxes(n_str, K, T, p["blocks"], t, use_vis, vis_thr, smooth, extrapolate, max_dt, max_age,
                              min_keypoints, pad, min_side, aspect, p["frame_wh"], None if off is None else
                              off.ctypes.data, p["sup_off"], p["sup_boxes"], iou_thr, p["boxes"], p["ids"],
                              p["scores"], p["status"], None)


def test_boxes_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in ((dict(n_str=-1), b"n_str"), (dict(K=0), b"K=0"), (dict(T=0), b"max_tracks=0"),
                         (dict(T=4097), b"max_tracks=4097"),
                         (dict(t=NAN), b"t="), (dict(t=INF), b"t="),
                         (dict(vis_thr=NAN), b"vis_thr"),
                         (dict(max_dt=-0.1), b"max_dt"), (dict(max_dt=NAN), b"max_dt"),
                         (dict(max_age=-1), b"max_age=-1"), (dict(min_keypoints=0), b"min_keypoints=0"),
                         (dict(pad=0.0), b"pad"), (dict(pad=INF), b"pad"), (dict(pad=NAN), b"pad"),
                         (dict(min_side=0.0), b"min_side"), (dict(min_side=-2.0), b"min_side"),
                         (dict(min_side=INF), b"min_side"),
                         (dict(aspect=-0.5), b"aspect"), (dict(aspect=INF), b"aspect"), (dict(aspect=NAN), b"aspect"),
                         (dict(iou_thr=-0.01), b"iou_thr"), (dict(iou_thr=1.01), b"iou_thr"),
                         (dict(iou_thr=NAN), b"iou_thr"),
                         (dict(host_off=(1, 1, 3)), b"sup_off does not start at 0"),
                         (dict(host_off=(0, 3, 1)), b"sup_off is not ascending at stream 1"),
                         (dict(null=("sup_boxes",)), b"sup_boxes is null"),
                         (dict(null=("sup_off",)), b"sup_off"), (dict(host_off=None), b"sup_off"),
                         *[(dict(null=(k,)), b"null argument") for k in ("blocks", "boxes", "ids", "scores",
                                                                          "status")]):
        rc = _boxes(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error() and b"pp_track_boxes" in L.pp_last_error(), (kwargs,
                                                                                                L.pp_last_error())
    # checked even when nothing would launch
    assert _boxes(L, n_str=0, host_off=(0,), pad=-1.0) != 0 and b"pad" in L.pp_last_error()


def test_what_launches_nothing_returns_zero(built_lib):
    L = built_lib
    assert _boxes(L, n_str=0, host_off=(0,)) == 0, L.pp_last_error()
    assert _boxes(L, n_str=0, host_off=None, null=("sup_off", "sup_boxes", "frame_wh", "blocks", "boxes", "ids",
                                                   "scores", "status")) == 0, L.pp_last_error()
    assert _boxes(L, n_str=0, host_off=(0,), use_vis=0, vis_thr=NAN, max_dt=0.0, aspect=0.75, iou_thr=1.0) == 0


def test_constants_and_exports():
    import probpose_pytorch_amd as pkg
    from probpose_pytorch_amd import _lib
    assert "pp_track_boxes" in _lib.EXPORTS
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    for n, name in enumerate(("FREE", "PROPOSED", "OLD", "FEW", "OUTSIDE", "SUPPRESSED")):
        assert getattr(_lib, "PP_TRACK_BOX_" + name) == n and f"#define PP_TRACK_BOX_{name} {n}\n" in header
    assert "PoseFollower" in pkg.__all__ and pkg.PoseFollower.__module__ == "probpose_pytorch_amd.follow"


def test_propose_boxes_and_the_follower_validate_without_a_gpu():
    import torch
    from probpose_pytorch_amd import PoseFollower, PoseTracker, _lib
    tr = PoseTracker(np.full(3, 0.05), vis_thr=0.3)
    for kwargs, word in ((dict(t=NAN), "t: "), (dict(t=-INF), "t: "), (dict(pad=0.0), "pad"), (dict(pad=INF), "pad"),
                         (dict(min_side=0.0), "min_side"), (dict(aspect=0.0), "aspect"), (dict(aspect=-1.0), "aspect"),
                         (dict(min_keypoints=0), "min_keypoints"), (dict(max_age=-1), "max_age"),
                         (dict(max_dt=-1.0), "max_dt"), (dict(max_dt=NAN), "max_dt"), (dict(iou_thr=1.5), "iou_thr"),
                         (dict(iou_thr=NAN), "iou_thr"),
                         (dict(suppress=(np.zeros((2, 3)), None)), r"suppress: expected boxes \[n, 4\]"),
                         (dict(suppress=(np.zeros((2, 4)), None)), "suppress: stream_ids are needed"),
                         (dict(suppress=(np.zeros((2, 4)), [0])), "suppress: expected stream_ids"),
                         (dict(suppress=(np.zeros((1, 4)), ["cam"])), "suppress: stream 'cam' is not in streams"),
                         (dict(frame_size=(0.0, 10.0)), "frame_size"), (dict(frame_size=(10.0,)), "frame_size"),
                         (dict(frame_size={"cam": (NAN, 10.0)}), "frame_size")):
        with pytest.raises(ValueError, match=word):
            tr.propose_boxes(**kwargs)
    with pytest.raises(KeyError):
        tr.propose_boxes(streams=["never seen"])
    with pytest.raises(ValueError, match="named twice"):
        tr.propose_boxes(streams=[0, 0])
    calls, t_prev = tr._calls, tr._t_prev
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipExtensionError):         # a well-formed call: the device is really needed now
            tr.propose_boxes()
        with pytest.raises(_lib.HipExtensionError):
            PoseFollower(tr, lambda frame, boxes: None).step(None, np.array([[0.0, 0.0, 4.0, 4.0]]))
    assert (tr._calls, tr._t_prev) == (calls, t_prev)
    with pytest.raises(ValueError, match="vis_thr"):
        PoseFollower(PoseTracker(np.full(3, 0.05)), lambda frame, boxes: None)
    with pytest.raises(ValueError, match="estimate"):
        PoseFollower(tr, None)
    with pytest.raises(ValueError, match="min_keypoints"):
        PoseFollower(tr, lambda frame, boxes: None, min_keypoints=0)
