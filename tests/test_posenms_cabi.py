"""CPU tests of the PoseNMS boundary: pp_posenms and pp_posenms_rescore refuse bad arguments on the host, with a
message, before anything is launched, and return 0 for empty batches; none of this needs a GPU (the device pointers
are never dereferenced on the host, so made-up addresses stand in for them)."""
import numpy as np

HARD, GAUSSIAN, LINEAR = 0, 1, 2
DEVICE = dict(off=0x10000, kpts=0x20000, vis=0x30000, area=0x40000, scores=0x50000, vars=0x60000,
              out_scores=0x70000, keep=0x80000, counts=0x90000)


def _nms(lib, host_off=(0, 3, 3, 10), n_img=None, K=17, Dtot=None, mode=HARD, oks_thr=0.9, vis_thr=0.2, max_dets=20,
         null=(), no_host=False):
    off = np.asarray(host_off, dtype=np.int64)
    n_img = len(off) - 1 if n_img is None else n_img
    Dtot = int(off[-1]) if Dtot is None else Dtot
    p = dict(DEVICE)
    for k in null:
        p[k] = None
    return lib.pp_posenms(n_img, K, Dtot, None if no_host else off.ctypes.data, p["off"], p["kpts"], p["vis"],
                          p["area"], p["scores"], p["vars"], mode, oks_thr, vis_thr, max_dets, p["out_scores"],
                          p["keep"], p["counts"], None)


def test_posenms_refuses_bad_arguments_before_any_launch(built_lib):
    L = built_lib
    for kwargs, word in (
            (dict(host_off=(1, 3, 10)), b"do not start at 0"),
            (dict(host_off=(0, 5, 3, 10)), b"not monotone at image 1"),
            (dict(host_off=(0, 3, 10), Dtot=11), b"the arrays hold 11"),
            (dict(host_off=(0, 3, 10), Dtot=-1), b"Dtot"),
            (dict(host_off=(0, 3, 10), n_img=-1), b"n_img"),
            (dict(host_off=(0, 2, 4099, 4100)), b"image 1 has 4097 detections"),
            (dict(K=0), b"K=0"), (dict(K=-3), b"K=-3"),
            (dict(oks_thr=0.0), b"oks_thr"), (dict(oks_thr=1.0000001), b"oks_thr"), (dict(oks_thr=-0.5), b"oks_thr"),
            (dict(oks_thr=float("nan")), b"oks_thr"),
            (dict(mode=3), b"unknown mode 3"), (dict(mode=-1), b"unknown mode"),
            (dict(max_dets=0), b"max_dets"), (dict(max_dets=-4), b"max_dets"),
            (dict(vis_thr=float("nan")), b"vis_thr"),
            (dict(no_host=True), b"null host offsets"),
            *[(dict(null=(k,)), b"null argument") for k in DEVICE if k != "vis"]):
        rc = _nms(L, **kwargs)
        assert rc != 0 and word in L.pp_last_error(), (kwargs, L.pp_last_error())
    # every refusal also holds for a batch that would launch nothing: the arguments are checked first
    assert _nms(L, host_off=(0,), mode=7) != 0 and b"unknown mode" in L.pp_last_error()


def test_posenms_empty_batches_return_zero(built_lib):
    L = built_lib
    assert _nms(L, host_off=(0,)) == 0, L.pp_last_error()                           # no image
    assert _nms(L, host_off=(0, 0, 0)) == 0, L.pp_last_error()                      # images without detections
    for mode in (HARD, GAUSSIAN, LINEAR):
        assert _nms(L, host_off=(0, 0), mode=mode, oks_thr=1.0, max_dets=1) == 0, L.pp_last_error()
    assert _nms(L, host_off=(0,), null=("vis",), vis_thr=float("nan")) == 0, L.pp_last_error()   # no visibilities


def test_rescore_refuses_bad_arguments_and_takes_an_empty_batch(built_lib):
    L = built_lib
    ks, bs, out = 0x10000, 0x20000, 0x30000
    assert L.pp_posenms_rescore(-1, 17, ks, bs, 0.2, out, None) != 0 and b"M=-1" in L.pp_last_error()
    assert L.pp_posenms_rescore(4, 0, ks, bs, 0.2, out, None) != 0 and b"K=0" in L.pp_last_error()
    assert L.pp_posenms_rescore(4, 17, ks, bs, float("nan"), out, None) != 0 and b"kpt_thr" in L.pp_last_error()
    for args in ((None, bs, out), (ks, None, out), (ks, bs, None)):
        rc = L.pp_posenms_rescore(4, 17, args[0], args[1], 0.2, args[2], None)
        assert rc != 0 and b"null argument" in L.pp_last_error()
    assert L.pp_posenms_rescore(1 << 40, 17, ks, bs, 0.2, out, None) != 0 and b"exceed one grid" in L.pp_last_error()
    assert L.pp_posenms_rescore(0, 17, ks, bs, 0.2, out, None) == 0, L.pp_last_error()


def test_python_binding_names_the_modes():
    from probpose_pytorch_amd import _lib
    assert (_lib.PP_POSENMS_HARD, _lib.PP_POSENMS_SOFT_GAUSSIAN, _lib.PP_POSENMS_SOFT_LINEAR) == (HARD, GAUSSIAN, LINEAR)
    assert _lib.PP_POSENMS_MAX_DETS == 4096
    assert {"pp_posenms", "pp_posenms_rescore"} <= set(_lib.EXPORTS)
    import probpose_pytorch_amd as pkg
    assert {"PoseNMS", "rescore_instances"} <= set(pkg.__all__)
    assert pkg.PoseNMS.__module__ == "probpose_pytorch_amd.posenms" and callable(pkg.rescore_instances)
