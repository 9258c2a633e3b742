"""CPU tests of pp_cocoeval_exoks' refusals: null pointers, a presence threshold that is not in [0, 1] and broken
offsets come back as errors with a message before anything is launched (there is no device here to launch on)."""
import numpy as np

GOOD = np.array([[0, 2, 5], [0, 1, 4], [0, 2, 11]], dtype=np.int64)
P = 0x1000


def _exoks(L, offs, n_img=2, K=17, tot=(5, 4, 11), thr=0.5, null=None):
    """The ten pointers after host_offs: offs, det_kpts, gt_kpts, gt_bbox, gt_area, gt_flags, vars, det_presence,
    gt_window | presence_thr | oks."""
    args = [P] * 10
    if null is not None:
        args[null] = None
    return L.pp_cocoeval_exoks(n_img, K, *tot, offs.ctypes.data if offs is not None else None, *args[:9], thr,
                               args[9], None)


def test_exoks_is_declared_exported_and_bound(built_lib):
    from probpose_pytorch_amd import _lib
    assert "pp_cocoeval_exoks" in _lib.EXPORTS and hasattr(built_lib, "pp_cocoeval_exoks")


def test_null_pointers_are_refused(built_lib):
    L = built_lib
    for i in range(10):
        assert _exoks(L, GOOD, null=i) != 0 and b"pp_cocoeval_exoks: null argument" in L.pp_last_error(), i
    assert _exoks(L, None) != 0 and b"null host offsets" in L.pp_last_error()
    for i in (7, 8):            # det_presence, gt_window: refused without work as well, like every other pointer
        assert _exoks(L, np.zeros((3, 1), dtype=np.int64), n_img=0, tot=(0, 0, 0), null=i) != 0


def test_a_bad_threshold_is_refused(built_lib):
    L = built_lib
    for thr in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf"), float("-inf")):
        assert _exoks(L, GOOD, thr=thr) != 0 and b"presence_thr" in L.pp_last_error(), thr
    # ... before the offsets are looked at, and also when there is nothing to do
    assert _exoks(L, np.zeros((3, 1), dtype=np.int64), n_img=0, tot=(0, 0, 0), thr=1.5) != 0
    assert b"presence_thr" in L.pp_last_error()


def test_broken_offsets_are_refused(built_lib):
    L = built_lib
    for bad, word in ((np.array([[0, 3, 2], [0, 1, 4], [0, 3, 0]], dtype=np.int64), b"not monotone"),
                      (np.array([[0, 2, 5], [0, 4, 1], [0, 8, -1]], dtype=np.int64), b"not monotone"),
                      (np.array([[0, 2, 5], [0, 1, 4], [0, 3, 11]], dtype=np.int64), b"OKS offsets"),
                      (np.array([[1, 2, 5], [0, 1, 4], [0, 1, 10]], dtype=np.int64), b"start at 0")):
        assert _exoks(L, bad) != 0 and word in L.pp_last_error(), L.pp_last_error()
        assert b"pp_cocoeval_exoks" in L.pp_last_error()
    assert _exoks(L, GOOD, tot=(6, 4, 11)) != 0 and b"offsets end" in L.pp_last_error()
    assert _exoks(L, GOOD, K=0) != 0 and b"K=0" in L.pp_last_error()
    assert _exoks(L, GOOD, n_img=-1) != 0 and b"n_img" in L.pp_last_error()


def test_nothing_to_do_returns_zero_without_a_launch(built_lib):
    """n_img = 0, and images whose D x G products are all 0: status 0 (the pointers are dummies; a launch would have
    failed without a device), at both ends of the threshold's range."""
    L = built_lib
    for thr in (0.0, 0.5, 1.0):
        assert _exoks(L, np.zeros((3, 1), dtype=np.int64), n_img=0, tot=(0, 0, 0), thr=thr) == 0, L.pp_last_error()
    empty = np.array([[0, 3, 3], [0, 0, 4], [0, 0, 0]], dtype=np.int64)      # (3, 0) and (0, 4)
    assert _exoks(L, empty, tot=(3, 4, 0)) == 0, L.pp_last_error()
    # the plain entry still answers the same way
    assert L.pp_cocoeval_oks(0, 17, 0, 0, 0, np.zeros((3, 1), dtype=np.int64).ctypes.data, *[P] * 8, None) == 0
