"""CPU tests of probpose_pytorch_amd/_ragged.py, the ragged-batch front end PoseNMS, PoseTracker and CocoKeypointEval
share: the first-seen order, the group layout and its limit messages, the shape, placement and dtype refusals, and the
visiting order against tests/posenms_reference.visiting_order, group by group.  None of this needs a GPU."""
import numpy as np
import pytest
import torch

from probpose_pytorch_amd import _lib, _ragged as R
from tests import posenms_reference as PR
from tests import ragged_fixture as F


@pytest.mark.parametrize("ids,names,pos", [
    (np.array([7, 3, 7, 9, 3]), [7, 3, 9], [0, 1, 0, 2, 1]),
    (np.array(["b", "a", "b", "c"]), ["b", "a", "c"], [0, 1, 0, 2]),
    (np.array(["cam", 4, ("x", 1), 4, "cam"], dtype=object), ["cam", 4, ("x", 1)], [0, 1, 2, 1, 0]),
    (np.zeros(0, dtype=np.int64), [], []),
    (np.zeros(0, dtype=object), [], []),
])
def test_first_seen(ids, names, pos):
    got_names, got_pos = R.first_seen(ids)
    assert got_names == names and got_pos.dtype == np.int64 and got_pos.tolist() == pos


def test_host_ids_reads_a_tensor_and_keeps_a_list():
    assert R.host_ids(torch.tensor([3, 1, 3])).tolist() == [3, 1, 3]
    assert R.host_ids(["a", "b"]).tolist() == ["a", "b"]


def test_group_layout_counts_offsets_and_limits():
    pos = np.array([2, 0, 2, 2, 0], dtype=np.int64)
    counts, off = R.group_layout(pos, ["a", "empty", "c"])              # "empty" is named and has no detection
    assert counts.dtype == off.dtype == np.int64
    assert counts.tolist() == [2, 0, 3] and off.tolist() == [0, 2, 2, 5]
    counts, off = R.group_layout(pos, 4)                                # the groups by their number alone
    assert counts.tolist() == [2, 0, 3, 0] and off.tolist() == [0, 2, 2, 5, 5]
    counts, off = R.group_layout(np.zeros(0, dtype=np.int64), [])
    assert counts.shape == (0,) and off.tolist() == [0]
    assert R.group_layout(pos, ["a", "b", "c"], "ids: group", [(3, "a call takes")])[0].tolist() == [2, 0, 3]
    with pytest.raises(ValueError, match="^ids: group 'c' has 3 detections, more than the 2 a call takes$"):
        R.group_layout(pos, ["a", "b", "c"], "ids: group", [(2, "a call takes")])
    # the limits in turn, each with its own words; the fullest group is the one named
    with pytest.raises(ValueError, match='^ids: group 12 has 3 detections, more than the 2 that "optimal" takes$'):
        R.group_layout(pos, [7, 8, 12], "ids: group", limits=[(5, "in all"), (2, 'that "optimal" takes')])


def _batch(M=4, K=3, cols=2):
    return [("keypoints", np.zeros((M, K, cols))), ("scores", np.ones(M)), ("areas", np.ones(M))]


def test_check_pose_batch_shapes():
    named, M = R.check_pose_batch(_batch(), 3)
    assert M == 4 and [n for n, _ in named] == ["keypoints", "scores", "areas"]
    named, M = R.check_pose_batch([("keypoints", [[[0.0, 1.0]]]), ("a", [1.0]), ("b", torch.ones(1))], 1, 1)
    assert M == 1 and isinstance(named[0][1], np.ndarray) and isinstance(named[2][1], torch.Tensor)
    R.check_pose_batch(_batch(cols=3), 3, 4, vis_thr=0.2)               # a third keypoint column holds visibilities
    R.check_pose_batch(_batch() + [("kpt_scores", np.ones((4, 3)))], 3, 4, vis_thr=0.2)
    tail = r" \(K = len\(sigmas\)\), got "
    with pytest.raises(ValueError, match=r"^keypoints: expected \[M, 3, 2\|3\]" + tail + r"\(4, 2, 2\)$"):
        R.check_pose_batch(_batch(K=2), 3)
    with pytest.raises(ValueError, match=r"^keypoints: expected \[5, 3, 2\|3\]" + tail + r"\(4, 3, 2\)$"):
        R.check_pose_batch(_batch(), 3, 5)
    with pytest.raises(ValueError, match=r"^keypoints: expected \[4, 3, 2\|3\]"):
        R.check_pose_batch(_batch(cols=4), 3, 4)
    with pytest.raises(ValueError, match=r"^keypoints: expected"):
        R.check_pose_batch([("keypoints", np.zeros((4, 3)))] + _batch()[1:], 3)
    bad = _batch()
    bad[2] = ("areas", np.ones(3))
    with pytest.raises(ValueError, match=r"^areas: expected \[4\], got \(3,\)$"):
        R.check_pose_batch(bad, 3)
    with pytest.raises(ValueError, match=r"^kpt_scores: expected \[4, 3\], got \(4, 2\)$"):
        R.check_pose_batch(_batch() + [("kpt_scores", np.ones((4, 2)))], 3)
    with pytest.raises(ValueError, match="^vis_thr: needs visibilities, kpt_scores or a third keypoint column$"):
        R.check_pose_batch(_batch(), 3, 4, vis_thr=0.2)


def test_placement_and_dtype_refusals():
    named, _ = R.check_pose_batch(_batch(), 3)
    assert R.on_device(named) is False
    ints = [named[0], ("scores", np.ones(4, dtype=np.int64)), named[2]]
    with pytest.raises(ValueError, match="^scores: expected a float dtype, got int64$"):
        R.device_f64(ints)
    with pytest.raises(ValueError, match="^areas: expected a float dtype, got torch.int32$"):
        R.device_f64([named[0], named[1], ("areas", torch.ones(4, dtype=torch.int32))])
    # well-formed host arrays: the device is really needed now, under the caller's names if it gives any
    with pytest.raises(_lib.HipExtensionError) as e:
        R.device_f64(named + [("kpt_scores", np.ones((4, 3)))], "keypoints / areas / scores")
    if torch.cuda.is_available():
        assert "keypoints / areas / scores: expected tensors on the GPU" in str(e.value)
        mixed = [named[0], ("scores", torch.ones(4, device="cuda")), named[2]]
        with pytest.raises(ValueError, match="^keypoints / scores / areas: either all device tensors or all host arr"):
            R.on_device(mixed)


def test_checked_f64_names_the_input_and_the_rule():
    """On CPU tensors (the function only asks for tensors): float64, contiguous, one stacked read-back."""
    ok = [("a", torch.ones(3, dtype=torch.float32)), ("b", torch.arange(6.0).reshape(2, 3).t())]
    a, b = R.checked_f64(ok)
    assert a.dtype == b.dtype == torch.float64 and b.is_contiguous() and b.tolist() == [[0, 3], [1, 4], [2, 5]]
    with pytest.raises(ValueError, match="^b: non-finite values$"):
        R.checked_f64([ok[0], ("b", torch.tensor([1.0, float("inf")]))])
    unit = (lambda p: ((p >= 0) & (p <= 1)).all(), "values outside [0, 1]")
    R.checked_f64([("p", torch.tensor([0.0, 1.0]))], {"p": unit})
    with pytest.raises(ValueError, match=r"^p: values outside \[0, 1\]$"):
        R.checked_f64([ok[0], ("p", torch.tensor([0.5, float("nan")]))], {"p": unit})


def _gauge_order(order):
    """The visiting order of the fixture's batch given in ``order``: tests/posenms_reference.visiting_order applied to
    every group, the groups by their number (positions in the batch as given)."""
    pos, score = F.POS[order], F.SCORE[order]
    want = []
    for g in sorted(set(pos.tolist())):
        idx = np.nonzero(pos == g)[0]
        want += [int(idx[i]) for i in PR.visiting_order(score[idx])]
    return want


@pytest.mark.parametrize("order", [np.arange(F.M), F.SHUFFLE], ids=["given", "shuffled"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_visiting_order_is_the_gauges(order, dtype):
    pos, score = F.POS[order], F.SCORE[order]
    sizes = np.bincount(pos).tolist()
    assert pos.size == 11 and sizes == [5, 5, 1] and (np.diff(F.POS) != 0).all()           # interleaved as given
    ties = [(a, b) for a in range(11) for b in range(a + 1, 11) if score[a] == score[b]]
    assert any(pos[a] == pos[b] for a, b in ties) and any(pos[a] != pos[b] for a, b in ties)
    perm, pos_t = R.visiting_order(torch.from_numpy(score).to(dtype), torch.from_numpy(pos))
    assert perm.dtype == torch.int64 and perm.tolist() == _gauge_order(order) and pos_t.tolist() == pos.tolist()
    uploads = []                                        # host positions go through the caller's upload, once
    again, pos_t = R.visiting_order(torch.from_numpy(score).to(dtype), pos,
                                    lambda a: uploads.append(a) or torch.from_numpy(a))
    assert again.tolist() == perm.tolist() and len(uploads) == 1 and pos_t.tolist() == pos.tolist()


def test_the_shuffle_turns_both_ties_round():
    given, shuffled = _gauge_order(np.arange(F.M)), [int(F.SHUFFLE[i]) for i in _gauge_order(F.SHUFFLE)]
    assert given.index(2) < given.index(7) and shuffled.index(7) < shuffled.index(2)
    assert given.index(6) < given.index(8) and shuffled.index(8) < shuffled.index(6)


def test_unsorted_is_the_way_back():
    perm = torch.tensor([2, 0, 3, 1])
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]])
    back = R.unsorted(perm, x[perm])
    assert back.dtype == x.dtype and torch.equal(back, x)
    assert R.unsorted(perm, torch.tensor([True, False, False, True])).tolist() == [False, True, True, False]
