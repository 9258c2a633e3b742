"""The gauge of the track-driven boxes (tests/trackbox_reference.py) against boxes computed by hand, a case per status
code, and the closed-loop scene: three people followed for 30 frames from the boxes of frame 0 alone.  CPU only."""
import functools

import numpy as np
import pytest

from tests import track_reference as TR
from tests import trackbox_reference as BR

SMOOTH = (1.0, 0.05, 1.0)
POINTS = np.array([[10.0, 20.0], [30.0, 60.0], [20.0, 40.0]])      # extent 20 x 40 about (20, 40)


def slot(points=POINTS, vis=(1.0, 1.0, 1.0), age=0, ident=0, t_last=1.0):
    st = TR.Stream(len(points), 1)
    st.id[0], st.age[0], st.t_last[0] = ident, age, t_last
    st.kp[0], st.vis[0] = points, vis
    return st


def one(st, t=1.1, **kw):
    boxes, ids, scores, status = BR.propose(st, t, **kw)
    return boxes[0].tolist(), int(ids[0]), float(scores[0]), int(status[0])


def test_three_points_by_hand():
    # w = 20 * 1.25 = 25, h = 40 * 1.25 = 50 about (20, 40)
    assert one(slot()) == ([7.5, 15.0, 25.0, 50.0], 0, 1.0, BR.PROPOSED)
    # aspect 0.75: w = 25 < 50 * 0.75 = 37.5, the width grows
    assert one(slot(), aspect=0.75) == ([1.25, 15.0, 37.5, 50.0], 0, 1.0, BR.PROPOSED)
    # aspect 0.25: w = 25 >= 50 * 0.25, the height grows to 25 / 0.25 = 100
    assert one(slot(), aspect=0.25) == ([7.5, -10.0, 25.0, 100.0], 0, 1.0, BR.PROPOSED)
    # pad 1: the extent itself; min_side lifts a degenerate extent
    assert one(slot(), pad=1.0)[0] == [10.0, 20.0, 20.0, 40.0]
    assert one(slot(np.array([[5.0, 5.0]] * 3)))[0] == [4.0, 4.0, 2.0, 2.0]
    assert one(slot(np.array([[5.0, 5.0]] * 3)), min_side=8.0)[0] == [1.0, 1.0, 8.0, 8.0]


def test_a_clamp_at_each_frame_edge():
    left, top = POINTS - [10.0, 0.0], POINTS - [0.0, 20.0]
    assert one(slot(left), frame_wh=(100.0, 100.0))[0] == [0.0, 15.0, 22.5, 50.0]        # bx -2.5 -> 0
    assert one(slot(top), frame_wh=(100.0, 100.0))[0] == [7.5, 0.0, 25.0, 45.0]          # by -5 -> 0
    assert one(slot(), frame_wh=(30.0, 100.0))[0] == [7.5, 15.0, 22.5, 50.0]             # ex 32.5 -> 30
    assert one(slot(), frame_wh=(100.0, 60.0))[0] == [7.5, 15.0, 25.0, 45.0]             # ey 65 -> 60
    assert one(slot(left), frame_wh=(0.0, 0.0))[0] == [-2.5, 15.0, 25.0, 50.0]           # (0, 0): no clamp
    assert one(slot(left))[0] == [-2.5, 15.0, 25.0, 50.0]


def test_the_filter_state_and_the_time_step():
    st = slot()
    st.xhat[0], st.dxhat[0], st.init[0] = POINTS + 100.0, [30.0, -10.0], 1
    assert one(st, smooth=False)[0] == [7.5, 15.0, 25.0, 50.0]                            # no filter: raw
    assert one(st, smooth=True, extrapolate=False)[0] == [107.5, 115.0, 25.0, 50.0]
    dt = np.float64(1.1) - np.float64(1.0)
    want = [float(np.float64(120.0) + np.float64(30.0) * dt - 12.5), float(np.float64(140.0) - np.float64(10.0) * dt - 25.0)]
    got = one(st, smooth=True)[0]
    assert got[2:] == [25.0, 50.0] and np.allclose(got[:2], want, rtol=0, atol=1e-12)
    assert one(st, t=1.5, smooth=True, max_dt=0.25)[0] == [115.0, 112.5, 25.0, 50.0]       # dt 0.5 -> 0.25
    assert one(st, t=1.5, smooth=True, max_dt=0.0)[0] == [107.5, 115.0, 25.0, 50.0]
    st.init[0, 1] = 0                   # keypoint 1 has no filter: raw (30, 60) beside (110, 120) and (120, 140)
    assert one(st, smooth=True, extrapolate=False)[0] == [75.0 - 56.25, 100.0 - 50.0, 112.5, 100.0]


def test_a_case_per_status_code():
    assert one(slot(ident=-1)) == ([0.0] * 4, -1, 0.0, BR.FREE)
    assert one(slot(age=1, ident=7)) == ([0.0] * 4, 7, 0.0, BR.OLD)
    assert one(slot(age=1, ident=7), max_age=1)[3] == BR.PROPOSED
    vis = (0.9, 0.9, 0.1)
    assert one(slot(vis=vis), vis_thr=0.3) == ([0.0] * 4, 0, 0.0, BR.FEW)
    # exactly min_keypoints counted keypoints: (10, 20) and (30, 60), score (0.9 + 0.9) / 2
    assert one(slot(vis=vis), vis_thr=0.3, min_keypoints=2) == ([7.5, 15.0, 25.0, 50.0], 0, 0.9, BR.PROPOSED)
    assert one(slot(vis=vis), vis_thr=0.1)[3] == BR.FEW                                   # > vis_thr, not >=
    assert one(slot(vis=vis))[2:] == ((0.9 + 0.9 + 0.1) / 3.0, BR.PROPOSED)               # vis_thr None: all count
    assert one(slot(), frame_wh=(5.0, 100.0)) == ([0.0] * 4, 0, 0.0, BR.OUTSIDE)          # ex 5 < bx 7.5
    assert one(slot(), frame_wh=(9.0, 100.0))[3] == BR.OUTSIDE                            # w = 1.5 < min_side
    assert one(slot(), frame_wh=(9.5, 100.0)) == ([7.5, 15.0, 2.0, 50.0], 0, 1.0, BR.PROPOSED)
    # a given box of the same size moved by 5: inter 20 * 50, union 2500 - 1000
    given, iou = [[12.5, 15.0, 25.0, 50.0]], np.float64(1000.0) / np.float64(1500.0)
    assert one(slot(), sup_boxes=given, iou_thr=np.nextafter(iou, 0)) == ([7.5, 15.0, 25.0, 50.0], 0, 1.0, BR.SUPPRESSED)
    assert one(slot(), sup_boxes=given, iou_thr=iou)[3] == BR.PROPOSED                   # > iou_thr, not >=
    assert one(slot(), sup_boxes=[[7.5, 15.0, 0.0, 50.0], [7.5, 15.0, 25.0, 0.0]], iou_thr=0.0)[3] == BR.PROPOSED
    assert one(slot(), sup_boxes=[[7.5, 15.0, 0.0, 50.0]] + given, iou_thr=0.5)[3] == BR.SUPPRESSED
    assert one(slot(), sup_boxes=[[200.0, 15.0, 25.0, 50.0]], iou_thr=0.0)[3] == BR.PROPOSED       # disjoint
    # a stream without given boxes beside one that has some
    status = [one(slot(), sup_boxes=g, iou_thr=0.5)[3] for g in ((), given)]
    assert status == [BR.PROPOSED, BR.SUPPRESSED]


def test_compact_takes_the_proposed_rows_slots_ascending():
    st = TR.Stream(3, 4)
    st.id[:] = [5, -1, 6, 7]
    st.age[2] = 3
    st.kp[:] = POINTS
    boxes, ids, scores = BR.compact(*BR.propose(st, 1.0))
    assert ids.tolist() == [5, 7] and boxes.tolist() == [[7.5, 15.0, 25.0, 50.0]] * 2 and scores.tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------ the closed loop
@functools.lru_cache(maxsize=None)
def loop(v, smooth, gone=None, other_stream=False, **options):
    """The scene through the gauge follower: (steps, tracker).  ``other_stream``: a second, empty stream is updated
    halfway between the frames, so the tracker's previous call time is not the tracks' t_last."""
    scene = BR.Scene(v, gone)
    tracker = scene.tracker(SMOOTH if smooth else None)
    follower = BR.Follower(tracker, scene.estimate, **options)
    if not other_stream:
        return scene.run(follower), tracker
    empty = TR.make_frame(np.zeros((0, scene.K, 2)), [], [], np.zeros((0, scene.K)))
    steps = []
    for f in range(scene.FRAMES):
        steps.append(follower.step(f, scene.first_boxes if f == 0 else None, frame_size=scene.SIZE,
                                   t=(f + 1) / scene.FPS))
        tracker.update({"other": empty}, (f + 1.5) / scene.FPS)
    return steps, tracker


def ids_of(steps):
    return [sorted(s["result"]["ids"].tolist()) for s in steps]


def visible(steps):
    return [int((s["kpt_scores"] > 0.3).sum()) for s in steps]


def followed(steps):
    return len(steps) == 30 and all(i == [0, 1, 2] for i in ids_of(steps)) and visible(steps) == [51] * 30


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("extrapolate", [False, True])
def test_slow_people_are_followed_in_every_mode(smooth, extrapolate):
    steps, _ = loop(2, smooth, extrapolate=extrapolate)
    assert followed(steps)
    assert [s["proposed"].shape[0] for s in steps] == [0] + [3] * 29
    assert all(s["source"].tolist() == ([0, 0, 0] if f == 0 else [1, 1, 1]) for f, s in enumerate(steps))


def test_fast_people_need_the_extrapolation():
    assert followed(loop(3, True, extrapolate=True)[0])
    lost, _ = loop(3, True, extrapolate=False)
    assert min(visible(lost)) == 17 and any(i != [0, 1, 2] for i in ids_of(lost))
    assert followed(loop(3, True, extrapolate=True, aspect=0.75)[0])


def test_a_person_who_leaves_gives_birth_to_nothing():
    steps, tracker = loop(3, True, gone=(2, 15))
    assert [s["proposed"].shape[0] for s in steps] == [0] + [3] * 15 + [2] * 14       # frame 15 still proposes three
    assert all(i == [0, 1, 2] for i in ids_of(steps)[:15]) and all(i == [0, 1] for i in ids_of(steps)[15:])
    st = tracker.streams[0]
    assert st.id.tolist() == [0, 1] + [-1] * 6 and st.next_id == 3


@pytest.mark.parametrize("fault, options", [("dt_from_call", dict(other_stream=True)), ("raw_always", {}),
                                            ("pad_after_aspect", dict(aspect=0.75))])
def test_each_planted_fault_changes_a_box(fault, options):
    boxes = lambda steps: b"".join(s["proposed"].tobytes() for s in steps)
    right, _ = loop(3, True, **options)
    wrong, _ = loop(3, True, **options, **{fault: True})
    assert followed(right) and boxes(right) != boxes(wrong)
