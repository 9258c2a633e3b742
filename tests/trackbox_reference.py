"""The gauge of PoseTracker.propose_boxes and PoseFollower: the rule of pp_track_boxes (include/probpose_hip.h, DESIGN
§4.7e) restated in plain loops over numpy float64 on a ``track_reference.Stream``, and the follow loop on a
``track_reference.Tracker``.  Written from the rule, not from the kernel.

  propose(st, t, ...) -> (boxes [T, 4], ids [T], scores [T], status [T] uint8)      one stream's slots
  compact(boxes, ids, scores, status) -> the PROPOSED rows, slots ascending
  Follower(tracker, estimate, **options).step(frame, boxes, ...) -> dict            the loop of follow.PoseFollower
  Scene(v, gone=None)                                                               the closed-loop fixture

Every step of the rule is one float64 operation in the stated order; min and max are single comparisons.  The switches
``dt_from_call``, ``raw_always`` and ``pad_after_aspect`` plant one fault each, so that tests/test_trackbox_reference.py
can show that the gauge tells the rule from it; their defaults are the rule.
"""
import numpy as np

from tests import track_reference as TR

FREE, PROPOSED, OLD, FEW, OUTSIDE, SUPPRESSED = range(6)
F = np.float64
HALF, ZERO = F(0.5), F(0.0)


def propose(st, t, *, vis_thr=None, smooth=False, extrapolate=True, max_dt=np.inf, max_age=0, min_keypoints=3,
            pad=1.25, min_side=2.0, aspect=0.0, frame_wh=None, sup_boxes=(), iou_thr=0.3, t_prev=None,
            dt_from_call=False, raw_always=False, pad_after_aspect=False):
    """``st``: a track_reference.Stream.  ``vis_thr`` None: every keypoint counts.  ``smooth``: whether the tracker
    filters (its ``smooth`` is not None).  ``frame_wh``: (w, h) or None; (0, 0) does not clamp.  ``sup_boxes``: the
    given boxes of this stream, xywh.  ``t_prev``: the tracker's previous call time, read only by ``dt_from_call``."""
    T, K = st.vis.shape
    t, max_dt, pad, min_side, aspect, iou_thr = F(t), F(max_dt), F(pad), F(min_side), F(aspect), F(iou_thr)
    boxes, ids = np.zeros((T, 4)), np.full(T, -1, dtype=np.int64)
    scores, status = np.zeros(T), np.zeros(T, dtype=np.uint8)
    for j in range(T):
        if st.id[j] < 0:                                                # 1
            status[j] = FREE
            continue
        ids[j] = st.id[j]
        if st.age[j] > max_age:                                         # 2
            status[j] = OLD
            continue
        dt = t - (F(t_prev) if dt_from_call else st.t_last[j])          # 3
        if dt > max_dt:
            dt = max_dt
        n, total = 0, ZERO
        x0 = x1 = y0 = y1 = ZERO
        for k in range(K):                                              # 4
            if vis_thr is not None and not st.vis[j, k] > F(vis_thr):
                continue
            if smooth and st.init[j, k] and not raw_always:
                px, py = st.xhat[j, k, 0], st.xhat[j, k, 1]
                if extrapolate:
                    px = px + st.dxhat[j, k, 0] * dt
                    py = py + st.dxhat[j, k, 1] * dt
            else:
                px, py = st.kp[j, k, 0], st.kp[j, k, 1]
            if n == 0:
                x0 = x1 = px
                y0 = y1 = py
            else:
                if px < x0:
                    x0 = px
                if px > x1:
                    x1 = px
                if py < y0:
                    y0 = py
                if py > y1:
                    y1 = py
            total = total + st.vis[j, k]
            n += 1
        if n < min_keypoints:                                           # 5
            status[j] = FEW
            continue
        cx, cy = (x0 + x1) * HALF, (y0 + y1) * HALF                     # 6
        w, h = x1 - x0, y1 - y0
        if not pad_after_aspect:
            w, h = w * pad, h * pad
        if not w >= min_side:
            w = min_side
        if not h >= min_side:
            h = min_side
        if aspect > 0:                                                  # 7
            wa = h * aspect
            if w < wa:
                w = wa
            else:
                h = w / aspect
        if pad_after_aspect:
            w, h = w * pad, h * pad
        bx, by = cx - w * HALF, cy - h * HALF                           # 8
        ex, ey = bx + w, by + h
        if frame_wh is not None and F(frame_wh[0]) > 0:                 # 9
            fw, fh = F(frame_wh[0]), F(frame_wh[1])
            if bx < 0:
                bx = ZERO
            if by < 0:
                by = ZERO
            if ex > fw:
                ex = fw
            if ey > fh:
                ey = fh
        w, h = ex - bx, ey - by                                         # 10
        if not all(np.isfinite(v) for v in (bx, by, w, h)) or not (w >= min_side and h >= min_side):    # 11
            status[j] = OUTSIDE
            continue
        status[j] = PROPOSED
        for g in np.asarray(sup_boxes, dtype=np.float64).reshape(-1, 4):            # 12
            gx, gy, gw, gh = g
            if not (gw > 0 and gh > 0):
                continue
            gex, gey = gx + gw, gy + gh
            ix = (ex if ex < gex else gex) - (bx if bx > gx else gx)
            iy = (ey if ey < gey else gey) - (by if by > gy else gy)
            inter = ix * iy if (ix > 0 and iy > 0) else ZERO
            uni = (w * h + gw * gh) - inter
            iou = inter / uni if uni > 0 else ZERO
            if iou > iou_thr:
                status[j] = SUPPRESSED
                break
        boxes[j] = (bx, by, w, h)                                       # 13
        scores[j] = total / F(n)
    return boxes, ids, scores, status


def compact(boxes, ids, scores, status):
    rows = np.flatnonzero(status == PROPOSED)
    return boxes[rows], ids[rows], scores[rows]


class Follower:
    """follow.PoseFollower on the gauge tracker: propose, crop list (given boxes first, then proposals), estimate, drop
    the poses with fewer than ``min_keypoints`` keypoints above vis_thr, update.  ``faults``: switches of ``propose``."""

    def __init__(self, tracker, estimate, *, pad=1.25, aspect=None, min_side=2.0, min_keypoints=3, max_age=0,
                 extrapolate=True, max_dt=None, iou_thr=0.3, **faults):
        assert tracker.vis_thr is not None
        self.tracker, self.estimate = tracker, estimate
        self.options = dict(pad=pad, aspect=0.0 if aspect is None else aspect, min_side=min_side,
                            min_keypoints=min_keypoints, max_age=max_age, extrapolate=extrapolate,
                            max_dt=np.inf if max_dt is None else max_dt, iou_thr=iou_thr, **faults)

    def proposals(self, t, stream, frame_size, given):
        tr = self.tracker
        st = tr.streams.get(stream)
        if st is None:
            return np.zeros((0, 4)), np.zeros(0, dtype=np.int64), np.zeros(0)
        return compact(*propose(st, t, vis_thr=tr.vis_thr, smooth=tr.smooth is not None, frame_wh=frame_size,
                                sup_boxes=given, t_prev=tr.t_prev, **self.options))

    def step(self, frame, boxes=None, box_scores=None, *, frame_size=None, t=None, stream=0):
        tr = self.tracker
        t = (tr.calls + 1) / tr.fps if t is None else t
        given = np.zeros((0, 4)) if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        g_scores = np.ones(given.shape[0]) if box_scores is None else np.asarray(box_scores, dtype=np.float64)
        p_boxes, p_ids, p_scores = self.proposals(t, stream, frame_size, given)
        crops = np.concatenate([given, p_boxes])
        source = np.concatenate([np.zeros(given.shape[0], dtype=np.int64), np.ones(p_boxes.shape[0], dtype=np.int64)])
        scores = np.concatenate([g_scores, p_scores])
        K = tr.K
        kp, vis = (np.zeros((0, K, 2)), np.zeros((0, K))) if not crops.shape[0] else self.estimate(frame, crops)
        keep = (vis > tr.vis_thr).sum(axis=1) >= self.options["min_keypoints"]
        frame_in = TR.make_frame(kp[keep], scores[keep], (crops[:, 2] * crops[:, 3])[keep], vis[keep])
        result = tr.update({stream: frame_in}, t)[stream]
        return dict(boxes=crops[keep], source=source[keep], result=result, kpt_scores=vis[keep], proposed=p_boxes,
                    proposed_ids=p_ids)


class Scene:
    """The closed-loop fixture: K = 17 keypoints of a 40 x 100 template (keypoint k at ((7 k) % 41, (13 k) % 101), the
    first four its corners), three people starting at (20, 20), (140, 60), (250, 120) and moving by v (1, 0.5),
    v (-0.5, 0.6), v (-1, -0.7) pixels per frame in a 320 x 240 frame, 30 frames at 30 fps.  ``gone``: (person, first
    frame without them).  A ``frame`` is its number."""
    K, FRAMES, FPS, SIZE = 17, 30, 30.0, (320.0, 240.0)
    START = np.array([[20.0, 20.0], [140.0, 60.0], [250.0, 120.0]])
    DIRECTION = np.array([[1.0, 0.5], [-0.5, 0.6], [-1.0, -0.7]])

    def __init__(self, v, gone=None):
        k = np.arange(self.K)
        self.template = np.stack([(7 * k) % 41, (13 * k) % 101], axis=1).astype(np.float64)
        self.template[:4] = [(0, 0), (40, 100), (0, 100), (40, 0)]
        self.v, self.gone = float(v), gone
        self.first_boxes = np.concatenate([self.START, np.tile([40.0, 100.0], (3, 1))], axis=1)

    def people(self, f):
        """(keypoints [P, K, 2], their means [P, 2]) of the people present in frame f."""
        who = [p for p in range(3) if self.gone is None or not (p == self.gone[0] and f >= self.gone[1])]
        kp = (self.START[who] + self.DIRECTION[who] * (self.v * f))[:, None, :] + self.template[None]
        return kp, kp.mean(axis=1)

    def estimate(self, f, boxes):
        """Per box the person whose keypoint mean lies inside it and is nearest its centre in L1: their keypoints with
        score 0.9 where inside the box, the box centre with 0.05 elsewhere; no such person: all keypoints 0.05."""
        kp_all, mean = self.people(f)
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        kp, sc = np.empty((b.shape[0], self.K, 2)), np.full((b.shape[0], self.K), 0.05)
        for i, (x, y, w, h) in enumerate(b):
            ex, ey, cx, cy = x + w, y + h, x + w * 0.5, y + h * 0.5
            best, best_d = None, None
            for p in range(mean.shape[0]):
                mx, my = mean[p]
                if x <= mx <= ex and y <= my <= ey:
                    d = abs(mx - cx) + abs(my - cy)
                    if best is None or d < best_d:
                        best, best_d = p, d
            kp[i] = (cx, cy)
            if best is not None:
                c = kp_all[best]
                inside = (c[:, 0] >= x) & (c[:, 0] <= ex) & (c[:, 1] >= y) & (c[:, 1] <= ey)
                kp[i][inside] = c[inside]
                sc[i][inside] = 0.9
        return kp, sc

    def tracker(self, smooth=None, **switches):
        return TR.Tracker(np.full(self.K, 0.05), match_thr=0.3, max_age=5, max_tracks=8, vis_thr=0.3, smooth=smooth,
                          fps=self.FPS, **switches)

    def run(self, follower, between=None):
        """The 30 frames through ``follower`` (boxes given on frame 0 only): the list of its steps' results.
        ``between(f)`` runs after frame f's step."""
        out = []
        for f in range(self.FRAMES):
            out.append(follower.step(f, self.first_boxes if f == 0 else None, frame_size=self.SIZE))
            if between is not None:
                between(f)
        return out
