"""The gauge of PoseTracker's motion prediction and two-stage association, in plain loops over numpy
float64 and Python ints.  Written from the rules (include/probpose_hip.h), not from the kernels; built on
tests/track_reference.py (state, One-Euro step, scenes) and tests/trackopt_reference.py (weights and solver).

  predicted_pose(st, j, t, max_dt)        where slot j's filter expects its keypoints at time t
  Tracker(sigmas, ..., assign, predict, predict_max_dt, high_thr, low_match_thr, low_max_age, birth_thr)
      .update(frames, t=None) -> {stream: dict(ids, keypoints, oks, born, dropped, ...)}

The rules, per named stream, on top of rules 1 - 6 of tests/track_reference.py:

  P. with ``predict``, the second pose of rule 2's pair OKS is, for a live slot j and keypoint k and coordinate c,
       dt = t - t_last[j]; if dt > max_dt: dt = max_dt
       p = xhat[j, k, c] + dxhat[j, k, c] * dt   (one product, then one sum)   if init[j, k] else kp[j, k, c]
     in place of the stored raw keypoints; the slot's stored visibilities and area are used as they are.
  S. rule 3 runs in two stages.  With "live" and "age" as they are when the call begins:
       stage 1: rows are the detections with score >= high_thr (in visiting order: a prefix), columns the live slots,
                the threshold is match_thr;
       stage 2: rows are the other detections, columns the live slots stage 1 did not take whose age <= low_max_age,
                the threshold is low_match_thr.
     Within a stage, assign "greedy": each row in turn takes the column not yet taken with the largest OKS (the lowest
     slot on equal OKS) if that OKS is > the threshold.  "optimal": trackopt_reference.solve on the stage's rows with
     quantise(oks, columns, threshold), so m = max(rows, T).  high_thr None is -inf: everything is stage 1.
  B. rule 6 bears an unmatched detection only if its score >= birth_thr (None: high_thr); every other unmatched
     detection is dropped: id -1, OKS 0, not born, ``dropped``, and ``overflow`` does not count it.

With every option off this is track_reference.Tracker (greedy) or trackopt_reference.Tracker (optimal).
"""
import numpy as np

from tests import posenms_reference as PR
from tests import track_reference as TR
from tests import trackopt_reference as OR

NEG_INF = np.float64(-np.inf)


def predicted_pose(st, j, t, max_dt):
    """[K, 2]: rule P for slot j of the stream state ``st``."""
    dt = np.float64(t) - st.t_last[j]
    if dt > max_dt:
        dt = np.float64(max_dt)
    pose = np.array(st.kp[j], dtype=np.float64)
    for k in range(pose.shape[0]):
        if st.init[j, k]:
            for c in range(2):
                pose[k, c] = st.xhat[j, k, c] + st.dxhat[j, k, c] * dt
    return pose


class Tracker(TR.Tracker):
    def __init__(self, sigmas, match_thr=0.3, max_age=30, max_tracks=64, vis_thr=None, smooth=None, fps=30.0,
                 assign="greedy", predict=False, predict_max_dt=None, high_thr=None, low_match_thr=None, low_max_age=0,
                 birth_thr=None):
        super().__init__(sigmas, match_thr, max_age, max_tracks, vis_thr, smooth, fps)
        assert assign in ("greedy", "optimal") and not (predict and smooth is None)
        self.assign, self.predict = assign, bool(predict)
        self.max_dt = np.float64(np.inf if predict_max_dt is None else predict_max_dt)
        self.high_thr = NEG_INF if high_thr is None else np.float64(high_thr)
        self.birth_thr = self.high_thr if birth_thr is None else np.float64(birth_thr)
        self.low_match_thr = self.match_thr if low_match_thr is None else np.float64(low_match_thr)
        self.low_max_age = int(low_max_age)

    def _update_stream(self, st, frame, t):
        kpts, area, vis, score = frame["kpts"], frame["area"], frame["vis"], frame["score"]
        if self.vis_thr is not None and vis is None:
            raise ValueError("vis_thr needs visibilities")
        D, T, K = kpts.shape[0], self.max_tracks, self.K
        order = PR.visiting_order(score)
        ids = np.full(D, -1, dtype=np.int64)
        out = np.array(kpts, dtype=np.float64)
        oks_out = np.zeros(D)
        born, dropped = np.zeros(D, dtype=bool), np.zeros(D, dtype=bool)
        live = st.id >= 0                                   # at entry
        age_in = st.age.copy()
        events = dict(match=0, birth=0, expiry=0, reid=0, overflow=0, reinit=0, low_match=0, dropped=0, refused=0,
                      kept_out=0)

        oks = np.zeros((D, T))                              # rows in visiting order; rules 2 and P
        for j in np.nonzero(live)[0]:
            pose = predicted_pose(st, j, t, self.max_dt) if self.predict else st.kp[j]
            for p, d in enumerate(order):
                oks[p, j] = PR.pair_oks(kpts[d], pose, area[d], st.area[j], self.sigmas,
                                        None if vis is None else vis[d], st.vis[j], self.vis_thr)

        n_high = sum(1 for d in order if score[d] >= self.high_thr)
        assert all(score[d] >= self.high_thr for d in order[:n_high])
        taken = np.zeros(T, dtype=bool)
        match, gaps, stages = {}, [], []
        for stage, rows in enumerate((range(0, n_high), range(n_high, D))):     # rule S
            if len(rows) == 0:
                continue
            if stage == 0:
                cols, thr = live.copy(), self.match_thr
            else:
                cols, thr = live & ~taken & (age_in <= self.low_max_age), self.low_match_thr
                barred = live & ~taken & (age_in > self.low_max_age)
                events["kept_out"] += int(sum(1 for j in np.nonzero(barred)[0] if (oks[list(rows), j] > thr).any()))
            found = {}
            if self.assign == "optimal":
                q = OR.quantise(oks[list(rows)], cols, thr)
                slots, _ = OR.solve(q)
                found = {rows[i]: j for i, j in enumerate(slots) if j >= 0}
                stages.append(dict(q=q, rows=len(rows), n_cols=int(cols.sum())))
            else:
                for p in rows:
                    best, best_j, second = None, None, None
                    for j in range(T):
                        if not cols[j] or j in found.values():
                            continue
                        v = oks[p, j]
                        if best is None or v > best:
                            best, best_j, second = v, j, best
                        elif second is None or v > second:
                            second = v
                    if best is None:
                        continue
                    gaps.append((best, second, thr))
                    if best > thr:
                        found[p] = best_j
            for p, j in found.items():
                taken[j] = True
                match[order[p]] = (j, oks[p, j])
            if stage == 1:
                events["low_match"] += len(found)

        for j in range(T):                                  # rule 4
            if live[j] and not taken[j]:
                st.age[j] += 1
                if st.age[j] > self.max_age:
                    st.id[j] = -1
                    events["expiry"] += 1

        def store_raw(j, d):
            st.age[j] = 0
            st.t_last[j] = t
            st.area[j] = area[d]
            st.kp[j] = kpts[d]
            st.vis[j] = 1.0 if vis is None else vis[d]

        for d, (j, v) in match.items():                     # rule 5
            ids[d], oks_out[d] = st.id[j], v
            events["match"] += 1
            events["reid"] += int(st.age[j] > 0)
            te = t - st.t_last[j]
            if self.smooth is not None:
                for k in range(K):
                    if not self.counted(None if vis is None else vis[d], k):
                        st.init[j, k] = 0
                    elif st.init[j, k] == 0:
                        st.xhat[j, k], st.dxhat[j, k], st.init[j, k] = kpts[d, k], 0.0, 1
                        events["reinit"] += 1
                    else:
                        for c in range(2):
                            st.xhat[j, k, c], st.dxhat[j, k, c] = TR.one_euro_step(kpts[d, k, c], st.xhat[j, k, c],
                                                                                   st.dxhat[j, k, c], te, self.smooth)
                        out[d, k] = st.xhat[j, k]
            store_raw(j, d)

        for d in order:                                     # rules 6 and B
            if d in match:
                continue
            if not score[d] >= self.birth_thr:
                dropped[d] = True
                events["dropped"] += 1
                events["refused"] += int(score[d] >= self.high_thr)      # a row of stage 1, yet below birth_thr
                continue
            free = [j for j in range(T) if st.id[j] < 0]
            if not free:
                st.overflow += 1
                events["overflow"] += 1
                continue
            j = free[0]
            st.id[j] = st.next_id
            st.next_id += 1
            ids[d], born[d] = st.id[j], True
            events["birth"] += 1
            store_raw(j, d)
            if self.smooth is not None:
                for k in range(K):
                    if self.counted(None if vis is None else vis[d], k):
                        st.init[j, k], st.xhat[j, k], st.dxhat[j, k] = 1, kpts[d, k], 0.0
                    else:
                        st.init[j, k] = 0
        return dict(ids=ids, keypoints=out, oks=oks_out, born=born, dropped=dropped, events=events, order=order,
                    gaps=gaps, stages=stages, n_high=n_high, n_live=int(live.sum()),
                    oks_seen=[float(x) for x in oks[:, live].reshape(-1)])
