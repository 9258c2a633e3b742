"""The gauge of PoseTracker: greedy OKS track association and One-Euro smoothing restated in plain loops over numpy
float64.  Written from the rules, not from the kernels (probpose_pytorch_amd/csrc/pp_track.hip).

  Stream(K, max_tracks)                                    the state of one stream: slots and two counters
  Tracker(sigmas, match_thr, max_age, max_tracks, vis_thr, smooth, fps)
      .update(frames, t=None) -> {stream: dict(ids, keypoints, oks, born, ...)}     one call: one frame per named stream
  alpha(te, fc), one_euro_step(x, xhat, dxhat, te, smooth)  the filter's arithmetic, one coordinate

A ``frame`` is a dict of arrays: kpts [D, K, 2], score [D], area [D] and vis [D, K] (or None).  ``smooth`` is None or
(min_cutoff, beta, d_cutoff).  The rules, per named stream:

  1. detections are visited by descending score, equal scores in the order they were given;
  2. the OKS of a detection and a live slot (id >= 0 when the call begins) is posenms_reference.pair_oks with the slot's
     stored raw keypoints, area and visibilities as the second detection;
  3. each detection in visiting order takes the live slot not yet taken in this call with the largest OKS (the lowest
     slot on equal OKS), if that OKS is > match_thr;
  4. then every live slot not taken ages by one and is freed when age > max_age;
  5. a matched detection gets the slot's id; every keypoint goes through the One-Euro step with te = t - t_last
     (uncounted: raw output, init = 0; init == 0: initialise; else filter); age = 0 and the raw state is replaced;
  6. then each unmatched detection in visiting order takes the lowest free slot (those freed in 4 included) with
     id = next_id++, or, with none free, gets id -1 and counts in ``overflow``.

The switches (``given_order``, ``ge_match``, ``births_first``, ``track_area``, ``te_from_age``,
``keep_uncounted``) exist so that tests/test_track_reference.py can show that the gauge tells each rule from its
mutation; their defaults are the rules.
"""
import numpy as np

from tests import posenms_reference as PR

TWO_PI = np.float64(2.0) * np.float64(np.pi)


def alpha(te, fc):
    r = (TWO_PI * np.float64(fc)) * np.float64(te)
    return r / (r + np.float64(1.0))


def one_euro_step(x, xhat, dxhat, te, smooth):
    """One coordinate: (new xhat, new dxhat); the products and sums unfused, in the order of the rules."""
    min_cutoff, beta, d_cutoff = (np.float64(v) for v in smooth)
    x, xhat, dxhat, te = np.float64(x), np.float64(xhat), np.float64(dxhat), np.float64(te)
    dx = (x - xhat) / te
    a_d = alpha(te, d_cutoff)
    dxhat = a_d * dx + (np.float64(1.0) - a_d) * dxhat
    a = alpha(te, min_cutoff + beta * np.abs(dxhat))
    xhat = a * x + (np.float64(1.0) - a) * xhat
    return xhat, dxhat


class Stream:
    def __init__(self, K, max_tracks):
        T = max_tracks
        self.id = np.full(T, -1, dtype=np.int64)
        self.age = np.zeros(T, dtype=np.int32)
        self.t_last = np.zeros(T)
        self.area = np.zeros(T)
        self.kp = np.zeros((T, K, 2))
        self.vis = np.ones((T, K))
        self.xhat = np.zeros((T, K, 2))
        self.dxhat = np.zeros((T, K, 2))
        self.init = np.zeros((T, K), dtype=np.uint8)
        self.next_id = 0
        self.overflow = 0


def make_frame(kpts, score, area, vis=None):
    return PR.make_image(kpts, score, area, vis)


class Tracker:
    def __init__(self, sigmas, match_thr=0.3, max_age=30, max_tracks=64, vis_thr=None, smooth=None, fps=30.0,
                 given_order=False, ge_match=False, births_first=False, track_area=False, te_from_age=False,
                 keep_uncounted=False):
        self.sigmas = np.asarray(sigmas, dtype=np.float64)
        self.K = self.sigmas.size
        self.match_thr, self.max_age, self.max_tracks = np.float64(match_thr), int(max_age), int(max_tracks)
        self.vis_thr = None if vis_thr is None else np.float64(vis_thr)
        self.smooth, self.fps = smooth, float(fps)
        self.switches = dict(given_order=given_order, ge_match=ge_match, births_first=births_first,
                             track_area=track_area, te_from_age=te_from_age, keep_uncounted=keep_uncounted)
        self.streams = {}
        self.calls = 0
        self.t_prev = None

    def reset(self, stream=None):
        if stream is None:
            self.streams.clear()
        else:
            self.streams.pop(stream, None)

    def counted(self, vis_row, k):
        return self.vis_thr is None or vis_row[k] > self.vis_thr

    def update(self, frames, t=None):
        """``frames``: {stream: frame}.  Returns {stream: dict(ids [D] int64, keypoints [D, K, 2], oks [D], born [D]
        bool in the order given; oks_seen (every evaluated pair OKS), gaps (per detection with a candidate: best OKS,
        second best or None, their slots), events (counts of match, birth, expiry, reid, overflow, reinit))}."""
        self.calls += 1
        t = np.float64(self.calls / self.fps if t is None else t)
        if self.t_prev is not None and not t > self.t_prev:
            raise ValueError("t: must increase strictly")
        self.t_prev = t
        return {s: self._update_stream(self.streams.setdefault(s, Stream(self.K, self.max_tracks)), f, t)
                for s, f in frames.items()}

    def _update_stream(self, st, frame, t):
        sw = self.switches
        kpts, area, vis = frame["kpts"], frame["area"], frame["vis"]
        if self.vis_thr is not None and vis is None:
            raise ValueError("vis_thr needs visibilities")
        D, T, K = kpts.shape[0], self.max_tracks, self.K
        order = list(range(D)) if sw["given_order"] else PR.visiting_order(frame["score"])
        ids = np.full(D, -1, dtype=np.int64)
        out = np.array(kpts, dtype=np.float64)
        oks_out = np.zeros(D)
        born = np.zeros(D, dtype=bool)
        live = st.id >= 0                                   # at entry
        taken = np.zeros(T, dtype=bool)
        match = {}
        oks_seen, gaps = [], []
        events = dict(match=0, birth=0, expiry=0, reid=0, overflow=0, reinit=0)

        for d in order:                                     # 2, 3
            best, best_j, second, second_j = None, None, None, None
            for j in range(T):
                if not live[j] or taken[j]:
                    continue
                a_det = st.area[j] if sw["track_area"] else area[d]     # (x + x) / 2 is x: the track's area alone
                v = PR.pair_oks(kpts[d], st.kp[j], a_det, st.area[j], self.sigmas, None if vis is None else vis[d],
                                st.vis[j], self.vis_thr)
                oks_seen.append(v)
                if best is None or v > best:
                    best, best_j, second, second_j = v, j, best, best_j
                elif second is None or v > second:
                    second, second_j = v, j
            if best is None:
                continue
            gaps.append((best, second, best_j, second_j))
            if best >= self.match_thr if sw["ge_match"] else best > self.match_thr:
                taken[best_j] = True
                match[d] = (best_j, best)

        def expire():                                       # 4
            for j in range(T):
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

        def births():                                       # 6
            for d in order:
                if d in match:
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

        if sw["births_first"]:
            births()
            expire()
        else:
            expire()

        for d, (j, v) in match.items():                     # 5
            ids[d], oks_out[d] = st.id[j], v
            events["match"] += 1
            events["reid"] += int(st.age[j] > 0)
            te = np.float64(int(st.age[j]) + 1) / np.float64(self.fps) if sw["te_from_age"] else t - st.t_last[j]
            if self.smooth is not None:
                for k in range(K):
                    if not self.counted(None if vis is None else vis[d], k):
                        if not sw["keep_uncounted"]:
                            st.init[j, k] = 0
                    elif st.init[j, k] == 0:
                        st.xhat[j, k], st.dxhat[j, k], st.init[j, k] = kpts[d, k], 0.0, 1
                        events["reinit"] += 1
                    else:
                        for c in range(2):
                            st.xhat[j, k, c], st.dxhat[j, k, c] = one_euro_step(kpts[d, k, c], st.xhat[j, k, c],
                                                                                st.dxhat[j, k, c], te, self.smooth)
                        out[d, k] = st.xhat[j, k]
            store_raw(j, d)

        if not sw["births_first"]:
            births()
        return dict(ids=ids, keypoints=out, oks=oks_out, born=born, oks_seen=oks_seen, gaps=gaps, events=events,
                    order=order)


# ------------------------------------------------------------------------------------------------ fixtures
def make_scene(seed, K, n_frames, n_people, max_age, leavers=0, entrants=0, duplicates=False, with_vis=True):
    """A seeded scene of one stream: (frames, times, who).  ``frames`` is a list of frames (make_frame), ``times`` the
    uneven frame times in seconds, ``who`` per frame the person behind every detection.

    People have a side of 40, 60 or 150 (x 0.8 .. 1.25), K keypoints spread over their square, a drift of at most 1.5 %
    of the side per frame and axis and a keypoint jitter of 2 % of the side (uniform, per frame, keypoint and axis);
    areas are 0.6 side^2 within 5 %.  Every third person (2, 5, 8, ...) is absent for a gap that cycles through 1 ..
    max_age + 3 frames, from frame 2 on; the last ``leavers`` people leave for good after frame 1 and the same number
    of ``entrants`` appear from frame n_frames // 2 on (by then the leavers' slots are free again: n_frames // 2 >
    max_age + 2).  With ``duplicates`` person 2 i + 1 is person 2 i moved by 10 % of the side, drifting with it.
    Scores are distinct in (0.05, 1) except one tie between the first two detections of frame 3; visibilities are
    uniform in (0, 1); the detections of a frame are shuffled."""
    rng = np.random.default_rng(seed)
    P = n_people + entrants
    side = rng.choice([40.0, 60.0, 150.0], P) * rng.uniform(0.8, 1.25, P)
    cols = int(np.ceil(np.sqrt(P)))
    centre = np.stack([(np.arange(P) % cols) * 420.0, (np.arange(P) // cols) * 420.0], axis=1) + rng.uniform(0, 60, (P, 2))
    shape = rng.uniform(0, 1, (P, K, 2)) * side[:, None, None]
    drift = rng.uniform(-0.015, 0.015, (P, 2)) * side[:, None]
    if duplicates:
        for i in range(1, P, 2):
            side[i], shape[i], drift[i] = side[i - 1], shape[i - 1], drift[i - 1]
            ang = rng.uniform(0, 2 * np.pi)
            centre[i] = centre[i - 1] + 0.1 * side[i] * np.array([np.cos(ang), np.sin(ang)])
    present = np.ones((n_frames, P), dtype=bool)
    gaps = list(range(1, max_age + 4))
    for n, i in enumerate(range(2, n_people - leavers, 3)):
        g = gaps[n % len(gaps)]
        start = 2 + n % 2
        present[start:start + g, i] = False
    present[1:, n_people - leavers:n_people] = False
    present[:n_frames // 2, n_people:] = False
    assert leavers == entrants and (not entrants or n_frames // 2 > max_age + 2)
    times = np.cumsum(rng.uniform(0.02, 0.06, n_frames))
    frames, who = [], []
    for f in range(n_frames):
        idx = rng.permutation(np.nonzero(present[f])[0])
        kp = (centre[idx] + drift[idx] * f)[:, None, :] + shape[idx] + \
            rng.uniform(-1, 1, (idx.size, K, 2)) * 0.02 * side[idx, None, None]
        area = 0.6 * side[idx] ** 2 * rng.uniform(0.95, 1.05, idx.size)
        score = rng.permutation(np.linspace(0.05, 0.99, 4 * P + 3))[:idx.size] + 0.0
        if f == 3 and idx.size > 1:
            score[1] = score[0]
        vis = rng.uniform(0, 1, (idx.size, K)) if with_vis else None
        frames.append(make_frame(kp, score, area, vis))
        who.append(idx)
    return frames, times, who
