"""The gauge of PoseTracker(assign="optimal"): the optimal track association restated in plain loops on Python ints.
Written from the rule (include/probpose_hip.h), not from the kernel.

  quantise(oks, live, thr) -> q            the integer weights of a stream and call: [D, T] (a list of lists of ints)
  solve(q) -> (slot per detection, steps)  shortest augmenting paths with potentials; -1 = unmatched
  total(q, slots)                          the sum of q over the matched pairs
  margin(q)                                the optimum's lead over every matching that lacks one of its pairs
  Tracker(...)                             tests/track_reference.Tracker with the association replaced
  EXAMPLE, crossing_pair(sigmas)           the 2 x 2 pair OKS on which greedy switches an identity, and a scene with them

The rule.  Rows are the stream's D detections in visiting order, columns 0 .. T-1 its slots, m = max(D, T); columns
T .. m-1 are virtual ("unmatched").  q[i][j] = 0 if j >= T, if slot j is not live when the call begins or if
not (oks[i][j] > match_thr) (a NaN is inadmissible); otherwise q = 1 + floor(min(oks[i][j] - match_thr, 1.0) * 2^40) in
IEEE float64.  Costs a = -q.  Then, all in integers, INF = 2^62:

  1. u[i] = 0, v[j] = 0, no column holds a row;
  2. rows i = 0 .. D-1 in order: minv[j] = INF, used[j] = false, way[j] = root; root is an extra start column that holds
     row i; cur = root.  Repeat: mark cur used; i0 = the row cur holds; for every unused column j: c = a[i0][j] - u[i0] -
     v[j], if c < minv[j]: minv[j] = c, way[j] = cur; delta = the minimum of minv over the unused columns and j1 the
     LOWEST column that attains it; every used column (root included): u[row it holds] += delta, v[col] -= delta; every
     unused column: minv[j] -= delta; cur = j1; stop when cur holds no row.  Walk back: while cur != root: prev =
     way[cur], cur takes the row prev held, cur = prev;
  3. detection i is matched to slot j iff column j holds row i, j < T and q[i][j] > 0.

The switches (``ge`` of quantise; ``highest`` and ``keep_zero`` of solve) are planted faults: tests/
test_trackopt_reference.py shows that the gauge tells the rule from each of them; their defaults are the rule.
"""
import numpy as np

from tests import posenms_reference as PR
from tests import track_reference as TR

SCALE = np.float64(2.0 ** 40)
INF = 1 << 62


def weight(oks, thr, ge=False):
    oks, thr = np.float64(oks), np.float64(thr)
    if not (oks >= thr if ge else oks > thr):
        return 0
    return 1 + int(np.floor(min(oks - thr, np.float64(1.0)) * SCALE))


def quantise(oks, live, thr, ge=False):
    """oks [D, T] float64, live [T] bool (at entry) -> q [D][T] ints."""
    oks = np.asarray(oks, dtype=np.float64)
    D, T = oks.shape
    return [[weight(oks[i, j], thr, ge) if live[j] else 0 for j in range(T)] for i in range(D)]


def solve(q, highest=False, keep_zero=False):
    """q [D][T] -> (slots [D]: the slot of every detection or -1, the number of inner steps)."""
    D = len(q)
    T = len(q[0]) if D else 0
    m = max(D, T)
    a = [[-q[i][j] if j < T else 0 for j in range(m)] for i in range(D)]
    ROOT = m
    u, v = [0] * D, [0] * (m + 1)
    holds = [-1] * (m + 1)                              # the row a column holds; holds[ROOT] is the row being added
    steps = 0
    for i in range(D):
        minv, used, way = [INF] * m, [False] * (m + 1), [ROOT] * m
        holds[ROOT] = i
        cur = ROOT
        while True:
            steps += 1
            used[cur] = True
            i0 = holds[cur]
            for j in range(m):
                if not used[j]:
                    c = a[i0][j] - u[i0] - v[j]
                    if c < minv[j]:
                        minv[j], way[j] = c, cur
            unused = [j for j in range(m) if not used[j]]
            delta = min(minv[j] for j in unused)
            j1 = (max if highest else min)(j for j in unused if minv[j] == delta)
            for j in range(m + 1):
                if used[j]:
                    u[holds[j]] += delta
                    v[j] -= delta
            for j in unused:
                minv[j] -= delta
            cur = j1
            if holds[cur] < 0:
                break
        assert steps <= (i + 1) * (m + 1)
        while cur != ROOT:
            prev = way[cur]
            holds[cur] = holds[prev]
            cur = prev
    slots = [-1] * D
    for j in range(T):
        i = holds[j]
        if i >= 0 and (keep_zero or q[i][j] > 0):
            slots[i] = j
    return slots, steps


def total(q, slots):
    return sum(q[i][j] for i, j in enumerate(slots) if j >= 0)


def margin(q):
    """The optimum total minus the best total among the matchings that lack at least one pair of the optimum (each
    optimal pair's weight set to 0 in turn, solved again, the largest of those totals); INF without an optimal pair."""
    slots, _ = solve(q)
    best, others = total(q, slots), []
    for i, j in enumerate(slots):
        if j >= 0:
            without = [list(r) for r in q]
            without[i][j] = 0
            others.append(total(without, solve(without)[0]))
    return best - max(others) if others else INF


EXAMPLE = ((0.9, 0.8), (0.85, 0.1))                         # pair OKS; with match_thr 0.3 greedy switches an identity


def crossing_pair(sigmas, areas=(100.0, 1500.0, 44.0)):
    """Two frames of two people whose pair OKS in the second frame is EXAMPLE to about 1e-12: frame 0 holds A and B
    (born into slots 0 and 1, area ``areas[0]``), frame 1 detection 0 (the higher score, area ``areas[1]``) and
    detection 1 (area ``areas[2]``).  Every keypoint of a person sits at the same point, so the OKS of a pair is a
    function f of their distance alone; the radii come from bisection on f and the detections sit where the circles
    about A = (0, 0) and B = (L, 0) meet.  The three areas give the two detections different scales: with one scale
    the four radii admit no L."""
    sigmas = np.asarray(sigmas, dtype=np.float64)
    K = sigmas.size
    at, a0, a1 = areas

    def person(x, y):
        return np.tile(np.array([x, y], dtype=np.float64), (K, 1))

    def oks_at(r, area):
        return PR.pair_oks(person(r, 0.0), person(0.0, 0.0), area, at, sigmas)

    def radius(target, area):
        lo, hi = 0.0, 1.0
        while oks_at(hi, area) > target:
            hi *= 2.0
        for _ in range(200):
            mid = (lo + hi) / 2.0
            lo, hi = (mid, hi) if oks_at(mid, area) > target else (lo, mid)
        return (lo + hi) / 2.0

    r = [[radius(EXAMPLE[i][j], a) for j in range(2)] for i, a in enumerate((a0, a1))]
    lo = max(abs(r[i][0] - r[i][1]) for i in range(2))
    hi = min(r[i][0] + r[i][1] for i in range(2))
    assert lo < hi, ("the four circles admit no distance between A and B", r)
    L = (lo + hi) / 2.0
    dets = []
    for i in range(2):
        x = (r[i][0] ** 2 - r[i][1] ** 2 + L * L) / (2.0 * L)
        dets.append(person(x, np.sqrt(r[i][0] ** 2 - x * x) * (1.0 if i == 0 else -1.0)))
    ones = np.ones((2, K))
    first = TR.make_frame(np.stack([person(0.0, 0.0), person(L, 0.0)]), [0.9, 0.8], [at, at], ones)
    second = TR.make_frame(np.stack(dets), [0.9, 0.8], [a0, a1], ones)
    return first, second


class Tracker(TR.Tracker):
    """track_reference.Tracker with rule 3 (the greedy walk) replaced by ``solve``; the state, ageing, the One-Euro step
    and the births are that module's.  Each stream's result also carries ``q`` (the weights), ``slots`` and ``oks_seen``
    (every OKS of a detection and a live slot)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        assert not any(self.switches.values()), "the greedy gauge's switches do not apply"

    def _update_stream(self, st, frame, t):
        kpts, area, vis = frame["kpts"], frame["area"], frame["vis"]
        if self.vis_thr is not None and vis is None:
            raise ValueError("vis_thr needs visibilities")
        D, T, K = kpts.shape[0], self.max_tracks, self.K
        order = PR.visiting_order(frame["score"])
        ids = np.full(D, -1, dtype=np.int64)
        out = np.array(kpts, dtype=np.float64)
        oks_out = np.zeros(D)
        born = np.zeros(D, dtype=bool)
        live = st.id >= 0                                   # at entry
        events = dict(match=0, birth=0, expiry=0, reid=0, overflow=0, reinit=0)

        oks = np.zeros((D, T))                              # rows in visiting order
        for p, d in enumerate(order):
            for j in np.nonzero(live)[0]:
                oks[p, j] = PR.pair_oks(kpts[d], st.kp[j], area[d], st.area[j], self.sigmas,
                                        None if vis is None else vis[d], st.vis[j], self.vis_thr)
        q = quantise(oks, live, self.match_thr)
        slots, steps = solve(q)
        match = {order[p]: (j, oks[p, j]) for p, j in enumerate(slots) if j >= 0}
        taken = np.zeros(T, dtype=bool)
        taken[[j for j, _ in match.values()]] = True

        for j in range(T):                                  # ageing
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

        for d, (j, v) in match.items():                     # matched pairs
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

        for d in order:                                     # births
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
        return dict(ids=ids, keypoints=out, oks=oks_out, born=born, events=events, order=order, q=q, slots=slots,
                    steps=steps, oks_seen=[float(x) for x in oks[:, live].reshape(-1)], n_live=int(live.sum()))
