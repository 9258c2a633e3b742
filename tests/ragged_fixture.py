"""The small ragged batch that tests/test_ragged.py (CPU) and tests/test_ragged_gpu.py share: M = 11 detections of three
interleaved groups, K = 3.  Group 0 and group 1 have five detections each, group 2 has one.  Scores tie inside a group
(detections 2 and 7 of group 0; 6 and 8 of group 1, the last two of their group, so with four slots or max_dets = 4
that tie decides who is left out) and across groups (0.9 in groups 0 and 1, 0.7 in both).  Every detection is a jittered
copy of one of five people (two per large group), so PoseNMS suppresses some, the tracker matches them in a second
frame and the evaluator finds its ground truths.  Read-only arrays; nothing here touches the package.
"""
import functools

import numpy as np

K, M, SIDE, SIGMA = 3, 11, 100.0, 0.05
POS = np.array([0, 1, 0, 2, 1, 0, 1, 0, 1, 0, 1])
SCORE = np.array([0.9, 0.9, 0.7, 0.5, 0.7, 0.8, 0.6, 0.7, 0.6, 0.3, 0.95])
PERSON = np.array([0, 2, 0, 4, 2, 1, 3, 0, 3, 1, 2])          # persons 0, 1 are in group 0; 2, 3 in group 1; 4 in 2
LEVEL = np.array([0.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.6, 0.6, 0.1, 0.6])       # jitter: OKS 1, 0.99, 0.67 with the GT
# the batch in another order: both ties the other way round (8 before 6, 7 before 2), groups first seen 1, 2, 0
SHUFFLE = np.array([8, 3, 9, 0, 6, 10, 7, 2, 1, 5, 4])


@functools.lru_cache(maxsize=None)
def batch():
    """dict(pos [M], score [M], area [M], kpts [M, K, 2], vis [M, K], kpts2 [M, K, 2] (the poses a frame later),
    people: [5] dicts(group, kpts [K, 3] with v = 2, bbox xywh, area))."""
    rng = np.random.default_rng(3)
    people = []
    for p in range(5):
        centre = np.array([400.0 * p, 300.0])
        kp = centre + rng.uniform(0.0, SIDE, (K, 2))
        lo, hi = kp.min(axis=0), kp.max(axis=0)
        people.append(dict(group=int(POS[np.nonzero(PERSON == p)[0][0]]), area=0.6 * SIDE * SIDE,
                           kpts=np.concatenate([kp, np.full((K, 1), 2.0)], axis=1),
                           bbox=np.array([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])))
    jitter = lambda level: level[:, None, None] * SIDE * 2 * SIGMA * rng.uniform(-1.0, 1.0, (M, K, 2))
    kpts = np.stack([people[p]["kpts"][:, :2] for p in PERSON]) + jitter(LEVEL)
    kpts2 = kpts + 0.01 * SIDE + jitter(np.full(M, 0.05))
    out = dict(pos=POS.copy(), score=SCORE.copy(), area=0.6 * SIDE * SIDE * rng.uniform(0.95, 1.05, M), kpts=kpts,
               kpts2=kpts2, vis=rng.uniform(0.3, 1.0, (M, K)))
    for a in out.values():
        a.setflags(write=False)
    out["people"] = tuple(people)
    return out


def groups(order=None):
    """[(group, the batch indices of its detections in the order ``order`` gives them)] in first-seen order of the
    batch taken in ``order`` (None: as it is)."""
    order = np.arange(M) if order is None else np.asarray(order)
    seen = list(dict.fromkeys(POS[order].tolist()))
    return [(g, order[POS[order] == g]) for g in seen]
