"""The gauge of PoseTrackEval: the CLEAR-MOT and identity metrics restated in plain loops on Python ints and numpy
float64.  Written from the rule (include/probpose_hip.h), not from the kernels and not from any evaluation
package.

  make_frame(...)                                   a frame dict with empty arrays for whatever is not given
  frame_oks(frame, sigmas) -> s [G, D]              cocoeval_reference.compute_oks with the predictions as detections
  weights(s, thr, prev, pred_ids) -> q [G][D]       the integer weights of a frame
  clear_sequence(frames, oks, thr) -> record        TP FN FP IDSW MT PT ML Frag, the OKS sum, per-frame details
  identity_sequence(frames, oks, thr) -> record     c, IDTP IDFN IDFP
  ratios(record) -> MOTA MOTP IDF1 IDP IDR          a ratio whose denominator is 0 is NaN
  evaluate(sequences, sigmas, thresholds) -> dict   what PoseTrackEval.evaluate returns, plus "details"

A frame is a dict: gt_ids [G] int, gt_kpts [G, K, 3], gt_bbox [G, 4], gt_area [G], pred_ids [D] int, pred_kpts
[D, K, 2|3].  ``sequences`` is a dict name -> list of frames in time order (insertion order is kept).

The rule.  CLEAR, per sequence and threshold, frames in order; per ground-truth identity ``last`` (the predicted identity
it was matched to most recently) and ``prev`` (the one it was matched to in the frame immediately before, none if it
was absent or unmatched there).  q[i][j] = 0 unless s[i][j] >= thr (a NaN is inadmissible), else 1 + floor(min(s - thr,
1.0) * 2^32) + (2^42 if prev[gt i] == pred j).  The assignment is trackopt_reference.solve(q).  TP / FN / FP count the
matches; IDSW += 1 for a matched (g, p) whose last[g] exists and is not p; the matched s add up to the OKS sum.  Per
identity: present, matched, runs (maximal runs of consecutive frames of the sequence in which it is matched); MT iff
5 matched > 4 present, ML iff 5 matched < present, PT otherwise; Frag += max(0, runs - 1).  Identity: c[a][b] = frames
with both present and s >= thr; IDTP = the largest total of c over one-to-one assignments (solve again).

The switches (``no_bonus``, ``switch_from_prev``, ``gt``, ``runs_over_present``) are planted faults:
tests/test_trackeval_reference.py shows that the gauge tells the rule from each of them; their defaults are the rule.
"""
import numpy as np

from tests.cocoeval_reference import compute_oks
from tests.trackopt_reference import solve, total

SCALE = np.float64(2.0 ** 32)
BONUS = 1 << 42
INT_KEYS = ("TP", "FN", "FP", "IDSW", "MT", "PT", "ML", "Frag", "IDTP", "IDFN", "IDFP")
RATIO_KEYS = ("MOTA", "MOTP", "IDF1", "IDP", "IDR")
NAN = float("nan")


def make_frame(gt_ids=(), gt_kpts=None, gt_bbox=None, gt_area=None, pred_ids=(), pred_kpts=None, K=17):
    gt_ids = np.asarray(gt_ids, dtype=np.int64).reshape(-1)
    pred_ids = np.asarray(pred_ids, dtype=np.int64).reshape(-1)
    G, D = gt_ids.size, pred_ids.size
    return dict(gt_ids=gt_ids,
                gt_kpts=np.zeros((0, K, 3)) if gt_kpts is None else np.asarray(gt_kpts, dtype=np.float64),
                gt_bbox=np.zeros((G, 4)) if gt_bbox is None else np.asarray(gt_bbox, dtype=np.float64).reshape(G, 4),
                gt_area=np.zeros(G) if gt_area is None else np.asarray(gt_area, dtype=np.float64).reshape(G),
                pred_ids=pred_ids,
                pred_kpts=np.zeros((0, K, 2)) if pred_kpts is None else np.asarray(pred_kpts, dtype=np.float64))


def frame_oks(frame, sigmas):
    """s [G, D] float64: rows the ground truths, columns the predictions, both in the order given."""
    G, D = len(frame["gt_ids"]), len(frame["pred_ids"])
    if G == 0 or D == 0:
        return np.zeros((G, D))
    return compute_oks(frame["pred_kpts"], frame["gt_kpts"], frame["gt_bbox"], frame["gt_area"], sigmas).T.copy()


def admissible(s, thr, gt=False):
    s, thr = np.float64(s), np.float64(thr)
    return bool(s > thr) if gt else bool(s >= thr)


def weight(s, thr, continued=False, gt=False):
    if not admissible(s, thr, gt):
        return 0
    q = 1 + int(np.floor(min(np.float64(s) - np.float64(thr), np.float64(1.0)) * SCALE))
    return q + (BONUS if continued else 0)


def weights(s, thr, prev, pred_ids, no_bonus=False, gt=False):
    """s [G, D]; prev [G]: the predicted identity each row continues, or None -> q [G][D] ints."""
    G, D = s.shape
    return [[weight(s[i, j], thr, not no_bonus and prev[i] is not None and prev[i] == int(pred_ids[j]), gt)
             for j in range(D)] for i in range(G)]


def clear_sequence(frames, oks, thr, no_bonus=False, switch_from_prev=False, gt=False, runs_over_present=False):
    """The CLEAR half for one sequence and threshold.  ``oks`` is the list of frame_oks results."""
    last, prev = {}, {}                                     # ground-truth identity -> predicted identity
    present, matched, runs, in_run = {}, {}, {}, {}
    tp = fn = fp = idsw = 0
    oks_sum = np.float64(0.0)
    details = []
    for frame, s in zip(frames, oks):
        gids = [int(g) for g in frame["gt_ids"]]
        pids = [int(p) for p in frame["pred_ids"]]
        G, D = len(gids), len(pids)
        q = weights(s, thr, [prev.get(g) for g in gids], pids, no_bonus=no_bonus, gt=gt)
        slots, steps = solve(q) if G else ([], 0)
        pairs = [(i, j) for i, j in enumerate(slots) if j >= 0]
        tp, fn, fp = tp + len(pairs), fn + G - len(pairs), fp + D - len(pairs)
        now = {}
        for i, j in pairs:
            g, p = gids[i], pids[j]
            seen = prev.get(g) if switch_from_prev else last.get(g)
            if seen is not None and seen != p:
                idsw += 1
            oks_sum = oks_sum + s[i, j]
            last[g] = p
            now[g] = p
        for g in gids:
            present[g] = present.get(g, 0) + 1
            if g in now:
                matched[g] = matched.get(g, 0) + 1
                if not in_run.get(g, False):
                    runs[g] = runs.get(g, 0) + 1
                in_run[g] = True
            else:
                in_run[g] = False
        if not runs_over_present:                           # a frame it is absent from ends an identity's run
            for g in in_run:
                if g not in now:
                    in_run[g] = False
        prev = now
        details.append(dict(q=q, slots=slots, steps=steps, total=total(q, slots) if G else 0))
    mt = pt = ml = frag = 0
    for g, n in present.items():
        m = matched.get(g, 0)
        if 5 * m > 4 * n:
            mt += 1
        elif 5 * m < n:
            ml += 1
        else:
            pt += 1
        frag += max(0, runs.get(g, 0) - 1)
    return dict(TP=tp, FN=fn, FP=fp, IDSW=idsw, MT=mt, PT=pt, ML=ml, Frag=frag, oks_sum=float(oks_sum),
                frames=details, present=present, matched=matched, runs=runs)


def identity_sequence(frames, oks, thr, gt=False, best_total=None):
    """The identity half: c over the identities in order of first appearance, and IDTP by the same solver.
    ``best_total(c)`` may stand in for the solver where plain loops over 1024 x 1024 take minutes: IDTP is the largest
    total, which is unique, so any exact solver returns it (tests/test_trackeval_reference.py holds ``solve`` against
    scipy's on the same matrices)."""
    gpos, ppos = {}, {}
    for frame in frames:
        for g in frame["gt_ids"]:
            gpos.setdefault(int(g), len(gpos))
        for p in frame["pred_ids"]:
            ppos.setdefault(int(p), len(ppos))
    c = [[0] * len(ppos) for _ in range(len(gpos))]
    n_gt = n_pred = 0
    for frame, s in zip(frames, oks):
        n_gt += len(frame["gt_ids"])
        n_pred += len(frame["pred_ids"])
        for i, g in enumerate(frame["gt_ids"]):
            for j, p in enumerate(frame["pred_ids"]):
                if admissible(s[i, j], thr, gt):
                    c[gpos[int(g)]][ppos[int(p)]] += 1
    idtp = (best_total(c) if best_total else total(c, solve(c)[0])) if c and ppos else 0
    return dict(IDTP=idtp, IDFN=n_gt - idtp, IDFP=n_pred - idtp, c=c)


def _ratio(num, den):
    return float(np.float64(num) / np.float64(den)) if den else NAN


def ratios(r):
    return dict(MOTA=1.0 - _ratio(r["FN"] + r["FP"] + r["IDSW"], r["TP"] + r["FN"]) if r["TP"] + r["FN"] else NAN,
                MOTP=_ratio(r["oks_sum"], r["TP"]),
                IDF1=_ratio(2 * r["IDTP"], 2 * r["IDTP"] + r["IDFP"] + r["IDFN"]),
                IDP=_ratio(r["IDTP"], r["IDTP"] + r["IDFP"]),
                IDR=_ratio(r["IDTP"], r["IDTP"] + r["IDFN"]))


def evaluate(sequences, sigmas, thresholds=(0.5,), no_bonus=False, switch_from_prev=False, gt=False,
             runs_over_present=False, best_total=None):
    """{"thresholds", "metrics": one dict per threshold (the integers summed over the sequences, oks_sum and the
    ratios), "per_sequence": name -> one dict of integers (and oks_sum) per threshold, "details": name -> per threshold
    the clear_sequence and identity_sequence results}."""
    thresholds = [float(t) for t in thresholds]
    per_sequence, details = {}, {}
    for name, frames in sequences.items():
        oks = [frame_oks(f, sigmas) for f in frames]
        per_sequence[name], details[name] = [], []
        for thr in thresholds:
            cl = clear_sequence(frames, oks, thr, no_bonus=no_bonus, switch_from_prev=switch_from_prev, gt=gt,
                                runs_over_present=runs_over_present)
            idn = identity_sequence(frames, oks, thr, gt=gt, best_total=best_total)
            rec = {k: (cl[k] if k in cl else idn[k]) for k in INT_KEYS}
            rec["oks_sum"] = cl["oks_sum"]
            per_sequence[name].append(rec)
            details[name].append(dict(clear=cl, identity=idn, oks=oks))
    metrics = []
    for t in range(len(thresholds)):
        tot = {k: sum(per_sequence[n][t][k] for n in per_sequence) for k in INT_KEYS}
        tot["oks_sum"] = float(sum(np.float64(per_sequence[n][t]["oks_sum"]) for n in per_sequence))
        tot.update(ratios(tot))
        metrics.append(tot)
    return dict(thresholds=thresholds, metrics=metrics, per_sequence=per_sequence, details=details)


# ------------------------------------------------------------------------------------------------ fixtures
def person(K, x, y, spread=10.0, seed=0):
    """[K, 2]: a person's keypoints around (x, y), the same shape for every call with the same K and seed."""
    rng = np.random.default_rng(1000 + seed)
    return np.array([x, y], dtype=np.float64) + rng.uniform(-spread, spread, (K, 2))


def gt_of(points, vis=2.0):
    """[G, K, 2] -> (gt_kpts [G, K, 3], bbox [G, 4], area [G]) with the box of the points and area = its area."""
    points = np.asarray(points, dtype=np.float64)
    G, K = points.shape[:2]
    kp = np.concatenate([points, np.full((G, K, 1), vis)], axis=2)
    lo, hi = points.min(axis=1), points.max(axis=1)
    wh = np.maximum(hi - lo, 1.0)
    return kp, np.concatenate([lo, wh], axis=1), wh[:, 0] * wh[:, 1]


def scene(K, tracks, n_frames, sigmas=None):
    """A sequence from a list of tracks.  A track is dict(gt=id or None, pred={frame: id} or id or None, at=(x, y),
    frames=range, shift={frame: dx} (the prediction's offset, default 0), v=(vx, vy)).  Each person is the same
    keypoint cloud moved to ``at + v * frame``; the prediction is that cloud shifted by dx along x."""
    frames = []
    for f in range(n_frames):
        gids, gpts, pids, ppts = [], [], [], []
        for n, tr in enumerate(tracks):
            if f not in tr.get("frames", range(n_frames)):
                continue
            vx, vy = tr.get("v", (0.0, 0.0))
            pts = person(K, tr["at"][0] + vx * f, tr["at"][1] + vy * f, seed=n)
            if tr.get("gt") is not None and f not in tr.get("gt_absent", ()):
                gids.append(tr["gt"]), gpts.append(pts)
            pred = tr.get("pred")
            pid = pred.get(f) if isinstance(pred, dict) else pred
            if pid is not None:
                pids.append(pid), ppts.append(pts + np.array([tr.get("shift", {}).get(f, 0.0), 0.0]))
        if gids:
            kp, bb, ar = gt_of(np.stack(gpts))
        else:
            kp, bb, ar = np.zeros((0, K, 3)), np.zeros((0, 4)), np.zeros(0)
        frames.append(make_frame(gids, kp, bb, ar, pids, np.stack(ppts) if pids else np.zeros((0, K, 2)), K=K))
    return frames


def cloud_frame(K, gt_x, pred_x, gt_ids, pred_ids):
    """One frame in which every person is the same keypoint cloud moved along x, so a pair's OKS depends on the distance
    of the two alone; gt_x / pred_x are the positions.  With area 400 and sigma 0.05: OKS = exp(-d^2 / 8)."""
    base = person(K, 0.0, 0.0)
    kp, bb, ar = gt_of(np.stack([base + (x, 0.0) for x in gt_x])) if len(gt_x) else (None, None, None)
    ar = None if ar is None else np.full(len(gt_x), 400.0)
    pk = np.stack([base + (x, 0.0) for x in pred_x]) if len(pred_x) else None
    return make_frame(gt_ids, kp, bb, ar, pred_ids, pk, K=K)


def continued_pair_frames(K):
    """Frame 0 pairs g0 - p0 and g1 - p1 beyond doubt; in frame 1 each prediction sits nearer the OTHER person, all
    four pairs admissible at 0.5 with sigma 0.05: the matching of largest OKS swaps the identities, the continued one
    has the lower OKS."""
    return [cloud_frame(K, (0.0, 3.0), (0.0, 3.0), (0, 1), (0, 1)),
            cloud_frame(K, (0.0, 3.0), (2.0, 1.0), (0, 1), (0, 1))]


# a person matched to 1, unmatched for one frame, then matched to 2: scene(K, ONE_FRAME_GAP, 5)
ONE_FRAME_GAP = [dict(gt=5, pred={0: 1, 1: 1, 3: 2, 4: 2}, at=(0, 0))]


def random_sequence(rng, K, n_frames, n_people, extent=600.0, miss_p=0.15, switch_p=0.1, stray_p=0.2, jitter=0.08,
                    blind_p=0.0, always=False):
    """A seeded sequence: people drift inside a square of side ``extent``, a tracker sees them with jitter (relative to
    their size), misses some, swaps or renews ids now and then, and adds strays.  Every person is one keypoint cloud
    with a small variation of its own, scaled by its size, and area = 0.6 size^2: with a small ``extent`` neighbours
    are admissible for one another and the assignment has to choose.  Ids are large and unordered.  ``blind_p``: the
    chance that a ground truth has no visible keypoint in a frame (it is then scored by its box).  ``always``:
    everybody is there from the first frame to the last."""
    side = rng.uniform(40.0, 120.0, n_people)
    pos = rng.uniform(0.0, extent, (n_people, 2))
    vel = rng.normal(0.0, 4.0, (n_people, 2))
    shape = rng.uniform(-0.5, 0.5, (K, 2)) + rng.uniform(-0.05, 0.05, (n_people, K, 2))
    gid = rng.permutation(10 ** 12 + np.arange(n_people) * 7919)
    pid = rng.permutation(5 * 10 ** 11 + np.arange(n_people) * 104729)
    next_pid = int(9 * 10 ** 11)
    life = [(0, n_frames) if always else
            (int(rng.integers(0, max(1, n_frames // 2))), int(rng.integers(n_frames // 2, n_frames + 1)))
            for _ in range(n_people)]
    frames = []
    for f in range(n_frames):
        gids, gpts, gside, pids, ppts = [], [], [], [], []
        order = [n for n in rng.permutation(n_people) if life[n][0] <= f < max(life[n][1], life[n][0] + 1)]
        for n in order:                                     # the tracker's mistakes come first: ids stay distinct
            if rng.random() < switch_p:
                if rng.random() < 0.5 and n_people > 1:
                    o = int(rng.integers(0, n_people))
                    pid[n], pid[o] = pid[o], pid[n]
                else:
                    pid[n], next_pid = next_pid, next_pid + 13
        for n in order:
            pts = pos[n] + vel[n] * f + shape[n] * side[n]
            gids.append(int(gid[n])), gpts.append(pts), gside.append(side[n])
            if rng.random() >= miss_p:
                pids.append(int(pid[n])), ppts.append(pts + rng.normal(0, 1, (K, 2)) * jitter * side[n] *
                                                      rng.choice([0.2, 1.0, 3.0]))
        if rng.random() < stray_p:
            pids.append(next_pid), ppts.append(rng.uniform(0, extent, 2) + rng.uniform(-30, 30, (K, 2)))
            next_pid += 13
        keep = rng.permutation(len(pids))
        pids, ppts = [pids[i] for i in keep], [ppts[i] for i in keep]
        if gids:
            kp = np.concatenate([np.stack(gpts), rng.integers(0, 3, (len(gids), K, 1)).astype(np.float64)], axis=2)
            kp[:, 0, 2] = 2.0
            kp[rng.random(len(gids)) < blind_p, :, 2] = 0.0
            gside = np.asarray(gside)
            centre = np.stack(gpts).mean(axis=1)
            bb = np.concatenate([centre - 0.1 * gside[:, None], np.repeat(0.2 * gside[:, None], 2, axis=1)], axis=1)
            ar = 0.6 * gside * gside
        else:
            kp, bb, ar = np.zeros((0, K, 3)), np.zeros((0, 4)), np.zeros(0)
        frames.append(make_frame(gids, kp, bb, ar, pids, np.stack(ppts) if pids else np.zeros((0, K, 2)), K=K))
    return frames


def many_identities(rng, n_ids, K=1, lanes=3, min_frames=1):
    """A sequence with exactly ``n_ids`` ground-truth and ``n_ids`` predicted identities built from short tracks: up to
    ``lanes`` people stand far apart; in every frame a lane's annotated id and, independently, its predicted id is
    replaced by a new one with chance 0.4 while ids remain; now and then a side of a lane is missing.  Two or three
    people per frame, so the OKS stage stays tiny while the identity stage sees n_ids x n_ids."""
    base = person(K, 0.0, 0.0)
    cur_g, cur_p = [None] * lanes, [None] * lanes
    new_g, new_p = [False] * lanes, [False] * lanes         # an id is shown at least once before it may go missing
    next_g = next_p = 0
    frames = []
    while next_g < n_ids or next_p < n_ids or len(frames) < min_frames:
        gids, gpts, pids, ppts = [], [], [], []
        for lane in range(lanes):
            if next_g < n_ids and (cur_g[lane] is None or rng.random() < 0.4):
                cur_g[lane], next_g, new_g[lane] = next_g, next_g + 1, True
            if next_p < n_ids and (cur_p[lane] is None or rng.random() < 0.4):
                cur_p[lane], next_p, new_p[lane] = next_p, next_p + 1, True
            pts = base + (300.0 * lane, 0.0)
            if cur_g[lane] is not None and (new_g[lane] or rng.random() >= 0.05):
                gids.append(3 * cur_g[lane] + 10 ** 9), gpts.append(pts)
            if cur_p[lane] is not None and (new_p[lane] or rng.random() >= 0.1):
                pids.append(7 * (n_ids - cur_p[lane])), ppts.append(pts + rng.normal(0.0, 0.5, (K, 2)))
            new_g[lane] = new_p[lane] = False
        if gids:
            kp, bb, _ = gt_of(np.stack(gpts))
            ar = np.full(len(gids), 400.0)
        else:
            kp, bb, ar = np.zeros((0, K, 3)), np.zeros((0, 4)), np.zeros(0)
        frames.append(make_frame(gids, kp, bb, ar, pids, np.stack(ppts) if pids else np.zeros((0, K, 2)), K=K))
    return frames


def min_threshold_gap(result):
    """The smallest |s - thr| over every OKS of the result's details and every threshold (inf without any)."""
    gap = float("inf")
    for name, per_thr in result["details"].items():
        for thr, d in zip(result["thresholds"], per_thr):
            for s in d["oks"]:
                if s.size:
                    gap = min(gap, float(np.abs(s - thr).min()))
    return gap
