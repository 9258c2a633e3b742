"""PoseTrackEval(hota=True) on the GPU against its gauge (tests/hota_reference.py).

Entry level: the OKS matrices are drawn directly as float64 and handed to the gauge and to the four pp_trackeval_hota_*
entries alike.  No exp() lies between them, both read the same bits, and the rule fixes every float operation, so pmc,
q, the held rows, the frames' and sequences' TP and mc are demanded exactly; loc and the three association sums within
relative 1e-12 (§4.7g's figure: far more than n * 2^-53, the bound on adding n terms of one sign in any order).

End to end through evaluate(): exp() may differ in its last bits between numpy and the device, so the fixture condition
is asserted on the gauge: no OKS within 1e-9 of an alpha, and the gauge's integers unchanged when its OKS matrices are
scaled by 1 +- 1e-12.

Shapes, the smallest at which each mechanism can go wrong: G or D of 0, 1, 63, 64, 65 and 256 (the lane boundary, a
second column per lane, the limit), G > D and D > G; entries equal to an alpha, zeros and NaNs; all-equal matrices (every
row's path goes through a held column); 1, 4 and 5 sequences (a partly filled workgroup of frames and of (sequence,
alpha) pairs); 1 and 19 alphas; 63 / 65 and 255 / 257 identities."""
import json
import math

import numpy as np
import pytest

from tests import hota_reference as H
from tests import trackeval_reference as R
from tests.cocoeval_reference import default_sigmas

pytestmark = pytest.mark.gpu
ALPHAS19 = H.DEFAULT_ALPHAS


# ------------------------------------------------------------------------------------------------ entry level
def _run_entries(seqs, oks, alphas):
    """The four entries on drawn matrices -> per sequence what the gauge's details hold, read back from the device."""
    import torch
    from probpose_pytorch_amd import _lib
    names = list(seqs)
    frames = [f for n in names for f in seqs[n]]
    mats = [m for n in names for m in oks[n]]
    S, F, A = len(names), len(frames), len(alphas)
    g_cnt = np.array([len(f["gt_ids"]) for f in frames], dtype=np.int64)
    d_cnt = np.array([len(f["pred_ids"]) for f in frames], dtype=np.int64)
    offs = np.zeros((3, F + 1), dtype=np.int64)
    offs[0, 1:], offs[1, 1:], offs[2, 1:] = np.cumsum(d_cnt), np.cumsum(g_cnt), np.cumsum(d_cnt * g_cnt)
    table = np.zeros((4, S + 1), dtype=np.int64)
    gt_idx, pred_idx, gt_present, pred_present = [], [], [], []
    for s, n in enumerate(names):
        gpos, ppos, ng, npr = {}, {}, [], []
        for f in seqs[n]:
            for g in f["gt_ids"]:
                a = gpos.setdefault(int(g), len(gpos))
                if a == len(ng):
                    ng.append(0)
                ng[a] += 1
                gt_idx.append(a)
            for p in f["pred_ids"]:
                b = ppos.setdefault(int(p), len(ppos))
                if b == len(npr):
                    npr.append(0)
                npr[b] += 1
                pred_idx.append(b)
        gt_present += ng
        pred_present += npr
        table[:, s + 1] = table[:, s] + (len(seqs[n]), len(gpos), len(ppos), len(gpos) * len(ppos))
    Dtot, Gtot, oks_total = (int(v) for v in offs[:, -1])
    n_gid, n_pid, c_total = (int(v) for v in table[1:, -1])
    flat = np.concatenate([np.asarray(m, dtype=np.float64).T.reshape(-1) for m in mats] + [np.zeros(1)])

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1))).cuda() \
            if np.asarray(a).size else torch.zeros(1, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")

    alphas = np.asarray(alphas, dtype=np.float64)
    d_offs, d_table, d_oks, d_alpha = dev(offs, np.int64), dev(table, np.int64), dev(flat, np.float64), \
        dev(alphas, np.float64)
    d_gi, d_pi = dev(gt_idx, np.int32), dev(pred_idx, np.int32)
    d_gp, d_pp = dev(gt_present, np.int64), dev(pred_present, np.int64)
    z = dict(device="cuda")
    pmc = torch.zeros(max(c_total, 1), dtype=torch.int64, **z)
    mc = torch.zeros(max(A * c_total, 1), dtype=torch.int32, **z)
    q = torch.full((max(oks_total, 1),), -7, dtype=torch.int64, **z)
    held = torch.full((max(Dtot, 1),), -7, dtype=torch.int32, **z)
    ftp = torch.full((max(F * A, 1),), -7, dtype=torch.int64, **z)
    floc = torch.full((max(F * A, 1),), -7.0, dtype=torch.float64, **z)
    tp = torch.full((max(S * A, 1),), -7, dtype=torch.int64, **z)
    sums = torch.full((max(4 * S * A, 1),), -7.0, dtype=torch.float64, **z)
    _lib.launch("pp_trackeval_hota_align", S, F, Dtot, Gtot, oks_total, c_total, offs, table, d_offs, d_table, d_oks,
                d_gi, d_pi, pmc)
    _lib.launch("pp_trackeval_hota_weights", S, F, Dtot, Gtot, oks_total, c_total, n_gid, n_pid, offs, table, d_offs,
                d_table, d_oks, d_gi, d_pi, pmc, d_gp, d_pp, q)
    _lib.launch("pp_trackeval_hota_match", S, A, F, Dtot, Gtot, oks_total, c_total, offs, table, alphas, d_offs,
                d_table, d_alpha, d_oks, q, d_gi, d_pi, mc, held, ftp, floc)
    _lib.launch("pp_trackeval_hota_assoc", S, A, F, c_total, n_gid, n_pid, table, d_table, mc, d_gp, d_pp, ftp, floc,
                tp, sums)
    torch.cuda.synchronize()
    pmc, mc, q, held, ftp, floc, tp, sums = (t.cpu().numpy() for t in (pmc, mc, q, held, ftp, floc, tp, sums))
    mc = mc[:A * c_total].reshape(A, c_total)
    ftp, floc = ftp[:F * A].reshape(F, A), floc[:F * A].reshape(F, A)
    tp, sums = tp[:S * A].reshape(S, A), sums[:4 * S * A].reshape(S, A, 4)
    out = {}
    for s, n in enumerate(names):
        f0, f1 = int(table[0, s]), int(table[0, s + 1])
        NG, NP = int(table[1, s + 1] - table[1, s]), int(table[2, s + 1] - table[2, s])
        c0 = int(table[3, s])
        out[n] = dict(
            pmc=pmc[c0:c0 + NG * NP].reshape(NG, NP).tolist(),
            mc=[mc[i, c0:c0 + NG * NP].reshape(NG, NP).tolist() for i in range(A)],
            q=[q[offs[2, f]:offs[2, f + 1]].reshape(int(g_cnt[f]), int(d_cnt[f])).tolist() for f in range(f0, f1)],
            held=[held[offs[0, f]:offs[0, f + 1]].tolist() for f in range(f0, f1)],
            frame_tp=ftp[f0:f1].sum(axis=0).tolist(), frame_loc=floc[f0:f1], TP=tp[s].tolist(),
            sums={k: sums[s, :, j].tolist() for j, k in enumerate(H.SUM_KEYS)})
    return out


def _entries_equal_the_gauge(seqs, oks, alphas):
    ref = H.evaluate(seqs, oks=oks, alphas=alphas)
    got = _run_entries(seqs, oks, alphas)
    for n in seqs:
        d, rec, g = ref["details"][n], ref["per_sequence_hota"][n], got[n]
        print(n, "TP", g["TP"], "steps", d["steps"], "loc", g["sums"]["loc_sum"][0], rec["loc_sum"][0], "assA",
              g["sums"]["assa_sum"][0], rec["assa_sum"][0])
        assert g["pmc"] == d["pmc"], n
        assert g["q"] == d["q"], n
        assert g["held"] == d["held"], n
        assert g["TP"] == rec["TP"] and g["frame_tp"] == rec["TP"], n
        assert g["mc"] == d["mc"], n
        assert np.all(g["frame_loc"] >= 0.0)
        for k in H.SUM_KEYS:
            for a, b in zip(g["sums"][k], rec[k]):
                assert abs(a - b) <= 1e-12 * abs(b), (n, k, a, b)
    return ref, got


def _frame(rng, gids, pids, values=None, zero_p=0.3):
    """(frame, s [G, D]): similarities uniform in (0.02, 1) with a share of zeros, or drawn from ``values``."""
    G, D = len(gids), len(pids)
    if values is None:
        s = rng.uniform(0.02, 1.0, (G, D)) * (rng.random((G, D)) >= zero_p)
    else:
        s = rng.choice(np.asarray(values, dtype=np.float64), size=(G, D))
    return R.make_frame(gids, pred_ids=pids, K=1), s


def _sequence(rng, shapes, n_gt, n_pred, **kw):
    """Frames of the given (G, D) whose ids are drawn from pools of n_gt / n_pred persistent identities."""
    frames, mats = [], []
    for G, D in shapes:
        f, s = _frame(rng, rng.choice(n_gt, G, replace=False) + 10 ** 9, rng.choice(n_pred, D, replace=False) * 7, **kw)
        frames.append(f), mats.append(s)
    return frames, mats


def _named(**pairs):
    return {n: p[0] for n, p in pairs.items()}, {n: p[1] for n, p in pairs.items()}


def test_entries_frame_sizes_at_the_lane_boundaries():
    rng = np.random.default_rng(1)
    shapes = [(0, 0), (0, 3), (3, 0), (1, 1), (63, 64), (64, 63), (65, 64), (64, 65), (1, 65), (65, 1), (5, 2)]
    seqs, oks = _named(sizes=_sequence(rng, shapes, 70, 70))
    ref, _ = _entries_equal_the_gauge(seqs, oks, ALPHAS19)
    assert ref["details"]["sizes"]["steps"] > 1.2 * sum(g for g, d in shapes if d)      # paths beyond the first step
    assert 0 < ref["hota"]["TP"][18] < ref["hota"]["TP"][0]


def test_entries_a_frame_at_the_limit():
    """256 on both sides, then on one side each, half of the pairs at 0.  The side frames are 230 wide: every row
    without a real column walks through the virtual ones, which is what the gauge's plain loops spend their time on."""
    rng = np.random.default_rng(2)
    seqs, oks = _named(limit=_sequence(rng, [(256, 256), (256, 230), (230, 256)], 256, 256, zero_p=0.5))
    ref, _ = _entries_equal_the_gauge(seqs, oks, (0.5,))
    assert ref["details"]["limit"]["steps"] > 2 * (256 + 256 + 230)
    assert ref["hota"]["TP"][0] > 500


def test_entries_values_equal_to_an_alpha_zeros_and_nans_in_five_sequences():
    """Every similarity is an alpha's own float64, 0, 1 or NaN: s >= alpha is decided at equality, weights tie, and the
    lowest column has to win.  Five sequences of one to five frames: the last workgroup of frames is partly filled."""
    rng = np.random.default_rng(3)
    values = list(ALPHAS19) + [0.0, 0.0, 0.0, 1.0, float("nan"), float("nan")]
    pairs = {}
    for s in range(5):
        shapes = [(int(rng.integers(0, 9)), int(rng.integers(0, 9))) for _ in range(s + 1)]
        pairs[("seq", s)] = _sequence(rng, shapes, 9, 9, values=values)
    seqs, oks = _named(**{str(k): v for k, v in pairs.items()})
    assert sum(len(f) for f in seqs.values()) % 4 != 0
    ref, _ = _entries_equal_the_gauge(seqs, oks, ALPHAS19)
    assert H.min_alpha_gap(ref) == 0.0 and ref["hota"]["TP"][0] > ref["hota"]["TP"][18] > 0


def test_entries_all_equal_matrices_in_four_sequences():
    """One frame of n x n equal similarities: all weights equal, every row after the first walks through a held column.
    65 x 70 and 130 x 130 take a second and a third column per lane."""
    rng = np.random.default_rng(4)
    pairs = {}
    for n, m, v in ((5, 5, 0.5), (64, 64, 0.25), (65, 70, 1.0), (130, 130, 0.7)):
        f = R.make_frame(np.arange(n) + 5, pred_ids=np.arange(m) * 3, K=1)
        pairs[f"equal{n}"] = ([f, f], [np.full((n, m), v), np.full((n, m), v)])
    seqs, oks = _named(**pairs)
    ref, got = _entries_equal_the_gauge(seqs, oks, (0.5,))
    assert ref["details"]["equal130"]["steps"] >= 2 * (2 * 130 - 1)
    assert got["equal130"]["held"][0] == list(range(130))     # the lowest column on equal minv: the diagonal
    assert ref["per_sequence_hota"]["equal64"]["TP"] == [0] and ref["per_sequence_hota"]["equal65"]["TP"] == [130]


@pytest.mark.parametrize("n_gt,n_pred", [(63, 65), (257, 255)])
def test_entries_identities_on_each_side_of_64_and_256(n_gt, n_pred):
    """Many short tracks: every frame shows some 50 identities, each identity in one or two frames."""
    rng = np.random.default_rng(n_gt)
    frames, mats = [], []
    per = 52 if n_gt > 64 else 21
    g_all, p_all = rng.permutation(n_gt) + 10 ** 6, rng.permutation(n_pred) * 11
    for k in range(0, max(n_gt, n_pred), per // 2):         # windows that overlap by half
        f, s = _frame(rng, g_all[k:k + per], p_all[k:k + per], zero_p=0.8)
        frames.append(f), mats.append(s)
    seqs, oks = _named(ids=(frames, mats))
    ref, _ = _entries_equal_the_gauge(seqs, oks, (0.3, 0.6))
    assert (len(ref["details"]["ids"]["ng"]), len(ref["details"]["ids"]["np"])) == (n_gt, n_pred)
    assert max(max(r) for r in ref["details"]["ids"]["mc"][0]) == 2


# ------------------------------------------------------------------------------------------------ end to end
def _device(seqs, sig, alphas=None, thresholds=(0.5,), hota=True, on_device=False):
    import torch
    from probpose_pytorch_amd import PoseTrackEval
    ev = PoseTrackEval(sig, thresholds=thresholds, hota=hota, hota_alphas=alphas)
    for name, frames in seqs.items():
        for f in frames:
            pk = torch.from_numpy(f["pred_kpts"]).cuda() if on_device else f["pred_kpts"]
            ev.add_frame(name, f["gt_ids"], f["gt_kpts"], f["gt_bbox"], f["gt_area"], f["pred_ids"], pk)
    return ev, ev.evaluate()


def _gauge(seqs, sig, alphas):
    """The gauge's result, with the fixture condition asserted on it."""
    ref = H.evaluate(seqs, sig, alphas)
    assert H.min_alpha_gap(ref) > 1e-9
    mats = {n: d["oks"] for n, d in ref["details"].items()}
    for scale in (1.0 + 1e-12, 1.0 - 1e-12):
        moved = H.evaluate(seqs, alphas=alphas, oks={n: [m * scale for m in ms] for n, ms in mats.items()})
        assert H.integers(moved) == H.integers(ref), scale
    return ref


def _same(got, ref):
    assert list(got["per_sequence_hota"]) == list(ref["per_sequence_hota"])
    for name, r in ref["per_sequence_hota"].items():
        g = got["per_sequence_hota"][name]
        print(name, g["TP"], g["loc_sum"][0], r["loc_sum"][0], g["assa_sum"][0], r["assa_sum"][0])
        for k in ("TP", "FN", "FP"):
            assert g[k] == r[k] and all(type(v) is int for v in g[k]), (name, k)
        for k in H.SUM_KEYS:
            for a, b in zip(g[k], r[k]):
                assert abs(a - b) <= 1e-12 * abs(b), (name, k, a, b)
    g, r = got["hota"], ref["hota"]
    assert g["alphas"] == r["alphas"] and all(g[k] == r[k] for k in ("TP", "FN", "FP"))
    assert list(g["curves"]) == list(H.CURVES)
    for k in H.CURVES:
        assert abs(g[k] - r[k]) <= 1e-12 * abs(r[k]), k
        for a, b in zip(g["curves"][k], r["curves"][k]):
            assert abs(a - b) <= 1e-12 * abs(b), k


@pytest.mark.parametrize("K,n_seq,n_alpha", [(1, 4, 19), (17, 5, 19), (17, 1, 1)])
def test_evaluate_equals_the_gauge(K, n_seq, n_alpha):
    rng = np.random.default_rng(10 * K + n_seq)
    seqs = {}
    for s in range(n_seq):                                  # odd ones crowded: the alignment has to choose
        seqs[("cam", s)] = R.random_sequence(rng, K, int(rng.integers(2, 9)), int(rng.integers(2, 8)),
                                             extent=60.0 if s % 2 else 600.0, blind_p=0.1)
    alphas = ALPHAS19 if n_alpha == 19 else (0.5,)
    ref = _gauge(seqs, default_sigmas(K), alphas)
    _, got = _device(seqs, default_sigmas(K), None if n_alpha == 19 else alphas, on_device=bool(n_seq % 2))
    _same(got, ref)
    assert 0.0 < got["hota"]["HOTA"] < 1.0 and got["hota"]["TP"][0] > 0
    assert set(got) == {"thresholds", "metrics", "per_sequence", "hota", "per_sequence_hota"}


def test_twice_the_same_reset_and_hota_off():
    rng = np.random.default_rng(3)
    K, sig = 3, np.full(3, 0.05)
    seqs = {s: R.random_sequence(rng, K, 6, 5, extent=60.0) for s in range(3)}
    ev, first = _device(seqs, sig, thresholds=(0.4, 0.6))
    second = ev.evaluate()
    assert second["hota"] == first["hota"] and second["per_sequence_hota"] == first["per_sequence_hota"]
    assert second["per_sequence"] == first["per_sequence"]
    _, plain = _device(seqs, sig, thresholds=(0.4, 0.6), hota=False)
    assert set(plain) == {"thresholds", "metrics", "per_sequence"}
    assert plain["per_sequence"] == first["per_sequence"]   # the CLEAR and identity results do not depend on hota
    ev.reset()
    empty = ev.evaluate()
    assert empty["per_sequence_hota"] == {} and empty["hota"]["TP"] == [0] * 19
    assert all(empty["hota"][k] == 0.0 for k in H.CURVES if k != "LocA") and empty["hota"]["LocA"] == 1.0


def test_eight_launches_by_name_and_nothing_waits_before_the_readback(monkeypatch):
    import torch
    from probpose_pytorch_amd import _lib
    rng = np.random.default_rng(4)
    seqs = {s: R.random_sequence(rng, 3, 5, 4) for s in range(6)}
    ev, first = _device(seqs, np.full(3, 0.05), thresholds=(0.4, 0.6), on_device=True)      # warm
    names, launch = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a: (names.append(name), launch(name, *a))[1])
    b = ev._tables()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, sizes, keep = ev._enqueue(b)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert names == ["pp_cocoeval_oks", "pp_trackeval_clear", "pp_trackeval_overlap", "pp_trackeval_identity",
                     "pp_trackeval_hota_align", "pp_trackeval_hota_weights", "pp_trackeval_hota_match",
                     "pp_trackeval_hota_assoc"]
    again = ev._finish(b, out.cpu().numpy(), *sizes)
    assert again["per_sequence_hota"] == first["per_sequence_hota"] and again["hota"] == first["hota"]
    del names[:]
    ev.hota = False
    assert "hota" not in ev.evaluate() and len(names) == 4


def test_a_clean_clip_through_the_tracker_scores_one():
    """Two people walk past each other at a distance; PoseTracker's ids and keypoints go back in as predictions against
    the poses it was given.  Every OKS is 1, so every alpha up to 1.0 is reached."""
    import torch
    from probpose_pytorch_amd import PoseTrackEval, PoseTracker
    K = 17
    sig = default_sigmas(K)
    tracker = PoseTracker(sig)
    alphas = ALPHAS19 + (1.0,)
    ev = PoseTrackEval(sig, hota=True, hota_alphas=alphas)
    base = R.person(K, 0.0, 0.0, spread=40.0)
    for f in range(8):
        pts = np.stack([base + (3.0 * f, 0.0), base + (500.0 - 3.0 * f, 200.0)])
        kp, bb, ar = R.gt_of(pts)
        res = tracker.update(torch.from_numpy(pts).cuda(), torch.from_numpy(ar).cuda(),
                             torch.tensor([0.9, 0.8], dtype=torch.float64).cuda())
        ev.add_frame("clip", [11, 22], kp, bb, ar, res.ids.cpu().numpy(), res.keypoints)
    h = ev.evaluate()["hota"]
    assert h["TP"] == [16] * 20 and h["FN"] == [0] * 20 and h["FP"] == [0] * 20
    for k in H.CURVES:
        assert h["curves"][k] == [1.0] * 20 and h[k] == 1.0, k


def test_the_command_line_prints_the_hota_line(tmp_path, capsys):
    """--hota on what inference.py --track wrote, scored against its own poses: one more JSON line, all ones."""
    from probpose_pytorch_amd import inference, trackeval
    from tests.test_track_inference import ARGS, BOXES, write_frames
    names, table = write_frames(tmp_path / "frames")
    out = tmp_path / "out"
    record = inference.main(ARGS + ["--frames", str(tmp_path / "frames"), "--boxes-json", str(table), "--track",
                                    "--output", str(out)])
    gt = []
    for f, r in enumerate(record):
        boxes = BOXES if f % 2 == 0 else BOXES[::-1]
        gt.append(dict(frame=r["frame"], persons=[
            dict(id=100 + (i if f % 2 == 0 else 1 - i), keypoints=[[x, y, 2.0] for x, y in d["keypoints"]],
                 bbox=box[:4], area=box[2] * box[3]) for i, (d, box) in enumerate(zip(r["detections"], boxes))]))
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    capsys.readouterr()
    argv = [str(tmp_path / "gt.json"), str(out / "tracks.json"), "--thr", "0.5", "--sigmas", "0.05", "--seq", "clip"]
    assert trackeval.main(argv) == 0
    without = capsys.readouterr().out.strip().splitlines()
    assert trackeval.main(argv + ["--hota"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[:-1] == without and len(without) == 2      # without the flag the output is unchanged
    row = json.loads(lines[-1])
    assert list(row) == list(H.CURVES) + ["alphas", "curve"]
    assert row["alphas"] == list(ALPHAS19) and row["curve"] == [1.0] * 19
    assert all(row[k] == 1.0 for k in H.CURVES) and math.isfinite(row["HOTA"])
