"""The ValidationMeter gauge (tests/valmeter_reference.py) against brute force, and against the reference's balanced
accuracy (probpose_pytorch_amd.loss._binary_accuracy, loss.py:653-697).  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import valmeter_reference as vr

THR = np.arange(0.1, 1.0, 0.05)


_batch = vr.random_batch


def _state_of(batches, K, thr=THR):
    st = vr.empty_state(K, len(thr))
    for b in batches:
        vr.update(st, thr, *b)
    return st


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_brute_force_binary_head():
    """AUROC by counting every (pos, neg) pair on bin indices; ECE, MCE and Brier from the per-sample quantised values
    in exact rationals; all must equal the gauge's fields, which are those rationals rounded once."""
    rng = np.random.default_rng(0)
    B, K, E = 60, 3, 16
    batch = _batch(rng, B, K)
    rep = vr.report(_state_of([batch], K), THR, E)
    prob, in_image, annotated = batch[0], batch[4], batch[5]
    for row in range(K + 1):
        cols = slice(row, row + 1) if row < K else slice(0, K)
        keep = annotated[:, cols] == 1
        p, y = prob[:, cols][keep], in_image[:, cols][keep]
        bins = [int(b) for b in vr.fine_bin(p)]
        pos = [b for b, lab in zip(bins, y) if lab]
        neg = [b for b, lab in zip(bins, y) if not lab]
        wins2 = sum(2 * (a > b) + (a == b) for a in pos for b in neg)
        got = rep["probability"]
        assert got["auroc"][row] == float(Fraction(wins2, 2 * len(pos) * len(neg)))
        qp = [int(v) for v in vr.q_fixed(p, vr.Q30)]
        qp2 = [int(v) for v in vr.q_fixed(p.astype(np.float64) ** 2, vr.Q30)]
        n = len(qp)
        brier = sum(Fraction(a2 - 2 * int(lab) * a + int(lab) * vr.Q30, vr.Q30) for a, a2, lab in zip(qp, qp2, y)) / n
        assert got["brier"][row] == float(brier)
        true_brier = float(np.mean((p.astype(np.float64) - y) ** 2))
        assert abs(got["brier"][row] - true_brier) <= 3 * 2.0 ** -31 + 4 * 2.0 ** -53      # Q30 rounds p and p^2
        ece, mce = Fraction(0), Fraction(-1)
        for c in range(E):
            members = [i for i, b in enumerate(bins) if b // (1024 // E) == c]
            if not members:
                assert got["reliability"][row, c, 0] == 0 and math.isnan(got["reliability"][row, c, 1])
                continue
            conf = sum(Fraction(qp[i], vr.Q30) for i in members)
            hit = sum(int(y[i]) for i in members)
            ece += abs(conf - hit)
            mce = max(mce, abs(conf - hit) / len(members))
            assert got["reliability"][row, c, 0] == len(members)
            assert got["reliability"][row, c, 1] == float(conf / len(members))
            assert got["reliability"][row, c, 2] == float(Fraction(hit, len(members)))
        assert got["ece"][row] == float(ece / n) and got["mce"][row] == float(mce)
        assert got["n_pos"][row] == len(pos) and got["n_neg"][row] == len(neg)
        assert got["base_rate"][row] == float(Fraction(len(pos), n))
        # bal_acc from the samples: strict float64 comparison
        for j, t in enumerate(THR):
            tp = sum(1 for v, lab in zip(p, y) if lab and float(v) > t)
            tn = sum(1 for v, lab in zip(p, y) if not lab and not float(v) > t)
            want = (Fraction(tp, len(pos)) + Fraction(tn, len(neg))) / 2
            assert got["bal_acc"][row, j] == float(want)


def test_pearson_against_corrcoef():
    """The state sums Q30 of x, t, x^2, t^2, x t separately, each within 2^-31 of the true value, so cov, var x and
    var t are each within 3 * 2^-31 of numpy's; for r = cov / sqrt(vx vt) that is at most
    3 * 2^-31 * (1 / sqrt(vx vt) + (1 / vx + 1 / vt) / 2), first order, plus corrcoef's own float64 noise."""
    rng = np.random.default_rng(1)
    B, K = 80, 2
    batch = _batch(rng, B, K, ties=False)
    batch[7] = np.clip(0.6 * batch[2] + 0.4 * batch[7], 0, 1).astype(np.float32)      # correlated targets
    rep = vr.report(_state_of([batch], K), THR)
    keep = (batch[4] == 1) & (batch[5] == 1)
    for row in range(K + 1):
        cols = slice(row, row + 1) if row < K else slice(0, K)
        x = batch[2][:, cols][keep[:, cols]].astype(np.float64)
        t = batch[7][:, cols][keep[:, cols]].astype(np.float64)
        vx, vt = x.var(), t.var()
        tol = 3 * 2.0 ** -31 * (1 / math.sqrt(vx * vt) + (1 / vx + 1 / vt) / 2) * 1.5 + 1e-13
        assert abs(rep["oks"]["pearson"][row] - np.corrcoef(x, t)[0, 1]) <= tol
        assert abs(rep["oks"]["mae"][row] - np.abs(x - t).mean()) <= 2.0 ** -30
        assert abs(rep["oks"]["bias"][row] - (x.mean() - t.mean())) <= 2.0 ** -30
        assert abs(rep["oks"]["rmse"][row] ** 2 - ((x - t) ** 2).mean()) <= 2.0 ** -30


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_equal_classes_reproduce_the_reference_exactly(seed):
    """n_pos == n_neg: loss.py:653-697 subsamples nothing, whatever it draws."""
    from probpose_pytorch_amd.loss import _binary_accuracy
    rng = np.random.default_rng(100 + seed)
    n = 64
    p = rng.random((n, 1), dtype=np.float32)
    p[rng.integers(0, n, 8), 0] = np.float32(0.15)
    label = np.zeros((n, 1), np.int64)
    label[rng.permutation(n)[: n // 2]] = 1
    ones = np.ones((n, 1), np.int64)
    st = vr.empty_state(1, len(THR))
    vr.update(st, THR, p, p, p, p, label, ones, ones, p, p)
    rep = vr.report(st, THR)["probability"]
    np.random.seed(seed)
    acc, thr = _binary_accuracy(p, label, ones.astype(bool), None, force_balanced=True)
    assert np.float32(rep["best_bal_acc"][0]) == acc.numpy() and np.float32(rep["best_thr"][0]) == thr.numpy()


def test_unequal_classes_are_the_expectation_of_the_reference():
    """At ONE threshold the reference's balanced accuracy (the same numpy calls as loss.py:661-690) is (m hits of the
    whole smaller class + a uniform m-subset of the larger) / 2m.  Only the subset is random: a hypergeometric count
    whose variance is at most m q (1 - q), q the larger class's true rate, so the accuracy's standard deviation is at
    most sqrt(q (1 - q) / m) / 2 and the mean of D draws has that over sqrt(D).  Six standard errors."""
    rng = np.random.default_rng(5)
    n_pos, n_neg, j, draws = 20, 90, 6, 400
    p = rng.random(n_pos + n_neg, dtype=np.float32)
    gt = np.arange(n_pos + n_neg) < n_pos
    col = lambda a: np.asarray(a).reshape(-1, 1)     # noqa: E731
    ones = np.ones((len(p), 1), np.int64)
    st = vr.empty_state(1, len(THR))
    vr.update(st, THR, col(p), col(p), col(p), col(p), col(gt.astype(np.int64)), ones, ones, col(p), col(p))
    want = vr.report(st, THR)["probability"]["bal_acc"][0, j]
    np.random.seed(11)
    accs = []
    for _ in range(draws):
        pos_idx, neg_idx = np.where(gt)[0], np.where(~gt)[0]
        np.random.shuffle(pos_idx)
        np.random.shuffle(neg_idx)
        idx = np.concatenate([pos_idx[:n_pos], neg_idx[:n_pos]])
        accs.append(((p[idx] > THR[j]) == gt[idx]).sum() / len(idx))
    q = float((~(p[~gt] > THR[j])).mean())
    se = math.sqrt(q * (1 - q) / n_pos) / 2 / math.sqrt(draws)
    assert abs(np.mean(accs) - want) <= 6 * se
    assert se < 0.004          # the check has teeth: a one-sided rate (TPR or TNR alone) is off by far more


def test_state_is_invariant_under_order_and_split():
    rng = np.random.default_rng(2)
    B, K = 24, 5
    whole = _batch(rng, B, K)
    base = _state_of([whole], K)
    perm = rng.permutation(B)
    assert _equal(base, _state_of([[a[perm] for a in whole]], K))
    parts = [[a[s] for a in whole] for s in (slice(0, 7), slice(7, 8), slice(8, B))]
    split = _state_of(parts, K)
    swapped = _state_of(parts[::-1], K)
    for name in base:
        if name != "scalars":       # the batch count differs, by construction
            assert np.array_equal(base[name], split[name]), name
    assert _equal(split, swapped)


def test_validity_and_populations():
    K = 2
    ones, zeros = np.ones((1, K), np.int64), np.zeros((1, K), np.int64)
    half = np.full((1, K), 0.5, np.float32)
    for head, name in enumerate(("probability", "visibility", "oks", "error")):
        for bad in (np.nan, -0.1, 1.5, np.inf):
            args = [half.copy() for _ in range(4)]
            args[head][0, 0] = bad
            st = vr.empty_state(K, len(THR))
            vr.update(st, THR, *args, ones, ones, ones, half, half)
            rej = vr.report(st, THR)["rejected"]
            if name == "error" and bad == 1.5:
                assert sum(rej.values()) == 0
                continue
            assert rej[name] == 1 and sum(rej.values()) == 1
            n = [st["hist"][0].sum(), st["hist"][1].sum(), st["oks_hist"].sum(), st["err"][:, 0].sum()]
            assert n == [2 - (head == i) for i in range(4)]
    st = vr.empty_state(K, len(THR))
    two = ones.copy()
    two[0, 1] = 2
    vr.update(st, THR, half, half, half, half, two, ones, ones, half, half)
    assert vr.report(st, THR)["rejected"]["mask"] == 1 and st["hist"].sum() == 2 and st["all"][0] == 2
    # the error bound: 2^20 is accepted, the next float32 is not
    st = vr.empty_state(K, len(THR))
    e = np.array([[2 ** 20, np.nextafter(np.float32(2 ** 20), np.float32(np.inf))]], np.float32)
    vr.update(st, THR, half, half, half, e, ones, ones, ones, half, half)
    assert st["err"][:, 0].tolist() == [1, 0] and st["rejected"][4] == 1
    # nothing annotated: only the whole-set counters move
    st = vr.empty_state(K, len(THR))
    vr.update(st, THR, half, half, half, half, ones, zeros, ones, half, half)
    rep = vr.report(st, THR)
    assert st["hist"].sum() == 0 and st["all"].tolist() == [2, 2, 2 ** 30]
    assert rep["probability"]["best_bal_acc"][K] == 0.0 and math.isnan(rep["probability"]["auroc"][K])
    assert rep["mean_prob"] == 0.5 and math.isnan(rep["oks"]["mae"][K])


def test_thresholds_compare_in_float64():
    """float32(0.15) lies above the float64 threshold 0.15000000000000002; a value equal to a threshold is not above."""
    assert float(np.float32(0.15)) > THR[1]
    exact = np.float32(0.5)
    thr = np.array([THR[1], 0.5])
    p = np.array([[np.float32(0.15)], [exact]], np.float32)
    ones = np.ones((2, 1), np.int64)
    st = vr.empty_state(1, 2)
    vr.update(st, thr, p, p, p, p, ones, ones, ones, p, p)
    assert st["above"][0, 0, 1].tolist() == [2, 0]
