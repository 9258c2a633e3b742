"""The gauge of HeadCalibration (tests/calibration_reference.py) against a brute force, and its properties.  No GPU.

The brute force is the min-max formula of isotonic regression, y_i = max_{a<=i} min_{b>=i} (sum_{a..b} P / sum_{a..b} n)
over the non-empty bins, in Fractions.

Round trip: on the data it was fitted on, every row on its own table, isotonic regression preserves the weighted mean,
so the exact mean_conf over the exact block values IS base_rate.  The gauge's mean_conf takes the float32 table values
instead: each differs from its block value by two roundings (float64 division 2^-53, float32 2^-24, relative), the
weighted mean of values <= 1 inherits that relative error, and both reports round once more (2^-53 each).  Bound:
|mean_conf - base_rate| <= base_rate (2^-24 + 2^-53) (1 + 2^-53) + 2 * 2^-53.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import calibration_reference as cr
from tests import valmeter_reference as vr

THR = np.arange(0.1, 1.0, 0.05)


def brute_force(P, n):
    idx = [i for i, w in enumerate(n) if w]
    vals = {}
    for pos, i in enumerate(idx):
        best = None
        for a in range(pos + 1):
            low = None
            for b in range(pos, len(idx)):
                seg = idx[a:b + 1]
                v = Fraction(sum(P[j] for j in seg), sum(n[j] for j in seg))
                low = v if low is None or v < low else low
            best = low if best is None or low > best else best
        vals[i] = best
    return vals


def random_bins(rng):
    m = int(rng.integers(1, 25))
    n = rng.integers(0, 4, size=m)              # zero weights mixed in
    if rng.random() < 0.5:
        n = n * int(rng.integers(1, 4))
    P = np.array([int(rng.integers(0, w + 1)) if w else 0 for w in n])       # small ranges: ties are common
    return [int(v) for v in P], [int(v) for v in n]


def test_pav_against_the_min_max_formula():
    rng = np.random.default_rng(0)
    pooled_ties = 0
    for _ in range(400):
        P, n = random_bins(rng)
        per_bin, blocks = cr.isotonic_blocks(P, n)
        want = brute_force(P, n)
        nonempty = [i for i, w in enumerate(n) if w]
        if not nonempty:
            assert per_bin == [(0, 0)] * len(P) and blocks == []
            continue
        for i in nonempty:                                              # the values, as Fractions
            assert Fraction(*per_bin[i]) == want[i], (P, n, i)
        # blocks are the maximal runs of equal fitted value: they tile the bins, increase strictly, and hold their sums
        assert blocks[0][0] == 0 and blocks[-1][1] == len(P)
        for (s0, e0, p0, w0), (s1, e1, p1, w1) in zip(blocks, blocks[1:]):
            assert e0 == s1 and Fraction(p0, w0) < Fraction(p1, w1)
        for s, e, p, w in blocks:
            assert p == sum(P[s:e]) and w == sum(n[s:e]) and w > 0
            assert s == 0 or n[s] > 0                                   # a block starts at a non-empty bin ...
            pooled_ties += len({want[i] for i in range(s, e) if n[i]}) == 1 and sum(1 for i in range(s, e) if n[i]) > 1
        # ... so an empty bin carries the nearest non-empty bin to its left, the leading ones the first block
        for i, w in enumerate(n):
            if w == 0:
                left = [j for j in nonempty if j < i]
                assert per_bin[i] == per_bin[left[-1] if left else nonempty[0]]
    assert pooled_ties > 50


def test_equal_neighbours_pool():
    per_bin, blocks = cr.isotonic_blocks([1, 2, 3], [2, 4, 6])
    assert blocks == [(0, 3, 6, 12)] and per_bin == [(6, 12)] * 3


def random_state(seed, K=3, J=18, batches=2, B=64):
    rng = np.random.default_rng(seed)
    state = vr.empty_state(K, J)
    for _ in range(batches):
        vr.update(state, THR[:J], *vr.random_batch(rng, B, K))
    return state


def test_fit_properties():
    K, J = 3, 18
    state = random_state(1)
    counts = [[int(cr.head_rows(state, h)[1][k].sum()) for k in range(K)] for h in range(3)]
    mc = sorted(c for row in counts for c in row)[4]                    # some rows below, some at or above
    blocks, table, row_of = cr.fit(state, K, J, mc)
    assert table.dtype == np.float32 and blocks.dtype == np.int64 and row_of.dtype == np.int32
    assert (np.diff(table, axis=-1) >= 0).all() and (table >= 0).all() and (table <= 1).all()
    for h in range(3):
        for k in range(K):
            assert row_of[h, k] == (k if counts[h][k] >= mc else K)
    assert (row_of == K).any() and (row_of < K).any()
    # the pool row is fitted on the summed state, not averaged from the keypoint rows
    P, n = cr.head_rows(state, 0)
    assert blocks[0, K].tolist() == [list(b) for b in cr.isotonic_blocks(P[:K].sum(0), n[:K].sum(0))[0]]


def test_empty_state_passes_through():
    K, J = 2, 1
    blocks, table, row_of = cr.fit(vr.empty_state(K, J), K, J, 1)
    assert (blocks == 0).all() and (table == 0).all() and (row_of == -1).all()
    aux = np.random.default_rng(0).random((3, 5, K), dtype=np.float32)
    assert cr.apply(aux, table, row_of).tobytes() == aux.tobytes()
    # one head seen, the others not: only that head gets rows
    state = vr.empty_state(K, J)
    state["hist"][1, 0, 1, 700] = 3
    _, _, row_of = cr.fit(state, K, J, 2)
    assert row_of.tolist() == [[-1, -1], [0, K], [-1, -1]]


def oks_wrap_bins():
    """Bins 500 and 501 of an OKS row, 2^20 samples each: Q30 sums 2^49 + 2^44 (mean achieved OKS 0.516) and
    2^49 + 2^30 (0.500001).  Left > right, so the exact fit pools them.  The products with N = 2^20 are 2^69 + 2^64 and
    2^69 + 2^50: modulo 2^64 they are 0 and 2^50, signed or unsigned, and a 64-bit comparison keeps the bins apart."""
    P, n = [0] * cr.BINS, [0] * cr.BINS
    n[500] = n[501] = 2 ** 20
    P[500], P[501] = 2 ** 49 + 2 ** 44, 2 ** 49 + 2 ** 30
    return P, n


def test_wrapped_products_would_order_blocks_wrongly():
    """The case the GPU test runs, under masked 64-bit arithmetic: the wrapped comparison orders the two blocks the
    wrong way, so a kernel that multiplied in int64 would fail that test."""
    P, n = oks_wrap_bins()
    assert P[500] * n[501] >= P[501] * n[500]
    assert cr.wrapped_mul(P[500], n[501]) < cr.wrapped_mul(P[501], n[500])
    exact, blocks = cr.isotonic_blocks(P, n)
    wrapped, wblocks = cr.isotonic_blocks(P, n, cr.wrapped_mul)
    assert blocks == [(0, cr.BINS, P[500] + P[501], 2 ** 21)] and len(wblocks) == 2
    assert exact != wrapped


def test_round_trip_on_the_fitting_state():
    K, J = 3, 18
    state = random_state(2)
    _, table, row_of = cr.fit(state, K, J, 1)
    assert (row_of == np.arange(K)).all()
    got = cr.score(state, K, J, table, row_of, 16)
    want = vr.report(state, THR, 16)
    for head in ("probability", "visibility"):
        base = want[head]["base_rate"]
        bound = base * (2.0 ** -24 + 2.0 ** -53) * (1 + 2.0 ** -53) + 2 * 2.0 ** -53
        assert (np.abs(got[head]["mean_conf"] - base) <= bound).all(), head
        assert (got[head]["n"] == want[head]["n_pos"] + want[head]["n_neg"]).all()
        assert (got[head]["skipped"] == 0).all()
    assert (got["oks"]["n"] == want["oks"]["n"]).all()
    # per row, on its own table, the calibrated OKS and the achieved OKS have the same mean: every E bin is a union of
    # whole blocks there, so the ECE of the fitting data is zero up to the float32 table
    assert (got["oks"]["ece"][:K] <= 2.0 ** -23).all()


def test_score_skips_rows_without_a_table():
    K, J = 3, 18
    state = random_state(3)
    _, table, row_of = cr.fit(state, K, J, 1)
    row_of[0, 1] = -1
    got = cr.score(state, K, J, table, row_of, 8)
    n1 = float(cr.head_rows(state, 0)[1][1].sum())
    assert got["probability"]["skipped"].tolist() == [0.0, n1, 0.0, n1]
    assert got["probability"]["n"][1] == 0 and np.isnan(got["probability"]["brier"][1])
    assert np.isnan(got["probability"]["reliability"][1, :, 1:]).all()
    assert got["probability"]["n"][K] == got["probability"]["n"][0] + got["probability"]["n"][2]


def test_report_parsing():
    from probpose_pytorch_amd import calibration
    E, K = 4, 2
    F = calibration.score_fields(E)
    assert F == 15 + 9 * E
    rep = np.arange((K + 1) * F, dtype=np.float64).reshape(K + 1, F)
    out = calibration.parse_score(rep, E)
    assert list(out) == ["probability", "visibility", "oks"]
    assert list(out["probability"]) == ["n", "skipped", "brier", "mean_conf", "ece", "mce", "reliability"]
    assert list(out["oks"]) == ["n", "skipped", "ece", "reliability"]
    assert out["probability"]["n"].tolist() == [0.0, F, 2.0 * F]
    assert out["visibility"]["n"][0] == 6 + 3 * E and out["oks"]["n"][0] == 2 * (6 + 3 * E)
    assert out["oks"]["reliability"].shape == (K + 1, E, 3)
    assert out["oks"]["reliability"][0, 0, 0] == 2 * (6 + 3 * E) + 3
    assert out["oks"]["reliability"][-1, -1, -1] == (K + 1) * F - 1


def test_state_dict_round_trip(tmp_path):
    from probpose_pytorch_amd import HeadCalibration
    K, J = 3, 18
    blocks, table, row_of = cr.fit(random_state(4), K, J, 50)
    cal = HeadCalibration(torch.from_numpy(table), torch.from_numpy(blocks), torch.from_numpy(row_of), 50)
    assert cal.K == K and cal.min_count == 50
    sd = cal.state_dict()
    assert sorted(sd) == ["K", "blocks", "min_count", "row_of", "table"]
    other = HeadCalibration.from_state_dict(sd)
    cal.save(tmp_path / "cal.pt")
    loaded = HeadCalibration.load(tmp_path / "cal.pt", "cpu")
    for c in (other, loaded):
        assert c.K == K and c.min_count == 50
        assert torch.equal(c.table, cal.table) and torch.equal(c.blocks, cal.blocks)
        assert torch.equal(c.row_of, cal.row_of)
    blank = HeadCalibration(torch.zeros_like(cal.table), torch.zeros_like(cal.blocks), torch.zeros_like(cal.row_of), 1)
    blank.load_state_dict(sd)
    assert torch.equal(blank.table, cal.table) and blank.min_count == 50
    with pytest.raises(ValueError):
        HeadCalibration(cal.table[:, :2], cal.blocks, cal.row_of, 1)
    with pytest.raises(ValueError):
        HeadCalibration.from_state_dict(dict(sd, K=K + 1))


def test_calibration_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from probpose_pytorch_amd import HeadCalibration, _lib
    blocks, table, row_of = cr.fit(vr.empty_state(2, 1), 2, 1, 1)
    cal = HeadCalibration(torch.from_numpy(table), torch.from_numpy(blocks), torch.from_numpy(row_of), 1)
    with pytest.raises(_lib.HipExtensionError):
        cal.apply(torch.zeros((3, 1, 2)))
    with pytest.raises(_lib.HipExtensionError):
        HeadCalibration.fit(None)
    with pytest.raises(_lib.HipExtensionError):
        cal.score(None)
