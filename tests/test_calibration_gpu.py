"""HeadCalibration on the GPU against the gauge (tests/calibration_reference.py).  States are written directly as int64
tensors in the meter's layout, so no model is needed.

Fit and apply are compared for equality (``torch.equal`` / the int32 views of the floats).  The score's counts are
compared for equality and its quotients within bounds counted in float64 roundings, u = 2^-53.  T is the number of
(keypoint, fine bin) cells of the row: 1024 per keypoint that has a table; E the number of ECE bins.  The device sums
in no fixed order, so every sum of m non-negative terms is charged m - 1 roundings, relative to the sum.

  brier       each term pos (1-y)^2 + neg y^2 takes at most 5 roundings (1-y, its square, two products by counts, one
              sum; y^2 is exact, y has 24 bits), the sum T - 1, the division 1, the gauge's own rounding 1:
              relative (T + 6) u, the bound the issue states.
  mean_conf   n_b y_b rounds once (31 + 24 bits), the sum T - 1, the division 1, the gauge 1: relative (T + 2) u.
  reliability mean calibrated value: as mean_conf over the cells of one bin, relative (T + 2) u.  Observed frequency:
              integers, one division, the gauge: relative 2 u.  Mean achieved OKS: the Q30 sum converts with one
              rounding, the division, the gauge: relative 3 u.
  ece         sum_e |S_e - t_e| / n.  S_e carries at most T u S_e, t_e at most u t_e, and sum S_e <= n, sum t_e <= n
              (table values and targets are at most 1): absolute (T + 1) u before the subtraction; the subtraction, the
              sum over E bins, the division and the gauge add (E + 3) u relative to an ECE of at most 1:
              absolute (T + E + 4) u.
  mce         max_e |S_e - t_e| / c_e with S_e <= c_e, t_e <= c_e: absolute (T + 1) u, then the subtraction, the
              division and the gauge, 3 u relative to at most 1: absolute (T + 4) u.

End to end: a second meter fed with the calibrated predictions.  Its pooled mean_conf is sum Q30(y) / (n 2^30): Q30
rounds each sample by at most 2^-31 absolute, y is the float32 of the float64 quotient of its block (2^-24 + 2^-53
relative), and the exact weighted mean of the block values is the base rate, so
|mean_conf - base_rate| <= base_rate (2^-24 + 2^-53) (1 + 2^-53) + 2^-31 + 2 u (the two reports round once each).
"""
import functools

import numpy as np
import pytest
import torch

from tests import calibration_reference as cr
from tests import valmeter_reference as vr
from tests.test_calibration_reference import oks_wrap_bins

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
THR = np.arange(0.1, 1.0, 0.05)
SECTIONS = list(vr.empty_state(1, 1))


def words(state) -> torch.Tensor:
    """The state dict of the gauge as the meter's int64 words on the device."""
    return torch.from_numpy(np.concatenate([state[name].reshape(-1) for name in SECTIONS])).cuda()


def meter_with(state, K, J):
    """A ValidationMeter whose device state is ``state`` (the calibration reads J, never the thresholds)."""
    from probpose_pytorch_amd import ValidationMeter
    meter = ValidationMeter(None, thresholds=THR[:J] if J <= len(THR) else np.linspace(0.01, 0.99, J))
    meter._ensure(K, torch.device("cuda", torch.cuda.current_device()))
    w = words(state)
    assert w.shape == meter._state.shape
    meter._state.copy_(w)
    return meter


def put(state, h, k, P, n):
    """Row (h, k) of the state takes numerators P and weights n over the fine bins."""
    P, n = np.asarray(P, dtype=np.int64), np.asarray(n, dtype=np.int64)
    if h < 2:
        state["hist"][h, k, 1], state["hist"][h, k, 0] = P, n - P
    else:
        state["oks_st"][k], state["oks_hist"][k] = P, n


def check_fit(state, K, J, min_count):
    from probpose_pytorch_amd import HeadCalibration
    cal = HeadCalibration.fit(meter_with(state, K, J), min_count=min_count)
    blocks, table, row_of = cr.fit(state, K, J, min_count)
    assert torch.equal(cal.row_of.cpu(), torch.from_numpy(row_of))
    assert torch.equal(cal.blocks.cpu(), torch.from_numpy(blocks))
    assert torch.equal(cal.table.cpu().view(torch.int32), torch.from_numpy(table).view(torch.int32))
    return cal, (blocks, table, row_of)


B_ = np.arange(1024)


def _empties():
    rng = np.random.default_rng(11)
    n = rng.integers(1, 50, size=1024)
    n[:100] = 0
    n[B_ % 7 == 3] = 0
    n[400:451] = 0
    n[900:] = 0
    return rng.integers(0, n + 1), n


def _straddle():
    """Increasing, but decreasing across each of 15/16, 63/64, 255/256, 511/512 (and over 254..257), so that blocks lie
    across the lane, wave and half boundaries of any partition."""
    P = 2 * B_ + 2
    for a in (15, 63, 255, 511):
        P[a], P[a + 1] = P[a + 1], P[a]
    P[254:258] = P[254:258][::-1].copy()
    return P, np.full(1024, 4096)


def _cascade():
    """(b + 1) / 2048 rising over bins 0..1022, then a heavy bin of zeros at 1023: the pooled tail falls below every
    block before it, down to bin 0 (523775 / 1073093056 < 1 / 2048).  The row holds 1.07e9 samples, below 2^31."""
    P, n = B_ + 1, np.full(1024, 2048)
    P[1023], n[1023] = 0, 1_071_000_000
    return P, n


def _near_2_31():
    P, n = np.zeros(1024, dtype=np.int64), np.zeros(1024, dtype=np.int64)
    n[10], P[10] = 2 ** 30, 2 ** 30 - 1
    n[20], P[20] = 2 ** 30 - 1, 2 ** 30 - 2          # 2^31 - 1 samples; the right value is the smaller by 2^-60
    return P, n


def _one_bin(b):
    P, n = np.zeros(1024, dtype=np.int64), np.zeros(1024, dtype=np.int64)
    n[b], P[b] = 5, 2
    return P, n


PATTERNS = {
    "empty": lambda: (np.zeros(1024, dtype=np.int64), np.zeros(1024, dtype=np.int64)),
    "one_bin_0": lambda: _one_bin(0),
    "one_bin_1023": lambda: _one_bin(1023),
    "increasing": lambda: (B_.copy(), np.full(1024, 2048)),
    "decreasing": lambda: (1023 - B_, np.full(1024, 2048)),
    "equal_neighbours": lambda: ((B_ // 8) * (1 + B_ % 3), 200 * (1 + B_ % 3)),
    "empties": _empties,
    "straddle": _straddle,
    "cascade": _cascade,
    "near_2_31": _near_2_31,
}


def pattern_state(name, K, J, h):
    """The pattern in row (h, K // 2); with K = 3 the other keypoints of that head hold a little data of their own,
    except where the row alone is near 2^31 samples."""
    state = vr.empty_state(K, J)
    put(state, h, K // 2, *PATTERNS[name]())
    if K > 1 and name not in ("near_2_31", "empty"):
        rng = np.random.default_rng(3)
        for k in (0, K - 1):
            n = rng.integers(0, 3, size=1024)
            put(state, h, k, rng.integers(0, n + 1) * (2 ** 20 if h == 2 else 1), n)
    return state


@pytest.mark.parametrize("K,J", [(1, 1), (3, 18)])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_fit_patterns(name, K, J):
    for h in ((0, 2) if name in ("empties", "straddle") else (1,)):
        P, n = PATTERNS[name]()
        state = pattern_state(name, K, J, h)
        if h == 2:                                  # the same shape as Q30 sums: numerators scaled by 2^20
            put(state, 2, K // 2, np.asarray(P) * 2 ** 20, n)
        _, (blocks, _, row_of) = check_fit(state, K, J, 1)
        row = [tuple(v) for v in blocks[h, K // 2].tolist()]
        runs = 1 + sum(a != b for a, b in zip(row, row[1:]))
        want = dict(empty=1, one_bin_0=1, one_bin_1023=1, increasing=1024, decreasing=1, equal_neighbours=128,
                    cascade=1, near_2_31=1).get(name)
        assert want is None or runs == want, (name, runs)       # the gauge itself pools what the case is about
        assert row_of[h, K // 2] == (-1 if name == "empty" else K // 2)


@pytest.mark.parametrize("K,J", [(1, 1), (3, 18)])
def test_fit_oks_products_beyond_64_bits(K, J):
    """N = 2^20 per bin, Q30 sums near 2^49: P_l N_r is about 2^69.  tests/test_calibration_reference.py shows that the
    comparison wrapped to 64 bits orders these two blocks the wrong way."""
    state = vr.empty_state(K, J)
    put(state, 2, K // 2, *oks_wrap_bins())
    _, (blocks, table, _) = check_fit(state, K, J, 1)
    assert (blocks[2, K // 2] == [2 ** 50 + 2 ** 44 + 2 ** 30, 2 ** 21]).all()
    assert table[2, K // 2, 0] == np.float32((2 ** 50 + 2 ** 44 + 2 ** 30) / 2 ** 21 / 2 ** 30)


def random_state(seed, K, J, batches=2, B=64):
    rng = np.random.default_rng(seed)
    state = vr.empty_state(K, J)
    for _ in range(batches):
        vr.update(state, THR[:J], *vr.random_batch(rng, B, K))
    return state


@pytest.mark.parametrize("seed", range(5))
def test_fit_random_states(seed):
    K, J = (1, 1) if seed == 4 else (3, 18)
    check_fit(random_state(seed, K, J), K, J, 20)


def test_min_count_just_above_and_below():
    K, J = 3, 18
    state = random_state(7, K, J)
    count = int(cr.head_rows(state, 1)[1][2].sum())
    for mc, want in ((count, 2), (count + 1, K), (count - 1, 2)):
        _, (_, _, row_of) = check_fit(state, K, J, mc)
        assert row_of[1, 2] == want


def test_fit_and_score_read_their_sections_whatever_lies_between():
    """The same hist / oks_hist / oks_st at K = 2 (the smallest K at which every section's keypoint stride counts) under
    J = 1, 7 and 64 (the cap), which moves ``above`` and all behind it; every word of the sections the calibration does
    not read is -1.  An offset that is off lands in a sentinel or in another keypoint's bins."""
    K = 2
    content = random_state(31, K, 1)
    got = []
    for J in (1, 7, 64):
        state = vr.empty_state(K, J)
        for name in ("hist", "oks_hist", "oks_st"):
            state[name][:] = content[name]
        for name in ("conf", "above", "sum_p", "sum_p2", "oks_sx"):
            state[name][:] = -1
        cal, (_, table, row_of) = check_fit(state, K, J, 70)     # rows of their own and rows sent to the pool
        assert set(row_of.reshape(-1).tolist()) == {0, 1, K}
        score, want = cal.score(meter_with(state, K, J)), cr.score(state, K, J, table, row_of, 16)
        counts = [score[head][name] if name != "reliability" else score[head][name][:, :, 0]
                  for head in cr.HEADS for name in ("n", "skipped", "reliability")]
        for c, head in zip(counts[::3], cr.HEADS):
            assert np.array_equal(c, want[head]["n"]) and c[-1] > 0, head
        got.append((cal, counts))
    for cal, counts in got[1:]:
        for name in ("blocks", "table", "row_of"):
            assert torch.equal(getattr(cal, name), getattr(got[0][0], name)), name
        assert all(np.array_equal(a, b) for a, b in zip(counts, got[0][1]))


# ----------------------------------------------------------------------------------------------- apply
@functools.lru_cache(maxsize=None)
def fitted(K):
    """A gauge fit on a seeded state of K keypoints, with a row_of that mixes own rows, the pool and pass-through in
    every head.  Shared by the apply and score tests; never written to."""
    J = 18
    state = random_state(20 + K, K, J, batches=1, B=128)
    blocks, table, row_of = cr.fit(state, K, J, 1)
    for h in range(3):
        for k in range(K):
            row_of[h, k] = (k, K, -1)[(h + k) % 3]
    for a in (blocks, table, row_of):
        a.setflags(write=False)
    return state, blocks, table, row_of


def device_calibration(K):
    from probpose_pytorch_amd import HeadCalibration
    _, blocks, table, row_of = fitted(K)
    return HeadCalibration(torch.from_numpy(table.copy()).cuda(), torch.from_numpy(blocks.copy()).cuda(),
                           torch.from_numpy(row_of.copy()).cuda(), 1)


def edge_inputs():
    """Every bin edge i / 1024 with its float32 neighbours on both sides, and what is not a probability."""
    e = (np.arange(1025, dtype=np.float32) / np.float32(1024)).astype(np.float32)
    v = np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2)),
                        np.array([1.0, -0.0, -0.25, 1.5, np.inf, -np.inf], dtype=np.float32)])
    nans = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001], dtype=np.uint32).view(np.float32)
    return np.concatenate([v, nans])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def test_apply_at_every_bin_edge():
    K = 3
    cal = device_calibration(K)
    _, _, table, row_of = fitted(K)
    v = edge_inputs()
    B = len(v)
    # every value in every (h, k) column
    aux = np.stack([np.stack([np.roll(v, 7 * (h + k)) for k in range(K)], axis=1) for h in range(3)])
    assert aux.shape == (3, B, K)
    want = cr.apply(aux, table, row_of)
    got = cal.apply(torch.from_numpy(aux).cuda()).cpu().numpy()
    assert same_bits(got, want)
    assert same_bits(got[0, :, 2], aux[0, :, 2])                     # row_of -1: the whole column passes
    assert not same_bits(got[0, :, 0], aux[0, :, 0])


@pytest.mark.parametrize("B,K", [(1, 1), (21, 3), (13, 5), (257, 1), (64, 17)])
def test_apply_shapes_in_and_out_of_place(B, K):
    cal = device_calibration(K)
    _, _, table, row_of = fitted(K)
    rng = np.random.default_rng(B * K)
    aux = rng.random((3, B, K), dtype=np.float32)
    v = edge_inputs()
    idx = rng.integers(0, aux.size, size=max(1, aux.size // 4))
    aux.reshape(-1)[idx] = v[rng.integers(0, len(v), size=len(idx))]
    want = cr.apply(aux, table, row_of)
    d = torch.from_numpy(aux).cuda()
    out = cal(d)
    assert same_bits(d.cpu().numpy(), aux) and same_bits(out.cpu().numpy(), want)
    given = torch.full_like(d, 7.0)
    assert cal.apply(d, out=given) is given and same_bits(given.cpu().numpy(), want)
    assert cal.apply(d, out=d) is d and same_bits(d.cpu().numpy(), want)


def test_apply_replays_from_a_graph():
    """One launch, nothing allocated or synchronised: a captured apply follows new values in its input."""
    K = 3
    cal = device_calibration(K)
    _, _, table, row_of = fitted(K)
    rng = np.random.default_rng(8)
    first, second = rng.random((3, 21, K), dtype=np.float32), rng.random((3, 21, K), dtype=np.float32)
    d, out = torch.from_numpy(first).cuda(), torch.empty((3, 21, K), device="cuda")
    cal.apply(d, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cal.apply(d, out=out)
    d.copy_(torch.from_numpy(second))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), cr.apply(second, table, row_of))


def test_apply_refuses_what_does_not_fit():
    cal = device_calibration(3)
    with pytest.raises(ValueError):
        cal.apply(torch.zeros((3, 4, 2), device="cuda"))
    with pytest.raises(ValueError):
        cal.apply(torch.zeros((3, 4, 3), device="cuda", dtype=torch.float64))
    from probpose_pytorch_amd import _lib
    flat = torch.zeros((3 * 4 * 3 + 1,), device="cuda")
    with pytest.raises(_lib.HipExtensionError, match="overlap in part"):
        _lib.launch("pp_calib_apply", flat[:36], flat[1:], 4, 3, cal.table, cal.row_of)


# ----------------------------------------------------------------------------------------------- score
def check_score(got, want, row_of, K, E):
    for h, head in enumerate(cr.HEADS):
        g, w = got[head], want[head]
        included = (row_of[h] >= 0).astype(np.int64)
        T = 1024.0 * np.concatenate([included, [included.sum()]])
        assert np.array_equal(g["n"], w["n"]) and np.array_equal(g["skipped"], w["skipped"]), head
        assert np.array_equal(g["reliability"][:, :, 0], w["reliability"][:, :, 0]), head
        for name in g:
            assert np.array_equal(np.isnan(g[name]), np.isnan(w[name])), (head, name)

        def close(name, a, b, rel, absolute=0.0):
            err = np.nan_to_num(np.abs(a - b))
            bound = np.nan_to_num(np.abs(b)) * rel + absolute
            print(head, name, "largest error / bound:", float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)))
            assert (err <= bound).all(), (head, name)

        rel_T = ((T + 2) * U)[:, None]
        close("reliability mean", g["reliability"][:, :, 1], w["reliability"][:, :, 1], rel_T)
        close("reliability target", g["reliability"][:, :, 2], w["reliability"][:, :, 2], (2 if h < 2 else 3) * U)
        close("ece", g["ece"], w["ece"], 0.0, (T + E + 4) * U)
        if h < 2:
            close("brier", g["brier"], w["brier"], (T + 6) * U)
            close("mean_conf", g["mean_conf"], w["mean_conf"], (T + 2) * U)
            close("mce", g["mce"], w["mce"], 0.0, (T + 4) * U)


@pytest.mark.parametrize("E", [16, 1, 1024])
def test_score_against_the_gauge(E):
    K, J = 3, 18
    fit_state, _, table, row_of = fitted(K)
    cal = device_calibration(K)
    held_out = random_state(99, K, J, batches=1, B=96)
    for state in (fit_state, held_out) if E == 16 else (held_out,):
        got = cal.score(meter_with(state, K, J), ece_bins=E)
        want = cr.score(state, K, J, table, row_of, E)
        assert (want["probability"]["skipped"] > 0).any() and (want["oks"]["n"] > 0).any()
        check_score(got, want, row_of, K, E)


def test_score_single_keypoint_and_empty_state():
    K, J = 1, 1
    state = random_state(5, K, J, batches=1, B=200)
    cal, (_, table, row_of) = check_fit(state, K, J, 1)
    check_score(cal.score(meter_with(state, K, J), ece_bins=8), cr.score(state, K, J, table, row_of, 8), row_of, K, 8)
    empty = vr.empty_state(K, J)
    got = cal.score(meter_with(empty, K, J), ece_bins=8)
    check_score(got, cr.score(empty, K, J, table, row_of, 8), row_of, K, 8)
    assert (got["probability"]["n"] == 0).all() and np.isnan(got["probability"]["brier"]).all()


# ----------------------------------------------------------------------------------------------- end to end
def heads_batch(seed, B=8, K=3):
    rng = np.random.default_rng(seed)
    batch = vr.random_batch(rng, B, K)
    batch[4][:] = rng.random((B, K)) < 0.7
    batch[5][:] = 1                                     # all annotated: B K samples in the probability head
    return batch


def feed(meter, batch):
    meter.update_heads(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch])


def test_end_to_end_a_second_meter_sees_calibrated_heads():
    from probpose_pytorch_amd import HeadCalibration, ValidationMeter
    batch = heads_batch(1)
    first, second = ValidationMeter(None), ValidationMeter(None)
    feed(first, batch)
    cal = HeadCalibration.fit(first, min_count=1)
    aux = torch.from_numpy(np.stack(batch[:3])).cuda()
    out = cal(aux).cpu().numpy()
    feed(second, [out[0], out[1], out[2], *batch[3:]])
    before, after = first.compute(), second.compute()
    for head in ("probability", "visibility"):
        base = after[head]["base_rate"][-1]
        assert base == before[head]["base_rate"][-1] and after[head]["n_pos"][-1] + after[head]["n_neg"][-1] > 0
        bound = base * (2.0 ** -24 + U) * (1 + U) + 2.0 ** -31 + 2 * U
        err = abs(after[head]["mean_conf"][-1] - base)
        print(head, "mean_conf", after[head]["mean_conf"][-1], "base_rate", base, "error / bound", err / bound)
        assert err <= bound, head


@pytest.mark.parametrize("kind", ["ArgMaxProbMap", "ProbMap"])
def test_codec_applies_the_calibration(kind, tmp_path):
    import probpose_pytorch_amd as pp
    from probpose_pytorch_amd import HeadCalibration, ValidationMeter
    B, K, H, W = 8, 3, 16, 12
    batch = heads_batch(2, B, K)
    meter = ValidationMeter(None)
    feed(meter, batch)
    cal = HeadCalibration.fit(meter, min_count=1)
    rng = np.random.default_rng(4)
    pred = tuple(torch.from_numpy(a).cuda() for a in
                 (rng.random((B, K, H, W), dtype=np.float32), *[a.reshape(B, K, 1, 1) for a in batch[:4]]))
    probmap = getattr(pp, kind)((48, 64), (W, H), np.array([0.05] * K))
    plain = pp.Codec(probmap).decode_device(pred)
    calibrated = pp.Codec(probmap, calibration=cal).decode_device(pred)
    assert torch.equal(calibrated["aux"].view(torch.int32), cal.apply(plain["aux"]).view(torch.int32))
    assert not torch.equal(calibrated["aux"], plain["aux"])
    for name in ("kpts", "scores", "err"):
        assert calibrated[name].cpu().numpy().tobytes() == plain[name].cpu().numpy().tobytes(), name
    host = pp.Codec(probmap, calibration=cal).decode(pred)
    assert same_bits(host[1].reshape(B, K), calibrated["aux"][0].cpu().numpy())
    two = getattr(pp, kind)((48, 64), (W, H), np.array([0.05] * 2))
    with pytest.raises(ValueError, match="keypoints"):
        pp.Codec(two, calibration=cal).decode_device(tuple(t[:, :2].contiguous() for t in pred))
    cal.save(tmp_path / "cal.pt")
    loaded = HeadCalibration.load(tmp_path / "cal.pt", "cuda")
    assert loaded.table.is_cuda and loaded.K == K and loaded.min_count == 1
    assert torch.equal(loaded.table, cal.table) and torch.equal(loaded.blocks, cal.blocks)
    assert torch.equal(loaded.row_of, cal.row_of)
