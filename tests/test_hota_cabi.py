"""CPU tests of the HOTA boundary: the pp_trackeval_hota_* entries are declared, exported and bound, refuse every bad
host argument with their own name in pp_last_error() before anything is launched, and return 0 for what launches
nothing; ``PoseTrackEval(hota=...)`` validates its arguments without a GPU.  Made-up addresses stand in for the device
pointers: the host never dereferences them."""
import numpy as np
import pytest

from tests.test_trackeval_cabi import FRAMES, SEQ, _frame, _host, _ids_table, _offs

NAN = float("nan")
ENTRIES = ("pp_trackeval_hota_align", "pp_trackeval_hota_weights", "pp_trackeval_hota_match",
           "pp_trackeval_hota_assoc")
POINTERS = {"pp_trackeval_hota_align": ("offs", "seq", "oks", "gt_idx", "pred_idx", "pmc"),
            "pp_trackeval_hota_weights": ("offs", "seq", "oks", "gt_idx", "pred_idx", "pmc", "gt_present",
                                          "pred_present", "q"),
            "pp_trackeval_hota_match": ("offs", "seq", "alpha", "oks", "q", "gt_idx", "pred_idx", "mc", "held_row",
                                        "frame_tp", "frame_loc"),
            "pp_trackeval_hota_assoc": ("seq", "mc", "gt_present", "pred_present", "frame_tp", "frame_loc", "tp",
                                        "sums")}
DEV = {k: 0x10000 * (i + 1) for i, k in enumerate(sorted({p for v in POINTERS.values() for p in v}))}


def _call(lib, entry, n_seq=2, n_alpha=2, frames=FRAMES, offs=(), seq=SEQ, alpha=(0.5, 1.0), totals=None, n_gid=None,
          n_pid=None, c_total=None, n_frames=None, null=()):
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    o = _offs(frames) if isinstance(offs, tuple) and not offs else _host(offs, np.int64)
    s, t = _host(seq, np.int64), _host(alpha, np.float64)
    n_frames = len(frames) if n_frames is None else n_frames
    Dtot, Gtot, oks_total = totals or (sum(f[1] for f in frames), sum(f[0] for f in frames),
                                       sum(f[0] * f[1] for f in frames))
    n_gid = (int(s[1, -1]) if s is not None else 0) if n_gid is None else n_gid
    n_pid = (int(s[2, -1]) if s is not None else 0) if n_pid is None else n_pid
    c_total = (int(s[3, -1]) if s is not None else 0) if c_total is None else c_total
    ho, hs, ht = (None if a is None else a.ctypes.data for a in (o, s, t))
    if entry == "pp_trackeval_hota_align":
        return lib.pp_trackeval_hota_align(n_seq, n_frames, Dtot, Gtot, oks_total, c_total, ho, hs, p["offs"], p["seq"],
                                           p["oks"], p["gt_idx"], p["pred_idx"], p["pmc"], None)
    if entry == "pp_trackeval_hota_weights":
        return lib.pp_trackeval_hota_weights(n_seq, n_frames, Dtot, Gtot, oks_total, c_total, n_gid, n_pid, ho, hs,
                                             p["offs"], p["seq"], p["oks"], p["gt_idx"], p["pred_idx"], p["pmc"],
                                             p["gt_present"], p["pred_present"], p["q"], None)
    if entry == "pp_trackeval_hota_match":
        return lib.pp_trackeval_hota_match(n_seq, n_alpha, n_frames, Dtot, Gtot, oks_total, c_total, ho, hs, ht,
                                           p["offs"], p["seq"], p["alpha"], p["oks"], p["q"], p["gt_idx"],
                                           p["pred_idx"], p["mc"], p["held_row"], p["frame_tp"], p["frame_loc"], None)
    return lib.pp_trackeval_hota_assoc(n_seq, n_alpha, n_frames, c_total, n_gid, n_pid, hs, p["seq"], p["mc"],
                                       p["gt_present"], p["pred_present"], p["frame_tp"], p["frame_loc"], p["tp"],
                                       p["sums"], None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_refuses_bad_arguments_before_any_launch(built_lib, entry):
    L = built_lib
    long_seq = ((0, (1 << 20) + 1), (0, 1), (0, 1), (0, 1))
    long_frames = ((0, 0),) * ((1 << 20) + 1)
    cases = [(dict(n_seq=-1), b"n_seq=-1"), (dict(seq=None), b"null host sequence table"),
             (dict(seq=((0, 2, 3), (1, 2, 3), (0, 3, 4), (0, 6, 7))), b"do not start at 0"),
             (dict(seq=((0, 2, 3), (0, 2, 1), (0, 3, 4), (0, 6, 7))), b"not monotone at sequence 1"),
             (dict(seq=((0, 2, 1), (0, 2, 3), (0, 3, 4), (0, 6, 7))), b"frame offsets are not monotone at sequence 1"),
             (dict(seq=((0, 2, 3), (0, 2, 3), (0, 3, 4), (0, 5, 6))), b"c offsets of sequence 0 span 5"),
             (dict(n_seq=1, frames=FRAMES[:1], seq=_ids_table(1025, 1)), b"PP_TRACKEVAL_MAX_IDS = 1024"),
             (dict(n_seq=1, frames=FRAMES[:1], seq=_ids_table(1, 1025)), b"PP_TRACKEVAL_MAX_IDS = 1024"),
             (dict(c_total=8), b"c offsets end at 7"), (dict(c_total=-1), b"c_total=-1"),
             (dict(n_seq=1, frames=long_frames, seq=long_seq),
              b"sequence 0 has 1048577 frames, more than PP_TRACKEVAL_HOTA_MAX_FRAMES = 1048576"),
             *[(dict(null=(k,)), b"null argument") for k in POINTERS[entry]]]
    if entry != "pp_trackeval_hota_assoc":
        cases += [(dict(offs=None), b"null host offsets"), (dict(offs=_offs(FRAMES) + 1), b"offsets do not start at 0"),
                  (dict(offs=((0, 1, 0, 5), (0, 2, 2, 3), (0, 2, 2, 3))), b"not monotone at frame 1"),
                  (dict(offs=((0, 1, 4, 5), (0, 2, 2, 3), (0, 2, 3, 4))), b"OKS offsets of frame 1 span 1"),
                  (dict(totals=(5, 3, 4)), b"offsets end at"), (dict(n_frames=-1), b"n_frames=-1"),
                  (dict(frames=FRAMES[:2]), b"frame offsets end at 3, there are 2 frames"),
                  (dict(n_seq=1, frames=((257, 1),), seq=_ids_table(257, 1)), b"PP_TRACKEVAL_MAX_FRAME = 256"),
                  (dict(n_seq=1, frames=((1, 257),), seq=_ids_table(1, 257)), b"PP_TRACKEVAL_MAX_FRAME = 256")]
    else:
        cases += [(dict(n_frames=-1), b"n_frames=-1"), (dict(n_frames=2), b"frame offsets end at 3, there are 2 frames")]
    if entry in ("pp_trackeval_hota_weights", "pp_trackeval_hota_assoc"):
        cases += [(dict(n_gid=4), b"identity offsets end at 3"), (dict(n_pid=5), b"predicted identity offsets end at 4"),
                  (dict(n_gid=-1), b"n_gid=-1"), (dict(n_pid=-2), b"n_pid=-2")]
    if entry in ("pp_trackeval_hota_match", "pp_trackeval_hota_assoc"):
        cases += [(dict(n_alpha=0), b"n_alpha=0 is outside [1, 32]"), (dict(n_alpha=33), b"n_alpha=33 is outside")]
    if entry == "pp_trackeval_hota_match":
        cases += [(dict(alpha=None), b"null host alphas"), (dict(alpha=(0.5, 0.0)), b"alpha 1 = 0 is outside (0, 1]"),
                  (dict(alpha=(1.5, 0.5)), b"alpha 0"), (dict(alpha=(0.5, NAN)), b"alpha 1"),
                  (dict(alpha=(-0.5, 0.5)), b"alpha 0")]
    for kwargs, word in cases:
        rc = _call(L, entry, **kwargs)
        err = L.pp_last_error()
        assert rc != 0 and word in err and entry.encode() in err, (kwargs, err)
    # checked even when nothing would launch
    assert _call(L, entry, n_seq=0, frames=(), seq=((0,),) * 4, null=(POINTERS[entry][0],)) != 0
    assert b"null argument" in L.pp_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_what_launches_nothing_returns_zero(built_lib, entry):
    assert _call(built_lib, entry, n_seq=0, frames=(), seq=((0,),) * 4) == 0, built_lib.pp_last_error()
    if entry in ("pp_trackeval_hota_align", "pp_trackeval_hota_weights"):   # not one (ground truth, prediction) pair
        assert _call(built_lib, entry, n_seq=1, frames=((2, 0), (0, 3)), seq=((0, 2), (0, 2), (0, 3), (0, 6))) == 0
    if entry == "pp_trackeval_hota_match":                  # a sequence without a frame
        assert _call(built_lib, entry, n_seq=1, frames=(), seq=((0, 0), (0, 0), (0, 0), (0, 0))) == 0


def test_constants_exports_and_names(built_lib):
    from probpose_pytorch_amd import _lib
    assert set(ENTRIES) <= set(_lib.EXPORTS) and all(hasattr(built_lib, name) for name in ENTRIES)
    assert [n for n in _lib.EXPORTS if n.startswith("pp_trackeval_hota_")] == list(ENTRIES)     # four, no more
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    for name in ENTRIES:
        assert f"int {name}(" in header
    assert _lib.PP_TRACKEVAL_HOTA_MAX_ALPHAS == 32 and "#define PP_TRACKEVAL_HOTA_MAX_ALPHAS 32\n" in header
    assert _lib.PP_TRACKEVAL_HOTA_MAX_FRAMES == 2 ** 20 and "#define PP_TRACKEVAL_HOTA_MAX_FRAMES 1048576\n" in header


def test_the_evaluator_validates_hota_arguments_without_a_gpu():
    from probpose_pytorch_amd import PoseTrackEval
    from probpose_pytorch_amd import trackeval as TE
    sig = np.full(3, 0.05)
    for bad in ((), (0.0,), (0.5, 1.5), (NAN,), (-0.1,), tuple(np.linspace(0.01, 0.99, 33))):
        with pytest.raises(ValueError, match="hota_alphas"):
            PoseTrackEval(sig, hota=True, hota_alphas=bad)
    with pytest.raises(TypeError):
        PoseTrackEval(sig, (0.5,), True)                    # keyword only
    ev = PoseTrackEval(sig, hota=True)
    assert ev.hota and ev.hota_alphas.tolist() == [i / 20.0 for i in range(1, 20)]
    assert not PoseTrackEval(sig).hota
    assert PoseTrackEval(sig, hota=True, hota_alphas=np.linspace(0.01, 1.0, 32)).hota_alphas.size == 32
    ev.add_frame("a", **_frame(G=2, D=1, gt_ids=np.array([10, 7]), pred_ids=np.array([99])))
    ev.add_frame("a", **_frame(G=0, D=3, pred_ids=np.array([5, 99, 8])))
    ev.add_frame("b", **_frame(G=1, D=1, gt_ids=np.array([7]), pred_ids=np.array([5])))
    b = ev._tables()
    assert b["present"].tolist() == [1, 1, 1] and b["pred_present"].tolist() == [2, 1, 1, 1]
    args = TE._parser().parse_args(["g.json", "t.json", "--hota"])
    assert args.hota and not TE._parser().parse_args(["g.json", "t.json"]).hota


def test_the_host_arithmetic_of_the_curves():
    """hota_curves against the gauge's finish on made-up totals, a zero denominator included."""
    from probpose_pytorch_amd import trackeval as TE
    from tests import hota_reference as H
    rec = dict(TP=[4, 2, 0], FN=[1, 3, 5], FP=[0, 2, 4], loc_sum=[3.5, 1.9, 0.0], assa_sum=[2.5, 1.0, 0.0],
               assre_sum=[3.0, 1.5, 0.0], asspr_sum=[3.5, 1.25, 0.0])
    got, want = TE.hota_curves(rec, (0.3, 0.6, 0.9)), H.finish([rec], (0.3, 0.6, 0.9))
    assert got == want and tuple(got["curves"]) == TE.HOTA_KEYS == H.CURVES
    assert got["curves"]["LocA"][2] == 1.0 and got["curves"]["HOTA"][2] == 0.0 and got["curves"]["DetA"][0] == 0.8
