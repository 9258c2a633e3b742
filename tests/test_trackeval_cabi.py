"""CPU tests of PoseTrackEval's boundary: the pp_trackeval_* entries are declared, exported and bound, refuse bad
arguments on the host with their own name in pp_last_error() before anything is launched, and return 0 for what launches
nothing; ``PoseTrackEval`` validates without a GPU and raises ``HipExtensionError`` only where a device is really
needed; the command line's JSON reading, the rule for detections without a slot included.  Made-up addresses stand in
for the device pointers: the host never dereferences them."""
import json

import numpy as np
import pytest

DEV = dict(offs=0x10000, seq=0x20000, thr=0x30000, oks=0x40000, gt_idx=0x50000, pred_idx=0x60000, last=0x70000,
           prev=0x80000, matched=0x90000, runs=0xa0000, rec=0xb0000, oks_sum=0xc0000, c=0xd0000, idtp=0xe0000)
NAN = float("nan")
# two sequences: frames (G, D) = (2, 1), (0, 3) | (1, 1); identities (2, 3) | (1, 1)
FRAMES = ((2, 1), (0, 3), (1, 1))
SEQ = ((0, 2, 3), (0, 2, 3), (0, 3, 4), (0, 6, 7))


def _offs(frames):
    g, d = np.array([f[0] for f in frames], dtype=np.int64), np.array([f[1] for f in frames], dtype=np.int64)
    o = np.zeros((3, len(frames) + 1), dtype=np.int64)
    o[0, 1:], o[1, 1:], o[2, 1:] = np.cumsum(d), np.cumsum(g), np.cumsum(d * g)
    return o


def _host(x, dtype):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dtype))


def _call(lib, entry, n_seq=2, n_thr=2, frames=FRAMES, offs=(), seq=SEQ, thr=(0.5, 1.0), totals=None, n_gid=None,
          c_total=None, null=()):
    p = {k: (None if k in null else v) for k, v in DEV.items()}
    o = _offs(frames) if isinstance(offs, tuple) and not offs else _host(offs, np.int64)
    s, t = _host(seq, np.int64), _host(thr, np.float64)
    n_frames = len(frames)
    Dtot, Gtot, oks_total = totals or (sum(f[1] for f in frames), sum(f[0] for f in frames),
                                       sum(f[0] * f[1] for f in frames))
    n_gid = (int(s[1, -1]) if s is not None else 0) if n_gid is None else n_gid
    c_total = (int(s[3, -1]) if s is not None else 0) if c_total is None else c_total
    ho, hs, ht = (None if a is None else a.ctypes.data for a in (o, s, t))
    if entry == "pp_trackeval_clear":
        return lib.pp_trackeval_clear(n_seq, n_thr, n_frames, Dtot, Gtot, oks_total, n_gid, ho, hs, ht, p["offs"],
                                      p["seq"], p["thr"], p["oks"], p["gt_idx"], p["pred_idx"], p["last"], p["prev"],
                                      p["matched"], p["runs"], p["rec"], p["oks_sum"], None)
    if entry == "pp_trackeval_overlap":
        return lib.pp_trackeval_overlap(n_seq, n_thr, n_frames, Dtot, Gtot, oks_total, c_total, ho, hs, ht, p["offs"],
                                        p["seq"], p["thr"], p["oks"], p["gt_idx"], p["pred_idx"], p["c"], None)
    return lib.pp_trackeval_identity(n_seq, n_thr, c_total, hs, p["seq"], p["c"], p["idtp"], None)


ENTRIES = ("pp_trackeval_clear", "pp_trackeval_overlap", "pp_trackeval_identity")
POINTERS = {"pp_trackeval_clear": ("offs", "seq", "thr", "oks", "gt_idx", "pred_idx", "last", "prev", "matched", "runs",
                                   "rec", "oks_sum"),
            "pp_trackeval_overlap": ("offs", "seq", "thr", "oks", "gt_idx", "pred_idx", "c"),
            "pp_trackeval_identity": ("seq", "c", "idtp")}


def _ids_table(ng, npr):
    return ((0, 1), (0, ng), (0, npr), (0, ng * npr))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_refuses_bad_arguments_before_any_launch(built_lib, entry):
    L = built_lib
    cases = [(dict(n_seq=-1), b"n_seq=-1"), (dict(n_thr=0), b"n_thr=0"), (dict(seq=None), b"null host sequence table"),
             (dict(seq=((0, 2, 3), (1, 2, 3), (0, 3, 4), (0, 6, 7))), b"do not start at 0"),
             (dict(seq=((0, 2, 3), (0, 2, 1), (0, 3, 4), (0, 6, 7))), b"not monotone at sequence 1"),
             (dict(seq=((0, 2, 3), (0, 2, 3), (0, 3, 4), (0, 5, 6))), b"c offsets of sequence 0 span 5"),
             (dict(n_seq=1, frames=FRAMES[:1], seq=_ids_table(1025, 1)), b"PP_TRACKEVAL_MAX_IDS = 1024"),
             (dict(n_seq=1, frames=FRAMES[:1], seq=_ids_table(1, 1025)), b"PP_TRACKEVAL_MAX_IDS = 1024"),
             *[(dict(null=(k,)), b"null argument") for k in POINTERS[entry]]]
    if entry != "pp_trackeval_identity":
        cases += [(dict(thr=None), b"null host thresholds"), (dict(thr=(0.5, 0.0)), b"threshold 1 = 0 is outside (0, 1]"),
                  (dict(thr=(1.5, 0.5)), b"threshold 0"), (dict(thr=(0.5, NAN)), b"threshold 1"),
                  (dict(thr=(-0.5, 0.5)), b"threshold 0"),
                  (dict(offs=None), b"null host offsets"),
                  (dict(offs=_offs(FRAMES) + 1), b"offsets do not start at 0"),
                  (dict(offs=((0, 1, 0, 5), (0, 2, 2, 3), (0, 2, 2, 3))), b"not monotone at frame 1"),
                  (dict(offs=((0, 1, 4, 5), (0, 2, 2, 3), (0, 2, 3, 4))), b"OKS offsets of frame 1 span 1"),
                  (dict(totals=(5, 3, 4)), b"offsets end at"),
                  (dict(frames=FRAMES[:2]), b"frame offsets end at 3, there are 2 frames"),
                  (dict(n_seq=1, frames=((257, 1),), seq=_ids_table(257, 1)), b"PP_TRACKEVAL_MAX_FRAME = 256"),
                  (dict(n_seq=1, frames=((1, 257),), seq=_ids_table(1, 257)), b"PP_TRACKEVAL_MAX_FRAME = 256")]
    if entry == "pp_trackeval_clear":                        # the totals an entry is given are the ones it checks
        cases += [(dict(n_gid=4), b"identity offsets end at 3")]
    else:
        cases += [(dict(c_total=8), b"c offsets end at 7")]
    for kwargs, word in cases:
        rc = _call(L, entry, **kwargs)
        err = L.pp_last_error()
        assert rc != 0 and word in err and entry.encode() in err, (kwargs, err)
    # checked even when nothing would launch
    assert _call(L, entry, n_seq=0, frames=(), seq=((0,),) * 4, n_thr=0) != 0 and b"n_thr=0" in L.pp_last_error()


def test_the_oks_stage_refuses_no_keypoints(built_lib):
    """K < 1 is refused where K is an argument: by pp_cocoeval_oks, the first of the four launches."""
    o = _offs(FRAMES)
    rc = built_lib.pp_cocoeval_oks(3, 0, 5, 3, 3, o.ctypes.data, *[0x1000 * (i + 1) for i in range(8)], None)
    assert rc != 0 and b"pp_cocoeval_oks: K=0" in built_lib.pp_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_what_launches_nothing_returns_zero(built_lib, entry):
    assert _call(built_lib, entry, n_seq=0, frames=(), seq=((0,),) * 4) == 0, built_lib.pp_last_error()
    if entry == "pp_trackeval_overlap":                     # sequences, but not one (ground truth, prediction) pair
        assert _call(built_lib, entry, n_seq=1, frames=((2, 0), (0, 3)), seq=((0, 2), (0, 2), (0, 3), (0, 6))) == 0


def test_constants_exports_and_names():
    import probpose
    import probpose_pytorch_amd as pkg
    from probpose_pytorch_amd import _lib
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    header = open(_lib.LIB_PATH.replace("probpose_pytorch_amd/lib/libprobpose_hip.so", "include/probpose_hip.h")).read()
    for name in ENTRIES:
        assert f"int {name}(" in header
    assert _lib.PP_TRACKEVAL_MAX_FRAME == 256 and "#define PP_TRACKEVAL_MAX_FRAME 256\n" in header
    assert _lib.PP_TRACKEVAL_MAX_IDS == 1024 and "#define PP_TRACKEVAL_MAX_IDS 1024\n" in header
    assert "PoseTrackEval" in pkg.__all__ and pkg.PoseTrackEval.__module__ == "probpose_pytorch_amd.trackeval"
    assert probpose.trackeval.PoseTrackEval is pkg.PoseTrackEval


def _frame(G=2, D=2, K=3, gt_ids=None, pred_ids=None):
    return dict(gt_ids=np.arange(G) if gt_ids is None else gt_ids, gt_keypoints=np.ones((G, K, 3)),
                gt_bboxes=np.ones((G, 4)), gt_areas=np.ones(G), pred_ids=np.arange(D) if pred_ids is None else pred_ids,
                pred_keypoints=np.ones((D, K, 2)))


def test_the_evaluator_validates_without_a_gpu():
    import torch
    from probpose_pytorch_amd import PoseTrackEval, _lib
    for bad in ((), (0.0,), (0.5, 1.5), (NAN,), (-0.1,)):
        with pytest.raises(ValueError, match="thresholds"):
            PoseTrackEval(np.full(3, 0.05), thresholds=bad)
    with pytest.raises(ValueError, match="sigmas"):
        PoseTrackEval(np.zeros(3))
    ev = PoseTrackEval(np.full(3, 0.05), thresholds=(0.5, 1.0))
    for change, word in ((dict(gt_keypoints=np.ones((2, 4, 3))), r"gt_keypoints: expected \[2, 3, 3\]"),
                         (dict(gt_keypoints=np.ones((2, 3, 2))), "gt_keypoints: expected"),
                         (dict(gt_bboxes=np.ones((2, 3))), r"gt_bboxes: expected \[2, 4\]"),
                         (dict(gt_areas=np.ones((2, 1))), r"gt_areas: expected \[2\]"),
                         (dict(pred_keypoints=np.ones((2, 3, 4))), r"pred_keypoints: expected \[2, 3, 2\|3\]"),
                         (dict(pred_keypoints=np.ones((3, 3, 2))), "pred_keypoints: expected"),
                         (dict(gt_ids=np.zeros((2, 1), dtype=np.int64)), r"gt_ids: expected \[N\]"),
                         (dict(pred_ids=np.array([0.5, 1.5])), "pred_ids: expected integers"),
                         (dict(gt_keypoints=np.ones((2, 3, 3), dtype=np.int64)), "gt_keypoints: expected a float dtype"),
                         (dict(gt_bboxes=np.ones((2, 4), dtype=np.int32)), "gt_bboxes: expected a float dtype"),
                         (dict(gt_areas=np.ones(2, dtype=np.int64)), "gt_areas: expected a float dtype"),
                         (dict(pred_keypoints=np.ones((2, 3, 2), dtype=np.int64)), "pred_keypoints: expected a float"),
                         (dict(pred_keypoints=torch.ones((2, 3, 2), dtype=torch.int32)), "pred_keypoints: expected a f"),
                         (dict(gt_ids=np.array([4, 4])), "gt_ids: id 4 occurs twice in one frame"),
                         (dict(pred_ids=np.array([9, 9])), "pred_ids: id 9 occurs twice in one frame"),
                         (dict(gt_ids=np.array([4, -1])), "gt_ids: id -1 is negative"),
                         (dict(pred_ids=np.array([-3, 2])), "pred_ids: id -3 is negative"),
                         (dict(gt_areas=np.array([1.0, NAN])), "gt_areas: non-finite"),
                         (dict(pred_keypoints=np.full((2, 3, 2), np.inf)), "pred_keypoints: non-finite")):
        with pytest.raises(ValueError, match=word):
            ev.add_frame("a", **{**_frame(), **change})
    with pytest.raises(ValueError, match="gt_ids: a frame holds 257, more than PP_TRACKEVAL_MAX_FRAME = 256"):
        ev.add_frame("a", **_frame(G=257))
    with pytest.raises(ValueError, match="pred_ids: a frame holds 257, more than PP_TRACKEVAL_MAX_FRAME = 256"):
        ev.add_frame("a", **_frame(D=257))
    assert ev._seqs == {}                                    # a refused frame leaves nothing behind
    ev.add_frame("a", **_frame(G=256, D=256))
    ev.add_frame("a", **_frame(G=0, D=0))
    ev.add_frame(("cam", 2), **_frame(pred_ids=np.array([2 ** 62, 5])))
    ev.add_frame("b", gt_ids=[3], gt_keypoints=torch.ones((1, 3, 3)), gt_bboxes=torch.ones((1, 4)),
                 gt_areas=torch.ones(1), pred_ids=torch.tensor([7, 8]), pred_keypoints=torch.ones((2, 3, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipExtensionError):          # a well-formed call: the device is really needed now
            ev.evaluate()
    ev.reset()
    assert ev._seqs == {}
    for f in range(5):                                       # 1025 identities, 205 a frame
        ev.add_frame("long", **_frame(G=1, D=205, pred_ids=np.arange(205) + 205 * f))
    with pytest.raises(ValueError, match="sequence 'long' has 1025 predicted identities, more than "
                                         "PP_TRACKEVAL_MAX_IDS = 1024"):
        ev.evaluate()
    ev.reset()
    for f in range(5):
        ev.add_frame(0, **_frame(G=205, D=1, gt_ids=np.arange(205) + 205 * f))
    with pytest.raises(ValueError, match="1025 ground-truth identities"):
        ev.evaluate()


def test_the_tables_of_a_batch():
    """The host arithmetic: ids become dense indices per sequence in order of first appearance; the offset tables are
    what the entries check."""
    from probpose_pytorch_amd import PoseTrackEval
    ev = PoseTrackEval(np.full(3, 0.05))
    ev.add_frame("a", **_frame(G=2, D=1, gt_ids=np.array([10 ** 15, 7]), pred_ids=np.array([99])))
    ev.add_frame("a", **_frame(G=0, D=3, pred_ids=np.array([5, 99, 2 ** 62])))
    ev.add_frame("b", **_frame(G=1, D=1, gt_ids=np.array([7]), pred_ids=np.array([5])))
    ev.add_frame("a", **_frame(G=2, D=0, gt_ids=np.array([7, 3])))
    b = ev._tables()
    assert b["names"] == ["a", "b"]
    assert b["offs"].tolist() == [[0, 1, 4, 4, 5], [0, 2, 2, 4, 5], [0, 2, 2, 2, 3]]
    assert b["table"].tolist() == [[0, 3, 4], [0, 3, 4], [0, 3, 4], [0, 9, 10]]
    assert b["gt_idx"].tolist() == [0, 1, 1, 2, 0] and b["gt_idx"].dtype == np.int32
    assert b["pred_idx"].tolist() == [0, 1, 0, 2, 0] and b["pred_idx"].dtype == np.int32
    assert b["present"].tolist() == [1, 2, 1, 1] and b["n_gt"].tolist() == [4, 1] and b["n_pred"].tolist() == [4, 1]


def test_the_command_line_reads_its_files(tmp_path):
    from probpose_pytorch_amd import trackeval as TE
    kp3 = [[1.0, 2.0, 2.0], [3.0, 4.0, 0.0]]
    gt = [dict(frame="f0.png", persons=[dict(id=4, keypoints=kp3, bbox=[0, 0, 2, 3], area=5.0)]),
          dict(frame="f1.png", persons=[]),
          dict(frame="f2.png", persons=[dict(id=4, keypoints=kp3, bbox=[0, 0, 2, 3]),
                                        dict(id=9, keypoints=kp3, bbox=[1, 1, 1, 1], area=2.0)])]
    kp2 = [[1.0, 2.0], [3.0, 4.0]]
    tracks = [dict(frame="f2.png", detections=[dict(id=-1, keypoints=kp2), dict(id=6, keypoints=kp2),
                                               dict(id=-1, keypoints=kp2)]),
              dict(frame="f0.png", detections=[dict(id=0, keypoints=kp2)]),
              dict(frame="zz.png", detections=[dict(id=3, keypoints=kp2)])]
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))
    frames, K, slotless = TE.load_json_frames(tmp_path / "gt.json", tmp_path / "tracks.json")
    assert (K, slotless, len(frames)) == (2, 2, 3)
    assert [f[0].tolist() for f in frames] == [[4], [], [4, 9]]
    # GT.json's order; a frame absent from TRACKS.json has no predictions; a negative id becomes a fresh one above
    # every id of the file, each its own
    assert [f[4].tolist() for f in frames] == [[0], [], [7, 6, 8]]
    assert frames[0][1].shape == (1, 2, 3) and frames[1][1].shape == (0, 2, 3) and frames[1][5].shape == (0, 2, 2)
    assert frames[0][3].tolist() == [5.0] and frames[2][3].tolist() == [6.0, 2.0]     # area defaults to the box's
    ev = TE.PoseTrackEval(TE._cli_sigmas("0.05", K), thresholds=(0.5,))
    for fr in frames:
        ev.add_frame("clip", *fr)                           # what main() does before it needs the device
    assert ev._tables()["table"].tolist() == [[0, 3], [0, 2], [0, 4], [0, 8]]
    assert TE._cli_sigmas("coco17", 17).shape == (17,) and TE._cli_sigmas("0.1,0.2", 2).tolist() == [0.1, 0.2]
    for spec, k in (("coco17", 3), ("0.1,0.2", 3), ("abc", 2)):
        with pytest.raises(ValueError, match="--sigmas"):
            TE._cli_sigmas(spec, k)
    with pytest.raises(ValueError, match="occurs twice"):
        TE.load_json_frames(gt, tracks + tracks[:1])
    args = TE._parser().parse_args(["g.json", "t.json", "--thr", "0.5,0.75", "--seq", "clip7"])
    assert (args.thr, args.sigmas, args.seq) == ("0.5,0.75", "coco17", "clip7")
