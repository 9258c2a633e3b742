"""Flip test on the GPU against tests/flip_reference.py: ``pp_hflip_pair`` and ``pp_flip_merge`` bit for bit (both
instances of each, guard words around every output), both auxiliary layouts, the model-level forward in fp32 and bf16
against the merge of the plain model's outputs on the concatenated batch (bit for bit) and, in fp32, against the float64
merge of the CPU oracle (1e-4, the bound tests/test_model_train_gpu.py holds eval outputs to), equivariance, no host
synchronisation, graph capture and a generic head."""
import numpy as np
import pytest
import torch

from tests import flip_reference as FR

pytestmark = pytest.mark.gpu

GUARD = 4096                         # floats on either side of an output that must keep their bits (16-byte multiples)
SENTINEL = 0xA5A5A5A5                # as a float32 bit pattern: no kernel result below is this value
PAIRS20 = [(2 * i + 1, 2 * i + 2) for i in range(8)]
PAIRS133 = PAIRS20 + [(17 + i, 132 - i) for i in range(30)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(count):
    buf = torch.full((count + 2 * GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[GUARD:GUARD + count]


def _guards_intact(buf, count):
    got = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    return (got[:GUARD] == SENTINEL).all() and (got[GUARD + count:] == SENTINEL).all()


# ---- pp_hflip_pair ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 5, 4), (3, 3, 7, 8), (2, 1, 4, 6), (2, 3, 3, 13), (2, 3, 32, 48)])
def test_hflip_pair_bits(built_lib, shape):
    """(1,3,5,4): one self-mirrored group a row; W = 6, 13: the one-pixel instance; inputs hold -0.0, a denormal, the
    infinities and NaNs with payloads, compared as bit patterns."""
    from probpose_pytorch_amd import ops
    x = FR.special_floats(shape, seed=sum(shape))
    want = FR.pair(x)
    count = 2 * x.size
    buf, out = _guarded(count)
    out = out.view(2 * shape[0], *shape[1:])
    d_x = torch.from_numpy(x).cuda()
    ops.hflip_pair(d_x, out)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert _guards_intact(buf, count)
    assert np.array_equal(_bits(d_x.cpu().numpy()), _bits(x))                  # the input is left alone
    if shape[-1] % 4 == 0:                                                    # a misaligned output: the one-pixel instance
        buf, out = _guarded(count + 1)
        out = out[1:].view(2 * shape[0], *shape[1:])
        ops.hflip_pair(d_x, out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        assert _guards_intact(buf, count + 1) and _bits(buf[GUARD:GUARD + 1].cpu().numpy())[0] == SENTINEL


# ---- pp_flip_merge ---------------------------------------------------------------------------------------------------------------
MERGE_CASES = [
    ((1, 1, 1, 4), []),
    ((1, 3, 2, 6), [(0, 2)]),                       # the one-pixel instance; keypoint 1 is a fixed point
    ((3, 17, 8, 12), [(i, i + 1) for i in range(1, 17, 2)]),
    ((2, 20, 96, 96), PAIRS20),
    ((2, 133, 16, 12), PAIRS133),                   # 4 B K = 1064: five auxiliary workgroups, the last one partly filled
    ((4, 16, 2, 4), [(0, 15), (3, 4)]),             # 4 B K = 256: exactly one auxiliary workgroup
]


def _merge_inputs(shape, seed):
    B, K, H, W = shape
    rng = np.random.default_rng(seed)
    heat2 = rng.random((2 * B, K, H, W), dtype=np.float32)
    heat2[rng.random(heat2.shape) < 0.3] = 0.0                       # clamped maps hold exact zeros
    aux2 = (rng.random((4, 2 * B, K), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    return heat2, aux2


@pytest.mark.parametrize("shape,pairs", MERGE_CASES, ids=[str(c[0]) for c in MERGE_CASES])
def test_flip_merge_bits(built_lib, shape, pairs):
    from probpose_pytorch_amd import flip, ops
    B, K, H, W = shape
    perm = flip.flip_permutation(pairs, K)
    assert np.array_equal(perm, FR.permutation(pairs, K))
    heat2, aux2 = _merge_inputs(shape, seed=K + W)
    want = FR.merge((heat2,) + tuple(a.reshape(2 * B, K, 1, 1) for a in aux2), perm)
    d_heat2, d_aux2, d_perm = torch.from_numpy(heat2).cuda(), torch.from_numpy(aux2).cuda(), torch.from_numpy(perm).cuda()
    n_heat, n_aux = B * K * H * W, 4 * B * K
    runs = []
    for _ in range(2):
        hbuf, heat = _guarded(n_heat)
        abuf, aux = _guarded(n_aux)
        ops.flip_merge(d_heat2, d_aux2, d_perm, heat.view(B, K, H, W), aux.view(4, B, K))
        got_h, got_a = heat.cpu().numpy().reshape(B, K, H, W), aux.cpu().numpy().reshape(4, B, K)
        assert np.array_equal(_bits(got_h), _bits(want[0]))
        for j in range(4):
            assert np.array_equal(_bits(got_a[j]), _bits(want[1 + j].reshape(B, K))), j
        assert _guards_intact(hbuf, n_heat) and _guards_intact(abuf, n_aux)
        runs.append((got_h.tobytes(), got_a.tobytes()))
    assert runs[0] == runs[1]
    assert np.array_equal(_bits(d_heat2.cpu().numpy()), _bits(heat2))          # the inputs are left alone
    # the planted faults differ from what the kernel gives (where the shape can show them)
    if pairs and W > 1:
        for fault in ("mirror_no_swap", "swap_no_mirror", "no_half", "off_by_one"):
            assert not np.array_equal(FR.merge((heat2,) + tuple(a.reshape(2 * B, K, 1, 1) for a in aux2), perm,
                                               fault=fault)[0], got_h), fault


@pytest.mark.parametrize("shape,pairs", MERGE_CASES[1:4], ids=[str(c[0]) for c in MERGE_CASES[1:4]])
def test_flip_merge_both_aux_layouts(built_lib, shape, pairs):
    """flip.flip_merge on the head's own layout (four views of one [4,2B,K] buffer: taken as it is) and on four
    separate tensors (packed by one copy): the same bits, shapes and dtypes as the head's."""
    from probpose_pytorch_amd import flip
    B, K, H, W = shape
    perm = FR.permutation(pairs, K)
    heat2, aux2 = _merge_inputs(shape, seed=3 * K + W)
    want = FR.merge((heat2,) + tuple(a.reshape(2 * B, K, 1, 1) for a in aux2), perm)
    d_perm = torch.from_numpy(perm.astype(np.int32)).cuda()
    d_heat2, d_aux2 = torch.from_numpy(heat2).cuda(), torch.from_numpy(aux2).cuda()
    views = tuple(d_aux2[j].reshape(2 * B, K, 1, 1) for j in range(4))
    separate = tuple(v.clone() for v in views)
    assert flip._packed_aux(views, 2 * B, K).data_ptr() == d_aux2.data_ptr()          # no copy
    assert flip._packed_aux(separate, 2 * B, K).data_ptr() not in [s.data_ptr() for s in separate]
    for aux in (views, separate, separate[:2] + views[2:]):             # mixed: packed like the separate ones
        got = flip.flip_merge((d_heat2,) + tuple(aux), d_perm)
        assert [tuple(g.shape) for g in got] == [(B, K, H, W)] + [(B, K, 1, 1)] * 4
        assert all(g.dtype == torch.float32 and g.is_contiguous() for g in got)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(w))


def test_flip_merge_python_refusals(built_lib):
    from probpose_pytorch_amd import _lib, flip
    B, K, H, W = 1, 3, 2, 8
    heat2, aux2 = (torch.from_numpy(a).cuda() for a in _merge_inputs((B, K, H, W), 0))
    aux = tuple(aux2[j].reshape(2 * B, K, 1, 1) for j in range(4))
    perm = torch.arange(K, dtype=torch.int32, device="cuda")
    flip.flip_merge((heat2,) + aux, perm)
    with pytest.raises(_lib.HipExtensionError):
        flip.flip_merge((heat2.double(),) + aux, perm)
    with pytest.raises(_lib.HipExtensionError):
        flip.flip_merge((heat2.bfloat16(),) + aux, perm)
    with pytest.raises(_lib.HipExtensionError):
        flip.flip_merge((heat2.cpu(),) + aux, perm)
    with pytest.raises(ValueError):
        flip.flip_merge((heat2.transpose(2, 3),) + aux, perm)                     # not contiguous
    with pytest.raises(ValueError):
        flip.flip_merge((heat2[:, :, :, ::2],) + aux, perm)
    with pytest.raises(ValueError):
        flip.flip_merge((heat2[:1],) + aux, perm)                                # an odd batch
    with pytest.raises(ValueError):
        flip.flip_merge((heat2,) + aux, perm.long())
    with pytest.raises(ValueError):
        flip.flip_merge((heat2,) + aux, perm.cpu())
    with pytest.raises(ValueError):
        flip.flip_merge((heat2,) + aux[:3] + (aux[3].reshape(2 * B, K),), perm)
    with pytest.raises(_lib.HipExtensionError):
        flip.flip_merge((heat2,) + aux[:3] + (aux[3].double(),), perm)


# ---- model level -----------------------------------------------------------------------------------------------------------------
B, K, C, HEADS, DEPTH, SIZE, POOLS = 3, 20, 384, 12, 2, (96, 96), [(3, 3), (2, 2)]


@pytest.fixture(scope="module")
def setup(built_lib):
    """The model (flip test off), its CPU state, the crops, and the plain fp32 outputs on [x, mirrored x]."""
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_head_state, synthetic_vit_state
    backbone = ScratchViTBackbone(SIZE, 16, embed_dim=C, depth=DEPTH, num_heads=HEADS)
    backbone.model.load_state_dict(synthetic_vit_state(SIZE, 16, C, DEPTH, seed=12))
    head = ProbMapHead(C, K, POOLS, (256, 256), (4, 4), final_layer_kernel_size=1)
    head.load_state_dict(synthetic_head_state(C, K, n_pools=len(POOLS), deconv_out=(256, 256), seed=13), strict=False)
    model = ProbPoseModel(backbone, head).cuda().eval()
    x = synthetic_crops(B, *SIZE, seed=14)
    x2 = torch.cat([x, x.flip(-1)])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return dict(model=model, sd=sd, x=x, x2=x2, xc=x.cuda(), x2c=x2.cuda(), perm=FR.permutation(PAIRS20, K))


def _np(outs):
    return tuple(o.detach().cpu().numpy() for o in outs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_model_flip_test_is_the_merge_of_the_plain_outputs(setup, dtype):
    from oracle import probpose_oracle as orc
    model, perm = setup["model"], setup["perm"]
    model.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            model.set_flip_test(None)
            plain2 = model(setup["x2c"])                              # the same batch through the same plans
            plain1 = model(setup["xc"])
            assert model.set_flip_test(PAIRS20) is model
            assert model._flip_perm.is_cuda and model._flip_perm.dtype == torch.int32
            got = model(setup["xc"])
            again = model(setup["xc"])
            want = FR.merge(_np(plain2), perm)
            assert [tuple(g.shape) for g in got] == [tuple(p.shape) for p in plain1]
            assert [g.dtype for g in got] == [p.dtype for p in plain1]
            assert all(g.is_contiguous() for g in got)
            for name, g, a, w in zip(("heatmaps", "prob", "vis", "oks", "err"), _np(got), _np(again), want):
                assert np.array_equal(_bits(g), _bits(w)), name
                assert np.array_equal(_bits(g), _bits(a)), name
            assert float(got[0].max()) > 0 and not np.array_equal(_np(got)[0], _np(plain1)[0])
            assert list(model.state_dict()) == list(setup["sd"])
            if dtype == torch.float32:
                ref2 = orc.model_forward(setup["sd"], setup["x2"], patch=16, heads=HEADS, pools=POOLS)
                ref = FR.merge(tuple(r.numpy() for r in ref2), perm, dtype=np.float64)
                for name, g, r in zip(("heatmaps", "prob", "vis", "oks", "err"), _np(got), ref):
                    d = float(np.abs(g.astype(np.float64) - r).max())
                    print(f"flip test fp32 vs the float64 merge of the CPU oracle, {name}: {d:.3g}")
                    assert d <= 1e-4, (name, d)
            # .train() runs the plain forward; a non-differentiable head refuses train mode itself, so only the
            # switch back is exercised: set_flip_test(None) gives the plain outputs bit for bit
            model.set_flip_test(None)
            back = model(setup["xc"])
            for g, p in zip(_np(back), _np(plain1)):
                assert np.array_equal(_bits(g), _bits(p))
            # a module saved before flip test existed has no such buffer: the forward reads it with a default
            del model._buffers["_flip_perm"]
            model._non_persistent_buffers_set.discard("_flip_perm")
            for g, p in zip(_np(model(setup["xc"])), _np(plain1)):
                assert np.array_equal(_bits(g), _bits(p))
    finally:
        model.set_flip_test(None)
        model.set_compute_dtype(torch.float32)


def test_model_flip_test_is_equivariant(setup):
    """Flip-test outputs for the mirrored crops are the mirrored-and-swapped flip-test outputs for the crops, exactly:
    the two passes trade places, the add commutes, and a crop's outputs do not depend on its batch slot."""
    model, perm = setup["model"], setup["perm"]
    model.set_compute_dtype(torch.float32)
    model.set_flip_test(PAIRS20)
    try:
        with torch.no_grad():
            a = _np(model(setup["xc"]))
            b = _np(model(setup["xc"].flip(-1).contiguous()))
    finally:
        model.set_flip_test(None)
    want = FR.unflip(a, perm)
    for name, g, w in zip(("heatmaps", "prob", "vis", "oks", "err"), b, want):
        d = float(np.abs(g.astype(np.float64) - w).max())
        print(f"equivariance, {name}: max difference {d:.3g}")
        assert np.array_equal(_bits(g), _bits(w)), (name, d)


def test_flip_forward_and_decode_make_no_host_sync(setup):
    from probpose_pytorch_amd.codec import Codec, ProbMap
    model = setup["model"]
    model.set_compute_dtype(torch.float32)
    model.set_flip_test(PAIRS20)
    codec = Codec(ProbMap(SIZE, (24, 24), np.full(K, 0.05)))
    try:
        with torch.no_grad():
            want = codec.decode(model(setup["xc"]))                        # the warm-up call: plans, tables, workspaces
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = model(setup["xc"])
                dec = codec.decode_device(out)       # decode up to its device-to-host copies, its documented sync points
            finally:
                torch.cuda.set_sync_debug_mode("default")
    finally:
        model.set_flip_test(None)
    assert np.array_equal(dec["kpts"].cpu().numpy(), want[0][0])
    assert np.array_equal(dec["scores"].cpu().numpy(), want[0][1])
    assert np.array_equal(dec["aux"].cpu().numpy()[0].reshape(B, 1, K), want[1])


def test_flip_forward_is_capturable(built_lib):
    """The tiny model of the graph test in tests/test_model_gpu.py with flip test on: captured, replayed, equal to eager."""
    from probpose_pytorch_amd.backbone import ScratchViTBackbone
    from probpose_pytorch_amd.flip import COCO17_FLIP_PAIRS
    from probpose_pytorch_amd.head import ProbMapHead
    from probpose_pytorch_amd.model import ProbPoseModel
    from probpose_pytorch_amd.synthetic import synthetic_crops, synthetic_model_state
    m = ProbPoseModel(ScratchViTBackbone((64, 48), 16, embed_dim=128, depth=2, num_heads=2),
                      ProbMapHead(128, 17, [(4, 3)], (64, 64), (4, 4), final_layer_kernel_size=1),
                      flip_pairs=COCO17_FLIP_PAIRS)
    m.load_state_dict(synthetic_model_state((64, 48), 16, 128, 2, 17, 1, (64, 64), seed=0))
    m = m.cuda().eval()
    assert m._flip_perm.is_cuda                                           # the buffer followed .cuda()
    x = synthetic_crops(4, 64, 48, seed=5).cuda()
    with torch.no_grad():
        want = [o.clone() for o in m(x)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out_g = m(x)
        for o in out_g:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
    for o, w in zip(out_g, want):
        assert torch.equal(o, w)
    perm = FR.permutation(COCO17_FLIP_PAIRS, 17)
    m.set_flip_test(None)
    with torch.no_grad():
        plain2 = m(torch.cat([x, x.flip(-1)]))
    for w, r in zip(want, FR.merge(_np(plain2), perm)):
        assert np.array_equal(_bits(w.cpu().numpy()), _bits(r))


class _StandInHead(torch.nn.Module):
    """Any other head: five separate contiguous tensors, computed in eager torch."""
    num_keypoints = 5

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.linspace(0.5, 1.5, 5))

    def forward(self, feats):
        heat = (feats.mean(1, keepdim=True) * self.scale[None, :, None, None]).contiguous()
        pooled = heat.amax((2, 3), keepdim=True)
        return heat, pooled * 0.5, pooled * 0.25 + 0.1, 1.0 - pooled, pooled * 3.0


def test_generic_head_path(built_lib):
    from probpose_pytorch_amd.model import ProbPoseModel
    pairs = [(0, 4), (1, 2)]
    model = ProbPoseModel(torch.nn.Identity(), _StandInHead(), flip_pairs=pairs).cuda().eval()
    plain = ProbPoseModel(torch.nn.Identity(), model.head).eval()
    x = torch.from_numpy(np.random.default_rng(5).random((3, 3, 8, 12), dtype=np.float32)).cuda()
    with torch.no_grad():
        got = model(x)
        want = FR.merge(_np(plain(torch.cat([x, x.flip(-1)]))), FR.permutation(pairs, 5))
        assert not np.array_equal(_np(got)[0], _np(plain(x))[0])
    assert [tuple(g.shape) for g in got] == [(3, 5, 8, 12)] + [(3, 5, 1, 1)] * 4
    for g, w in zip(_np(got), want):
        assert np.array_equal(_bits(g), _bits(w))
    with pytest.raises(ValueError):
        model.set_flip_test([(0, 5)])                                    # checked against the head's num_keypoints
