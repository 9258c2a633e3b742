"""Tests of the three stochastic-depth kernels (csrc/pp_droppath.hip), each on its own against float64.

Shapes (B, N, C): (3, 35, 64) and (4, 48, 128) take the 128-bit path; (2, 5, 36) takes it too when its buffers are
16-byte aligned (C % 4 == 0), so it also runs from buffers that start 4 bytes past an aligned address, which together
with (2, 5, 37) (C % 4 != 0) covers the scalar path.  idx cases: one crop, all crops, a strict subset that does not
start at crop 0.

Bounds, u = 2^-24, element by element against the float64 value of the same f32 inputs (scale as the f32 the kernel
takes):
* gather to f32: scale 1 is a copy (bit-equal); a scale is one f32 multiply, |d| <= u |want|.  To bf16: that product
  rounded once more, u |want| + 2^-9 (1 + u) |want| <= 2^-8 |want|.
* pp_droppath_add (the header states the fma form): one rounding of the exact r + scale branch, |d| <= u |want|;
  dropped crops' rows carry r's bits.
* scatter-add: one f32 add, |d| <= u |want|; dres_c rows = the new dres rounded to its dtype, bit-equal to
  ``dres.to(dtype)``; rows of crops outside idx keep their bits in both buffers.
The argument checks run before any launch and need no GPU.
"""
import pytest
import torch

from tests.head_grad_reference import U_BF16, U_F32

gpu = pytest.mark.gpu

SHAPES = [(3, 35, 64), (4, 48, 128), (2, 5, 36), (2, 5, 37)]
CASES = [(B, N, C, off) for B, N, C in SHAPES for off in ((0, 1) if C == 36 else (0,))]
IDX = ("one", "all", "subset")


@pytest.fixture
def ops(built_lib):
    from probpose_pytorch_amd import ops
    return ops


def _idx(kind, B):
    if kind == "one":
        return [0]
    if kind == "all":
        return list(range(B))
    return [1, 3] if B >= 4 else list(range(1, B))


def _buf(shape, dtype, off, fill=None, seed=0):
    """A contiguous device tensor that starts ``off`` elements past its allocation (off = 1: not 16-byte aligned)."""
    n = 1
    for s in shape:
        n *= s
    base = torch.empty(n + off, dtype=dtype, device="cuda")
    t = base[off:].view(shape)
    if fill is not None:
        t.copy_(fill)
    else:
        t.copy_(torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype))
    return t


def _tables(kind, B):
    idx = _idx(kind, B)
    slot = [-1] * B
    for j, b in enumerate(idx):
        slot[b] = j
    return idx, torch.tensor(idx, dtype=torch.int32).cuda(), torch.tensor(slot, dtype=torch.int32).cuda()


def _rel(got, want, u):
    """max |got - want| / (u |want|) over the elements (0 where both are 0)."""
    got, want = got.double().cpu(), want.double().cpu()
    return float(((got - want).abs() / (u * want.abs()).clamp_min(1e-300)).max())


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@gpu
@pytest.mark.parametrize("kind", IDX)
@pytest.mark.parametrize("B,N,C,off", CASES)
def test_gather(ops, B, N, C, off, kind):
    idx, idx_d, _ = _tables(kind, B)
    k = len(idx)
    src = _buf((B * N, C), torch.float32, off, seed=1)
    rows = src.reshape(B, N * C)[idx].reshape(k * N, C)
    out = _buf((k * N, C), torch.float32, off, seed=2)
    ops.crop_rows_gather(src, idx_d, B, N, C, out)
    assert torch.equal(_bits(out), _bits(rows))
    scale = 1.0 / (1.0 - 0.3)
    want = rows.double() * float(torch.tensor(scale, dtype=torch.float32))
    ops.crop_rows_gather(src, idx_d, B, N, C, out, scale)
    r32 = _rel(out, want, U_F32)
    o16 = _buf((k * N, C), torch.bfloat16, off, seed=3)
    ops.crop_rows_gather(src, idx_d, B, N, C, o16, scale)
    r16 = _rel(o16, want, U_BF16)
    print(f"d/bound gather {(B, N, C)} off {off} {kind}: f32 {r32:.3g}, bf16 {r16:.3g}")
    assert r32 <= 1.0 and r16 <= 1.0
    again, again16 = torch.empty_like(out), torch.empty_like(o16)
    ops.crop_rows_gather(src, idx_d, B, N, C, again, scale)
    ops.crop_rows_gather(src, idx_d, B, N, C, again16, scale)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(o16), _bits(again16))


@gpu
@pytest.mark.parametrize("kind", IDX)
@pytest.mark.parametrize("B,N,C,off", CASES)
def test_droppath_add(ops, B, N, C, off, kind):
    idx, _, slot_d = _tables(kind, B)
    k = len(idx)
    r = _buf((B * N, C), torch.float32, off, seed=4)
    r[:, 0] = -0.0                       # a bit pattern that an add of +0 would not preserve
    branch = _buf((k * N, C), torch.float32, off, seed=5)
    out = _buf((B * N, C), torch.float32, off, seed=6)
    scale = 1.0 / (1.0 - 0.4)
    ops.droppath_add(r, branch, slot_d, B, k, N, C, scale, out)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    rc, oc = r.reshape(B, N * C), out.reshape(B, N * C)
    dropped = [b for b in range(B) if b not in idx]
    assert torch.equal(_bits(oc[dropped]), _bits(rc[dropped]))
    want = rc[idx].double().cpu() + s32 * branch.reshape(k, N * C).double().cpu()
    ratio = _rel(oc[idx], want, U_F32)
    print(f"d/bound droppath_add {(B, N, C)} off {off} {kind}: {ratio:.3g}")
    assert ratio <= 1.0
    again = torch.empty_like(out)
    ops.droppath_add(r, branch, slot_d, B, k, N, C, scale, again)
    assert torch.equal(_bits(out), _bits(again))


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", IDX)
@pytest.mark.parametrize("B,N,C,off", CASES)
def test_scatter_add(ops, B, N, C, off, kind, dt):
    idx, idx_d, _ = _tables(kind, B)
    k = len(idx)
    dx = _buf((k * N, C), torch.float32, off, seed=7)
    d0 = _buf((B * N, C), torch.float32, off, seed=8)
    c0 = _buf((B * N, C), dt, off, seed=9)            # unrelated values: an untouched row is recognisable
    runs = []
    for _ in range(2):
        dres = _buf((B * N, C), torch.float32, off, fill=d0)
        dres_c = _buf((B * N, C), dt, off, fill=c0)
        ops.crop_rows_scatter_add(dx, idx_d, B, N, C, dres, dres_c)
        runs.append((dres, dres_c))
    dres, dres_c = runs[0]
    outside = [b for b in range(B) if b not in idx]
    crops = lambda t: t.reshape(B, N * C)  # noqa: E731
    assert torch.equal(_bits(crops(dres)[outside]), _bits(crops(d0)[outside]))
    assert torch.equal(_bits(crops(dres_c)[outside]), _bits(crops(c0)[outside]))
    want = crops(d0)[idx].double().cpu() + dx.reshape(k, N * C).double().cpu()
    ratio = _rel(crops(dres)[idx], want, U_F32)
    print(f"d/bound scatter_add {(B, N, C)} off {off} {kind} {dt}: {ratio:.3g}")
    assert ratio <= 1.0
    assert torch.equal(_bits(crops(dres_c)[idx]), _bits(crops(dres)[idx].to(dt)))
    assert torch.equal(_bits(dres), _bits(runs[1][0])) and torch.equal(_bits(dres_c), _bits(runs[1][1]))


def test_argument_validation_without_gpu(built_lib):
    """Null pointer, kept > B and N <= 0 are refused on the host, before any launch."""
    from probpose_pytorch_amd import _lib
    L = built_lib
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000         # never dereferenced: every call below fails its checks
    calls = {
        "pp_crop_rows_gather": lambda src, idx, B, k, N: L.pp_crop_rows_gather(src, idx, B, k, N, 64, 1.0, c,
                                                                               _lib.PP_F32, None),
        "pp_droppath_add": lambda r, br, B, k, N: L.pp_droppath_add(r, br, c, B, k, N, 64, 1.0, d, None),
        "pp_crop_rows_scatter_add": lambda dx, idx, B, k, N: L.pp_crop_rows_scatter_add(dx, idx, B, k, N, 64, c, d,
                                                                                        _lib.PP_BF16, None),
    }
    for name, call in calls.items():
        assert call(None, b, 4, 2, 48) != 0 and b"null" in L.pp_last_error(), name
        assert call(a, None, 4, 2, 48) != 0 and b"null" in L.pp_last_error(), name
        assert call(a, b, 4, 5, 48) != 0 and b"bad shape" in L.pp_last_error(), name
        assert call(a, b, 4, 0, 48) != 0 and b"bad shape" in L.pp_last_error(), name
        assert call(a, b, 4, 2, 0) != 0 and b"bad shape" in L.pp_last_error(), name
        assert call(a, b, 4, 2, -3) != 0 and b"bad shape" in L.pp_last_error(), name
    assert L.pp_droppath_add(a, b, c, 4, 2, 48, 64, 1.0, a, None) != 0 and b"alias" in L.pp_last_error()
    assert L.pp_crop_rows_gather(a, b, 4, 2, 48, 64, 1.0, c, 7, None) != 0 and b"dtype" in L.pp_last_error()
    with pytest.raises(_lib.HipExtensionError, match="pp_crop_rows_scatter_add"):
        _lib.check(L.pp_crop_rows_scatter_add(a, b, 4, 2, 48, 64, c, c, _lib.PP_F32, None), "pp_crop_rows_scatter_add")
