"""The pp_gemm calls that only a training step makes, built from what head_train.py and vit_train.py build them from
(the head's dimension keywords are head_calls' descriptors, the product's own), each with its ground truth from torch
autograd in float64 on the layer itself: the independent side.

A builder takes layer parameters, an output gradient (or, for the train-mode forward, an input) and the operand dtype,
and returns a ``Call``: ``kw`` holds the keyword arguments of ``ops.gemm`` with A, W and out among them (what
tests/gemm_reference.py restates and what a GPU test launches), ``truth`` the float64 result shaped like ``out``.
Weights and tables come from the product's own packers (pack.conv3x3_data_grad_weights, pack.deconv_data_grad_weights,
pack.deconv_data_grad_table, head_train._aux0_dgrad_table, vit_train._wt, ops.linear) and the descriptors from
head_calls, all looked up through their modules at call time, so that ``planted(fault)`` can swap one of them for a
wrong one: FAULTS lists those, each with the call
kinds whose comparison with the truth it must fail.  The truth is computed from the operands as the kernel reads them
(rounded to the operand dtype first), so on integer data it is exact and the restatement must equal it bit for bit.

An in-place residual call (the second aux-0 form) has ``kw["residual"] is kw["out"]``, and ``out`` holds the prior
values.  CASES are the shapes of tests/test_dgrad_reference.py and tests/test_dgrad_gemm_gpu.py; ``make`` draws the
data of one: integers in [-3, 3] (every sum exact in f32), or randn gradients with randn * Kd^-1/2 weights."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from probpose_pytorch_amd import head_calls, head_train, ops, pack, vit_train
from tests import gemm_reference as gr

EPI_OUT_F32 = gr.EPI_OUT_F32
f32, f64 = torch.float32, torch.float64


@dataclass
class Call:
    kind: str
    kw: dict
    truth: torch.Tensor

    @property
    def in_place(self) -> bool:
        return self.kw.get("residual") is self.kw["out"]


def rows(t: torch.Tensor) -> torch.Tensor:
    """(B, C, h, w) -> channels-last rows [B*h*w, C]."""
    B, C, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * h * w, C).contiguous()


def _input_grad(layer, shape, dy: torch.Tensor) -> torch.Tensor:
    """autograd's float64 gradient of layer(x) with respect to x (of ``shape``) under the output gradient dy."""
    x = torch.zeros(shape, dtype=f64, requires_grad=True)
    (g,) = torch.autograd.grad(layer(x), (x,), dy.double())
    return g


# ---------------------------------------------------------------------------------------------------------------
# head_train.py
# ---------------------------------------------------------------------------------------------------------------
def final_dgrad(weight, dz, dt) -> Call:
    """The final 1x1 layer's data gradient.  weight: final_layer.weight (K, cin, 1, 1); dz [M, KPAD]: the heatmap
    gradient at head_train's channel pitch (columns from K on meet the weight's zero padding: any finite value)."""
    K, cin = weight.shape[:2]
    KPAD = head_calls.kpad(K)
    M = dz.shape[0]
    assert dz.shape[1] == KPAD
    fw = weight.detach().reshape(K, cin).to(dt).contiguous()
    wt = torch.zeros((cin, KPAD), dtype=dt)
    wt[:, :K] = fw.t()
    A = dz.to(dt).contiguous()
    kw = dict(head_calls.final_dgrad(M, cin, K), A=A, W=wt, out=torch.empty((M, cin), dtype=f32), epilogue=EPI_OUT_F32)
    return Call("final", kw, _input_grad(lambda x: F.linear(x, fw.double()), (M, cin), A[:, :K]))


def deconv_dgrad(weight, dY, dt) -> Call:
    """A 4x4 stride-2 deconvolution's data gradient.  weight (cin, cout, 4, 4); dY (B, cout, 2h, 2w)."""
    cin, cout = weight.shape[:2]
    B, _, H, W = dY.shape
    h, w = H // 2, W // 2
    M = B * h * w
    tab = pack.deconv_data_grad_table(B, h, w, 4, cout)
    wt = pack.deconv_data_grad_weights(weight.detach()).to(dt).contiguous()
    A = rows(dY).to(dt)
    kw = dict(head_calls.deconv_dgrad(M, cin, cout), A=A, W=wt, out=torch.empty((M, cin), dtype=f32), rowoff=tab,
              epilogue=EPI_OUT_F32)
    w64 = weight.detach().to(dt).double()
    g = _input_grad(lambda x: F.conv_transpose2d(x, w64, stride=2, padding=1), (B, cin, h, w), dY.to(dt))
    return Call("deconv", kw, rows(g))


def _conv_input_grad(weight, dy, dt):
    w64 = weight.detach().to(dt).double()
    B, _, h, w = dy.shape
    return _input_grad(lambda x: F.conv2d(x, w64, padding=1), (B, weight.shape[1], h, w), dy.to(dt))


def aux_stage_dgrad(weights, dY, dt) -> Call:
    """A later aux stage's data gradient: the four branches' 3x3 convolutions as batch = 4 over column slabs of one
    [M, 4C] buffer.  weights: four (C, C, 3, 3); dY (B, 4C, h, w)."""
    C = weights[0].shape[0]
    B, _, h, w = dY.shape
    M = B * h * w
    ro = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * C)
    wt = torch.stack([pack.conv3x3_data_grad_weights(wb.detach()) for wb in weights]).to(dt).contiguous()
    A = rows(dY).to(dt)
    kw = dict(head_calls.aux_stage(M, C), A=A, W=wt, out=torch.empty((M, 4 * C), dtype=f32), rowoff=ro,
              epilogue=EPI_OUT_F32)
    g = torch.cat([_conv_input_grad(wb, dY[:, b * C:(b + 1) * C], dt) for b, wb in enumerate(weights)], dim=1)
    return Call("aux_stage", kw, rows(g))


def aux0_dgrad(weights, dY, brs, dt, prior=None) -> Call:
    """The first aux stage's data gradient into the tokens: the branches ``brs`` in one GEMM, written plainly or
    (prior [M, C] f32 given: the heatmap branch's token gradient) added to the buffer in place."""
    C = weights[0].shape[0]
    B, _, h, w = dY.shape
    M = B * h * w
    brs = list(brs)
    tab = head_train._aux0_dgrad_table(B, h, w, C, brs, "cpu")
    wt = torch.stack([pack.conv3x3_data_grad_weights(weights[bi].detach()).view(C, 9, C) for bi in brs],
                     dim=2).reshape(C, 9 * len(brs) * C).to(dt).contiguous()
    A = rows(dY).to(dt)
    kw = dict(head_calls.aux0_dgrad(M, C, len(brs)), A=A, W=wt, rowoff=tab, epilogue=EPI_OUT_F32)
    g = sum(rows(_conv_input_grad(weights[bi], dY[:, bi * C:(bi + 1) * C], dt)) for bi in brs)
    if prior is None:
        kw["out"] = torch.empty((M, C), dtype=f32)
    else:
        kw["out"] = prior.to(f32).reshape(M, C).clone()
        kw["residual"] = kw["out"]
        g = g + kw["out"].double()
    return Call("aux0_resid" if prior is not None else "aux0", kw, g)


# ---------------------------------------------------------------------------------------------------------------
# vit_train.py
# ---------------------------------------------------------------------------------------------------------------
def linear_dgrad(kind, weight, dY, dt, out_f32=True) -> Call:
    """dX = dY W through vit_train._wt.  weight (n_out, n_in); dY [M, n_out].  The fc2, fc1 and qkv gradients write
    f32; the proj gradient (out_f32 False) writes the compute dtype with no epilogue bit."""
    n_out, n_in = weight.shape
    M = dY.shape[0]
    A = dY.to(dt).contiguous()
    kw = dict(A=A, W=vit_train._wt(weight, dt), out=torch.empty((M, n_in), dtype=f32 if out_f32 else dt), M=M, N=n_in,
              Kd=n_out, lda=n_out, ldw=n_out, ldc=n_in)
    if out_f32:
        kw["epilogue"] = EPI_OUT_F32
    w64 = weight.detach().to(dt).double()
    return Call(kind, kw, _input_grad(lambda x: F.linear(x, w64), (M, n_in), A))


def train_linear(kind, x, weight, bias, dt, residual=None) -> Call:
    """A train-mode forward linear with an f32 output, through ops.linear as vit_train calls it: with an out-of-place
    f32 residual (proj, fc2), or without one (a branch under drop path, fc1's pre-activation)."""
    M, N = x.shape[0], weight.shape[0]
    A, W, b = x.to(dt).contiguous(), weight.detach().to(dt).contiguous(), bias.detach().float().contiguous()
    out = torch.empty((M, N), dtype=f32)
    got = {}
    real = ops.gemm
    ops.gemm = lambda A_, W_, out_, **kw: got.update(kw, A=A_, W=W_, out=out_)
    try:
        if residual is not None:
            residual = residual.to(f32).contiguous()
            ops.linear(A, W, b, out=out, residual=residual)
        else:
            ops.linear(A, W, b, out=out, out_dtype=f32)
    finally:
        ops.gemm = real
    kw = {k: v for k, v in got.items() if v is not None}
    truth = F.linear(A.double(), W.double(), b.double())
    if residual is not None:
        truth = truth + residual.double()
    return Call(kind, kw, truth)


# ---------------------------------------------------------------------------------------------------------------
# the restatement of a Call, and the comparison every test makes
# ---------------------------------------------------------------------------------------------------------------
def restated(call: Call):
    """(ref float64, written bool), shaped like out: gemm_reference.expected_output over a NaN-bit buffer (over the
    prior values for an in-place residual call)."""
    out = call.kw["out"]
    before = out.reshape(-1).clone() if call.in_place else gr.nan_like_bits(out.numel(), out.dtype, out.device)
    ref, written = gr.expected_output(call.kw, before)
    return ref.view(out.shape), written.view(out.shape)


def equals_truth(call: Call) -> bool:
    ref, written = restated(call)
    return bool(written.all()) and torch.equal(ref, call.truth)


# ---------------------------------------------------------------------------------------------------------------
# case shapes and data
# ---------------------------------------------------------------------------------------------------------------
_LIN = [(70, 64, 256), (195, 64, 256)]                       # (M, C, hidden)
CASES = {
    "final": [(K, M, cin) for K in (5, 17, 133) for M in (30, 195, 385) for cin in (64, 256)],
    "deconv": [(1, 1, 1, 8, 64), (2, 5, 3, 24, 64), (3, 13, 5, 200, 64), (5, 11, 7, 40, 128), (2, 5, 3, 6, 64)],
    "aux_stage": [(1, 2, 2, 64), (2, 5, 3, 64), (3, 13, 5, 64), (1, 3, 2, 256)],
    "aux0": [(g, brs) for g in ((2, 5, 3, 64), (3, 13, 5, 64)) for brs in ((0,), (1,), (0, 1))],
    "fc2_dgrad": _LIN, "fc1_dgrad": _LIN, "qkv_dgrad": _LIN,
    # whole-tile shapes (M, C, C) with K >= 512 for the persistent, duo and stream forms
    "proj_dgrad": _LIN + [(768, 576, 576), (768, 768, 512)],
    "fwd_resid": [(M, C, hid, which) for M, C, hid in _LIN for which in ("proj", "fc2")],
    "fwd_branch": [(M, C, hid, which) for M, C, hid in _LIN for which in ("proj", "fc2")],
    "fwd_fc1": _LIN,
}
CASES["aux0_resid"] = CASES["aux0"]
KINDS = tuple(CASES)
PROJ_HOT = 28       # non-zeros per dY row of the exact proj case: |sum| <= 28 * 3 * 3 = 252 <= 256, exact in bf16


def make(kind: str, case, dt, ints: bool, seed: int = 0) -> Call:
    """The Call of one case with seeded data: integers in [-3, 3], or randn gradients and randn * Kd^-1/2 weights."""
    gen = torch.Generator().manual_seed(seed)

    def draw(shape, scale=1.0):
        if ints:
            return torch.randint(-3, 4, shape, generator=gen).float()
        return torch.randn(shape, generator=gen) * scale

    if kind == "final":
        K, M, cin = case
        KPAD = head_calls.kpad(K)
        return final_dgrad(draw((K, cin, 1, 1), KPAD ** -0.5), draw((M, KPAD)), dt)
    if kind == "deconv":
        B, h, w, cin, cout = case
        return deconv_dgrad(draw((cin, cout, 4, 4), (16 * cout) ** -0.5), draw((B, cout, 2 * h, 2 * w)), dt)
    if kind == "aux_stage":
        B, h, w, C = case
        return aux_stage_dgrad([draw((C, C, 3, 3), (9 * C) ** -0.5) for _ in range(4)], draw((B, 4 * C, h, w)), dt)
    if kind in ("aux0", "aux0_resid"):
        (B, h, w, C), brs = case
        ws = [draw((C, C, 3, 3), (9 * len(brs) * C) ** -0.5) for _ in range(4)]
        dY = draw((B, 4 * C, h, w))
        return aux0_dgrad(ws, dY, brs, dt, prior=draw((B * h * w, C)) if kind == "aux0_resid" else None)
    if kind.endswith("_dgrad"):
        M, C, hid = case
        if kind == "proj_dgrad":
            n_out, n_in = (C, C) if case in _LIN else (hid, C)       # the whole-tile rows are (M, N, K)
        else:
            n_out, n_in = {"fc2_dgrad": (C, hid), "fc1_dgrad": (hid, C), "qkv_dgrad": (3 * C, C)}[kind]
        weight = draw((n_out, n_in), n_out ** -0.5)
        dY = draw((M, n_out))
        if kind == "proj_dgrad" and ints:       # a bf16 output: keep every result an integer within +-256
            keep = torch.rand((M, n_out), generator=gen).argsort(dim=1) < PROJ_HOT
            dY = dY * keep
        return linear_dgrad(kind, weight, dY, dt, out_f32=kind != "proj_dgrad")
    if kind in ("fwd_resid", "fwd_branch"):
        M, C, hid, which = case
        n_in = C if which == "proj" else hid
        x, weight, bias = draw((M, n_in)), draw((C, n_in), n_in ** -0.5), draw((C,))
        return train_linear(kind, x, weight, bias, dt, residual=draw((M, C)) if kind == "fwd_resid" else None)
    if kind == "fwd_fc1":
        M, C, hid = case
        return train_linear(kind, draw((M, C)), draw((hid, C), C ** -0.5), draw((hid,)), dt)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------
# planted faults: a wrong packer in place of the product's
# ---------------------------------------------------------------------------------------------------------------
def _conv_w(perm, flip=True):
    def f(w):
        w = w.flip(2, 3) if flip else w
        return w.permute(*perm).reshape(w.shape[perm[0]], -1).contiguous()
    return f


def _deconv_w(perm):
    return lambda w: w.permute(*perm).reshape(w.shape[perm[0]], -1).contiguous()


def _pad_as_row_zero(real):
    return lambda *a, **k: real(*a, **k).clamp_min(0)


def _reversed_branches(real):
    return lambda B, h, w, C, brs, dev: real(B, h, w, C, list(reversed(brs)), dev)


def _with(**wrong):
    """A head_calls descriptor with some keywords replaced: wrong[key](the right value) -> the wrong one."""
    return lambda real: lambda *a, **k: {key: (wrong[key](v) if key in wrong else v) for key, v in real(*a, **k).items()}


_CONV_KINDS = ("aux_stage", "aux0", "aux0_resid")
# name: (module, attribute, wrong function or a wrapper of the real one, wraps the real one?, the kinds it must fail)
FAULTS = {
    "conv3x3 taps not flipped": (pack, "conv3x3_data_grad_weights", _conv_w((1, 2, 3, 0), flip=False), False, _CONV_KINDS),
    "conv3x3 ky and kx swapped": (pack, "conv3x3_data_grad_weights", _conv_w((1, 3, 2, 0)), False, _CONV_KINDS),
    "conv3x3 Cin and Cout swapped": (pack, "conv3x3_data_grad_weights", _conv_w((0, 2, 3, 1)), False, _CONV_KINDS),
    "deconv taps flipped": (pack, "deconv_data_grad_weights", lambda w: _deconv_w((0, 2, 3, 1))(w.flip(2, 3)), False,
                            ("deconv",)),
    "deconv ky and kx swapped": (pack, "deconv_data_grad_weights", _deconv_w((0, 3, 2, 1)), False, ("deconv",)),
    "deconv Cin and Cout swapped": (pack, "deconv_data_grad_weights", _deconv_w((1, 2, 3, 0)), False, ("deconv",)),
    "deconv table pad off by one": (pack, "deconv_geometry", lambda k: (2, 0), False, ("deconv",)),
    "deconv table -1 as offset 0": (pack, "deconv_data_grad_table", _pad_as_row_zero, True, ("deconv",)),
    "conv table -1 as offset 0": (pack, "conv_gather_table", _pad_as_row_zero, True, _CONV_KINDS),
    "aux-0 table -1 as offset 0": (head_train, "_aux0_dgrad_table", _pad_as_row_zero, True, ("aux0", "aux0_resid")),
    "aux-0 branch order reversed": (head_train, "_aux0_dgrad_table", _reversed_branches, True, ("aux0", "aux0_resid")),
    # one per head_calls descriptor these builders use: the comparison sees the product's call, not a transcription
    "final dgrad weight pitch short": (head_calls, "final_dgrad", _with(ldw=lambda v: v - 16), True, ("final",)),
    "deconv dgrad last tap dropped": (head_calls, "deconv_dgrad", _with(Kd=lambda v: v - v // 16), True, ("deconv",)),
    "aux stage strideC wrong": (head_calls, "aux_stage", _with(strideC=lambda v: v // 2), True, ("aux_stage",)),
    "aux stage strideW wrong": (head_calls, "aux_stage", _with(strideW=lambda v: v // 9), True, ("aux_stage",)),
    "aux-0 dgrad last segment dropped": (head_calls, "aux0_dgrad", _with(Kd=lambda v: v - 64), True,
                                         ("aux0", "aux0_resid")),
    "_wt not transposed": (vit_train, "_wt", lambda p, dt: p.detach().to(dt).contiguous(), False, ("proj_dgrad",)),
}


# the case each kind's faults are planted on: maps of at least 2 x 2 (on a 1 x 1 map only the centre tap is in range and
# a missing flip cannot be seen), square layers where two axes are swapped, two branches where their order is
FAULT_CASES = {
    "deconv": (2, 3, 2, 64, 64), "aux_stage": (2, 5, 3, 64), "aux0": ((2, 5, 3, 64), (0, 1)),
    "aux0_resid": ((2, 5, 3, 64), (0, 1)), "proj_dgrad": (70, 64, 256), "final": (17, 30, 64),
}


@contextlib.contextmanager
def planted(name: str):
    """Builders run inside build with the named packer replaced by its wrong variant."""
    mod, attr, fn, wraps, _ = FAULTS[name]
    real = getattr(mod, attr)
    setattr(mod, attr, fn(real) if wraps else fn)
    try:
        yield
    finally:
        setattr(mod, attr, real)
