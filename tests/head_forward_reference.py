"""Restatements for the forward head kernels of csrc/pp_ops.hip, pp_sparsemax.hip and pp_dark.hip (CPU only; pinned by
tests/test_head_forward_reference.py, used by tests/test_head_forward_forms_gpu.py).

* ``final_heatmap_form`` restates the host dispatch of pp_final_heatmap / pp_final_logits (final_heatmap_launch): which
  kernel instantiation a call runs, with how much LDS, and for the matrix-core form how its 16-row tiles fall on waves.
* ``final_heatmap_f64`` is the float64 value of the layer on the operands as stored.
* ``coded_operands`` builds operands whose result is exact in float32 in any summation order and names the output
  element it belongs to, so that an indexing error of any size changes bits.
* float64 / exact restatements of patchify, the two poolings, the aux tail and the layout transposes.
* ``dark_tolerance`` bounds what one float32 ulp in logf may move a DARK keypoint.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import probpose_oracle as orc

BF16, F32 = torch.bfloat16, torch.float32
_CT = {F32: "float", BF16: "unsigned short"}          # kernel template argument T
FH_ROWS, FHM_MAXKS, FHM_MAXK = 64, 16, 144


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# final heatmap / logits: host dispatch
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    name: str                       # the kernel instantiation
    lds: int                        # dynamic LDS bytes of the launch
    tiles: Optional[int] = None     # MFMA form: 16-row tiles, waves of the launch, most tiles one wave takes
    nwaves: Optional[int] = None
    max_tiles: Optional[int] = None

    @property
    def mfma(self):
        return self.tiles is not None

    def tiles_per_wave(self):
        """The set of tile counts that the launch's waves take (0: an idle wave)."""
        return {cdiv(max(self.tiles - wv, 0), self.nwaves) for wv in range(self.nwaves)}


def final_heatmap_form(dtype, B, HW, Cin, K, x_mod16=0, w_mod16=0, out_mod16=0, clamp=True, temperature=1.0):
    """final_heatmap_launch<CLAMP> of pp_ops.hip restated.  None: the host refuses the call."""
    if not (B > 0 and HW > 0 and Cin > 0 and K > 0) or temperature == 0:
        return None
    es = 2 if dtype == BF16 else 4
    vec = 16 // es
    if Cin % vec or B * HW >= 2 ** 31:
        return None
    M = B * HW
    c = "true" if clamp else "false"
    if (dtype == BF16 and HW % 16 == 0 and Cin % 32 == 0 and Cin <= 32 * FHM_MAXKS and K <= FHM_MAXK
            and x_mod16 == 0 and w_mod16 == 0 and out_mod16 == 0):
        nt = cdiv(K, 16)
        NT = 2 if nt <= 2 else (4 if nt <= 4 else 9)
        tiles = M // 16
        nwaves = 4 * min(cdiv(tiles, 4), 512)
        return Form(f"final_heatmap_mfma_kernel<{NT}, {c}>", NT * 16 * (Cin * 2 + 16), tiles, nwaves,
                    cdiv(tiles, nwaves))
    lds = FH_ROWS * (Cin // vec + 1) * 16 + K * Cin * es
    if lds > 160 * 1024:
        return None
    return Form(f"final_heatmap_kernel<{_CT[dtype]}, {c}>", lds)


FH_FORMS = ([f"final_heatmap_mfma_kernel<{nt}, {c}>" for nt in (2, 4, 9) for c in ("true", "false")]
            + [f"final_heatmap_kernel<{t}, {c}>" for t in ("float", "unsigned short") for c in ("true", "false")])


def _fh(dtype, B, HW, Cin, K, out_off=0, note=""):
    return dict(dtype=dtype, B=B, HW=HW, Cin=Cin, K=K, out_off=out_off, note=note)


def _fh_cases():
    cs = []
    # matrix-core form, bf16, every pointer 16-byte aligned
    cs.append(_fh(BF16, 1, 16, 32, 1, note="one tile, three idle waves, ks = 1"))
    cs += [_fh(BF16, 3, 48, 256, K, note="NT = 2") for K in (16, 17, 32)]
    cs += [_fh(BF16, 3, 48, 64, K, note="NT = 4") for K in (33, 48, 64)]
    cs += [_fh(BF16, 2, 48, 512, K, note="NT = 9, ks = 16") for K in (65, 144)]
    cs.append(_fh(BF16, 1367, 48, 32, 17, note="4101 tiles on 2048 waves: 3 and 2 tiles"))
    cs.append(_fh(BF16, 1367, 48, 64, 40, note="the same loop with NT = 4"))
    cs.append(_fh(BF16, 11, 3072, 256, 17, note="ViT-B map, 2112 tiles: 2 and 1 tile"))
    cs.append(_fh(BF16, 5, 6912, 256, 133, note="whole-body map, NT = 9, 2160 tiles"))
    # VALU form
    for dt, Cin in ((F32, 36), (BF16, 40)):
        cs += [_fh(dt, 3, 50, Cin, K, note="k passes") for K in (20, 21, 24, 41)]
        cs += [_fh(dt, 1, M, Cin, 5, note="row tails") for M in (1, 63, 64, 65, 129)]
        cs.append(_fh(dt, 70, 1, Cin, 5, note="HW = 1"))
    cs += [_fh(F32, 3, 50, 4, 5, note="one chunk per row"), _fh(BF16, 3, 50, 8, 5, note="one chunk per row")]
    cs.append(_fh(F32, 2, 50, 256, 60, note="dynamic LDS, 128 000 B"))
    cs.append(_fh(BF16, 2, 48, 256, 145, note="fall-back: K > 144"))
    cs.append(_fh(BF16, 2, 48, 544, 17, note="fall-back: Cin > 512"))
    cs.append(_fh(BF16, 3, 50, 64, 17, note="fall-back: HW % 16"))
    cs.append(_fh(BF16, 3, 48, 40, 17, note="fall-back: Cin % 32"))
    cs.append(_fh(BF16, 3, 48, 256, 17, out_off=4, note="fall-back: out 4 bytes off 16-byte alignment"))
    return cs


FH_CASES = _fh_cases()
# (dtype, B, HW, Cin, K, temperature): each is refused and writes nothing
FH_REFUSALS = [(F32, 3, 50, 38, 5, 0.5), (BF16, 3, 50, 36, 5, 0.5), (F32, 3, 50, 36, 5, 0.0), (BF16, 3, 48, 256, 17, 0.0),
               (F32, 1, 64, 256, 133, 0.5)]


def fh_case_id(c):
    s = f"{str(c['dtype'])[6:]}-B{c['B']}-HW{c['HW']}-C{c['Cin']}-K{c['K']}"
    return s + (f"-out+{c['out_off']}B" if c["out_off"] else "")


def fh_case_form(c, clamp=True):
    return final_heatmap_form(c["dtype"], c["B"], c["HW"], c["Cin"], c["K"], 0, 0, c["out_off"] % 16, clamp, 0.5)


# ---------------------------------------------------------------------------------------------------------------
# final heatmap / logits: values
# ---------------------------------------------------------------------------------------------------------------
def final_heatmap_f64(x, w, bias, B, HW, K, T, clamp):
    """x [B*HW, Cin], w [K, Cin] as stored (bf16 or f32), bias [K] f32 -> float64 [B, K, HW]:
    (x w^T + bias) / T, torch.clamp(., 0, 1) if clamp."""
    v = (x.double() @ w.double().t() + bias.double()) / float(T)
    if clamp:
        v = torch.clamp(v, 0.0, 1.0)
    return v.reshape(B, HW, K).permute(0, 2, 1).contiguous()


def product_clamp(v):
    """What pp_final_heatmap gives for the float64 pre-clamp value v: fminf(fmaxf(v, 0), 1), where a NaN gives 0
    (include/probpose_hip.h), unlike torch.clamp."""
    return torch.clamp(torch.nan_to_num(v, nan=0.0, posinf=float("inf"), neginf=-float("inf")), 0.0, 1.0)


def _pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


@dataclass
class Coded:
    x: torch.Tensor            # [M, Cin] float32 holding values exact in bf16
    w: torch.Tensor            # [K, Cin]
    bias: torch.Tensor         # [K] float32, distinct per k
    T: float                   # a power of two
    abs_sum: float             # max over (m, k) of sum_c |x w| + |bias|: every partial sum of any order is below it


def coded_operands(B, HW, Cin, K, which, clamp):
    """Operands whose every product and partial sum is an exact float32 (abs_sum < 2^24, T a power of two), so that
    (x w^T + bias) / T is the same float32 in any summation order: the kernels' results are known bit for bit.

    which = "m": the value is m P + k (P = the power of two >= K): it names the row m and, through the bias alone, k.
    which = "k": the value is 256 k + m % 256 + (k + 1) / 256: the weights carry k.
    Columns 0 and Cin - 1 carry the code; the columns between hold +1 / -1 against weights of 1 and cancel only if every
    one of them is summed.  clamp: the bias is lowered by T / 2 and the power of two T chosen so that the values span
    [-0.5, vmax / T - 0.5] with vmax / T in (1.5, 3]: both bounds of clamp(., 0, 1) bind; otherwise T = 0.5."""
    M = B * HW
    assert Cin >= 4 and Cin % 2 == 0 and K <= 256 and M <= 256 * 257
    m, k = torch.arange(M), torch.arange(K)
    x, w = torch.zeros((M, Cin)), torch.zeros((K, Cin))
    half = (Cin - 2) // 2
    x[:, 1:1 + half], x[:, 1 + half:Cin - 1] = 1.0, -1.0
    w[:, 1:Cin - 1] = 1.0
    if which == "m":
        P = _pow2_at_least(K)
        x[:, 0], x[:, Cin - 1] = (m % 256).float(), (m // 256).float()
        w[:, 0], w[:, Cin - 1] = float(P), float(256 * P)
        bias = k.float()
        vmax = (M - 1) * P + K - 1
    else:
        x[:, 0], x[:, Cin - 1] = (m % 256).float(), 256.0
        w[:, 0], w[:, Cin - 1] = 1.0, k.float()
        bias = (k + 1).float() / 256.0
        vmax = 256 * (K - 1) + min(M - 1, 255) + 1
    T = 0.5
    if clamp:
        T = float(_pow2_at_least(max(vmax, 2) / 1.5)) / 2.0          # vmax / T in (1.5, 3]
        bias = bias - T / 2.0
    abs_sum = float((x.abs().double() @ w.abs().double().t() + bias.abs().double()).max())
    return Coded(x, w, bias, T, abs_sum)


def bits_differ(got: torch.Tensor, want64: torch.Tensor) -> int:
    """The comparator of the exact runs: elements of the float32 `got` whose bits are not those of `want64` as float32
    (-0.0 and +0.0 count as equal, any NaN equals any NaN).  want64 must be exact in float32."""
    want = want64.to(torch.float32)
    assert torch.equal(torch.nan_to_num(want.double()), torch.nan_to_num(want64)), "the expected values are not float32"
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    return int((~same).sum())


def out_of_bound(got: torch.Tensor, ref64: torch.Tensor, rtol, atol):
    """(elements with |got - ref| > rtol |ref| + atol, NaN counting as out; the worst |got - ref| / bound)."""
    d = (got.double() - ref64).abs()
    bound = rtol * ref64.abs() + atol
    bad = ~(d <= bound)
    ratio = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d / bound)
    return int(bad.sum()), float(ratio.max()) if d.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# the other forward ops
# ---------------------------------------------------------------------------------------------------------------
def patchify_ref(x, p, dtype):
    """x [B, 3, H, W] f32 -> [B * (H // p) * (W // p), 3 p p] in dtype; rows and columns past the last whole patch drop."""
    return F.unfold(x, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p).to(dtype)


def _pool_relu(v, B, h, w, C, kh, kw):
    oh, ow = h // kh, w // kw
    win = v.reshape(B, h, w, C)[:, :oh * kh, :ow * kw].reshape(B, oh, kh, ow, kw, C)
    return torch.relu(win.amax(dim=(2, 4))).reshape(B * oh * ow, C)      # amax and relu keep a NaN, like max_pool2d


def maxpool_relu_ref(x, B, h, w, C, kh, kw):
    """x [B*h*w, C] channels-last -> ReLU(MaxPool) [B*(h//kh)*(w//kw), C] in x's dtype (a selection: exact)."""
    return _pool_relu(x.float(), B, h, w, C, kh, kw).to(x.dtype)


def maxpool_relu_sum_ref(parts, bias, B, h, w, C, kh, kw, dtype):
    """parts [S, >= B*h*w*C] f32 (only the first B*h*w*C of a split are read), bias [C]: the partials added in split
    order in float32, then the bias, then the pooling; cast to dtype (round to nearest even)."""
    n = B * h * w * C
    a = parts[0, :n].clone().float()
    for s in range(1, parts.shape[0]):
        a = a + parts[s, :n]
    a = a.reshape(B * h * w, C) + bias.float()
    return _pool_relu(a, B, h, w, C, kh, kw).to(dtype)


def aux_tail_ref(x, w, bias):
    """x [B, 4 C] (branch br at columns br C ..), w [4, K, C], bias [4, K] -> float64 [4, B, K]: sigmoid for branches
    0-2, ReLU for branch 3 (torch's: a NaN stays)."""
    nbr, K, C = w.shape
    out = []
    for br in range(nbr):
        pre = x[:, br * C:(br + 1) * C].double() @ w[br].double().t() + bias[br].double()
        out.append(torch.relu(pre) if br == 3 else torch.sigmoid(pre))
    return torch.stack(out)


AUX_STEPS = (2.0 ** -6, -(2.0 ** -6), 2.0 ** -7, 1.0)


def aux_coded(B, C, K):
    """Coded aux-tail operands, exact in bf16.  Branch br reads x only at its own column cb = (3 br + 1) % C (the crop
    index b; every other column holds 0.5 against a weight of 0 in that branch) and its pre-activation is
    AUX_STEPS[br] (b K + k - (B K) // 2): exact in float32, it names (b, k), and each branch has its own step, sign,
    weights and bias.  A read from another branch's columns or weights meets a 0.5 or a 0 instead."""
    assert C >= 8 and K * 1 <= 256 and B <= 256
    x = torch.full((B, 4 * C), 0.5)
    w = torch.zeros((4, K, C))
    bias = torch.zeros((4, K))
    k = torch.arange(K).float()
    for br, step in enumerate(AUX_STEPS):
        cb = (3 * br + 1) % C
        x[:, br * C + cb] = torch.arange(B).float()
        w[br, :, cb] = K * step
        bias[br] = (k - (B * K) // 2) * step
    return x, w, bias


def tokens_to_nchw_ref(x, B, N, C):
    return x.float().reshape(B, N, C).permute(0, 2, 1).contiguous()


def nchw_to_tokens_ref(x, B, C, HW, dtype):
    return x.reshape(B, C, HW).permute(0, 2, 1).contiguous().to(dtype)


# ---------------------------------------------------------------------------------------------------------------
# DARK
# ---------------------------------------------------------------------------------------------------------------
DARK_CASES = [(2, 2, 1), (2, 2, 3), (2, 2, 11), (2, 2, 31), (3, 5, 1), (3, 5, 3), (3, 5, 11), (3, 5, 31),
              (8, 6, 1), (8, 6, 3), (8, 6, 11), (8, 6, 31), (33, 27, 1), (33, 27, 3), (33, 27, 11), (33, 27, 31),
              (64, 48, 1), (64, 48, 3), (64, 48, 11), (64, 48, 31)]                     # (H, W, ksize)
DARK_SIGMAS = (1.0, 2.0, 3.0)


def dark_blob_centres(H, W):
    """(cx, cy) of the K = 9 blobs: the four corners, four edge mid-points off the grid along the edge, the interior."""
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W / 2 - .3, 0), (W / 2 + .2, H - 1), (0, H / 2 - .4),
            (W - 1, H / 2 + .3), (W / 2 - .3, H / 2 + .4)]


def dark_blobs(H, W):
    """[3, 9, H, W] float32: crop b holds the nine blobs with sigma DARK_SIGMAS[b], amplitude 0.9."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([np.stack([(0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))).astype(np.float32)
                               for cx, cy in dark_blob_centres(H, W)]) for sg in DARK_SIGMAS])


def dark_tolerance(hm, ksize, in_size):
    """hm [K, H, W] f32 -> [K, 2] float64: how far pp_dark_decode_f32 may be from orc.dark_udp_decode, in input pixels.

    The kernel's blur is the oracle's bit for bit (same order, no contraction); only logf against np.log differs, by at
    most one float32 ulp of L: delta = 2^-23 max(max |L| over the seven stencil points, 1).  dx, dy then move by at most
    delta, dxx, dyy, dxy by at most 4 delta; to first order the step p = H^-1 g moves by at most
    (|dg| + |dH| |p|) / lambda_min <= (2 + 8 max|p|) delta / lambda_min, lambda_min the smaller absolute eigenvalue of
    the oracle's Hessian + eps I.  A factor 2 covers second order; scale = in_size / (W - 1, H - 1).  Dead maps: 0."""
    K, H, W = hm.shape
    scale = np.array([in_size[0] / (W - 1), in_size[1] / (H - 1)], np.float64)
    tol = np.zeros((K, 2), np.float64)
    for k in range(K):
        if not hm[k].max() > 0:
            continue
        L = orc.gaussian_blur_zero_padded(hm[k], ksize)
        np.clip(L, 1e-3, 50., L)
        np.log(L, L)
        Lp = np.pad(L, 1, mode="edge").astype(np.float64)
        a = int(np.argmax(hm[k]))
        y, x = a // W + 1, a % W + 1
        i_, ix1, iy1 = Lp[y, x], Lp[y, x + 1], Lp[y + 1, x]
        ix1y1, ix1_y1_, ix1_, iy1_ = Lp[y + 1, x + 1], Lp[y - 1, x - 1], Lp[y, x - 1], Lp[y - 1, x]
        dx, dy = .5 * (ix1 - ix1_), .5 * (iy1 - iy1_)
        dxx, dyy = ix1 - 2 * i_ + ix1_, iy1 - 2 * i_ + iy1_
        dxy = .5 * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_)
        Hm = np.array([[dxx, dxy], [dxy, dyy]], np.float64) + np.finfo(np.float32).eps * np.eye(2)
        lam = np.abs(np.linalg.eigvalsh(Hm)).min()
        p = np.abs(np.linalg.pinv(Hm) @ np.array([dx, dy], np.float64)).max()
        delta = 2.0 ** -23 * max(max(abs(v) for v in (i_, ix1, iy1, ix1y1, ix1_y1_, ix1_, iy1_)), 1.0)
        tol[k] = scale * 2 * (2 + 8 * p) * delta / lam + 1e-9
    return tol


def sparsemax_ref(z: torch.Tensor) -> torch.Tensor:
    """orc.sparsemax_lastdim: a row holding a NaN or +Inf comes back all NaN by torch's own rules (x.max keeps the
    NaN; Inf - Inf is NaN; torch.max(0, z - tau) keeps it), so nothing is restated here
    (tests/test_head_forward_reference.py checks that)."""
    return orc.sparsemax_lastdim(z)
