"""Execution plans: packed weights + cached workspaces + the launch sequence of
the HIP kernels for the ViT backbone and the ProbMapHead.

A plan is built from an ``nn.Module``'s parameters (the modules in
backbone.py / head.py only hold parameters and structure, mirroring the
reference's attribute names) and re-built when the parameters change.  All
activations stay on the device as channels-last rows; the residual stream is
fp32, GEMM operands are ``dtype`` (bf16: ``v_mfma_f32_16x16x32_bf16``; fp32:
exact ``v_mfma_f32_16x16x4_f32``).
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, head_calls, ops, pack
from ._buffers import CaptureCache
from .ops import EPI_GELU, EPI_OUT_F32, EPI_RELU

_PLANS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()

# bench.py's kernel-timing pass sets this to run the head's two branches back to back on one stream,
# so that per-launch event timings are not inflated by the other branch sharing the CUs
SERIALIZE_HEAD = False

# Run the ViT blocks of a batch as two half-batch kernel chains on two HIP streams (see VitPlan.forward_tokens).
# fp8 mode: also run attn.proj on the fp8 MFMA (attention then writes e4m3 with a static per-tensor scale).  Off: on the
# synthetic ViT-B it buys +2.5 % throughput but moves the decoded keypoints by a median of 4 px against the bf16 path
# (0.3 px without it): one scale per tensor is too coarse for the attention output (tools/fp8_deviation.py).
FP8_PROJ = False
DUAL_CHAIN = False
DUAL_CHAIN_MIN_BATCH = 16
# aux stages >= 1 (M = 16 B / 4 B rows, K = 9 C) as split-K launches with the reduction folded into the pooling kernel
SPLITK_AUX = True
# bf16 heads with K <= 32 keypoints: the last deconvolution's epilogue applies the final 1x1 layer (see HeadPlan._forward)
FUSE_FINAL = True
# head-major q / k / v for head dims that are not whole cache lines (see VitPlan.__init__)
HEADMAJOR_QKV = True
# bf16 models with N = 192 tokens and head_dim 64 (ViT-B / ViT-L at 256x192): attn.qkv and the attention of a block run as
# one launch (ops.qkv_attention) that keeps q, k and v in LDS; see VitPlan.__init__.  Read at plan build (the packed
# weights) and at every forward (off: the two-kernel path, on the same plan).
FUSE_QKV_ATTENTION = True


def _signature(module: torch.nn.Module):
    sig = []
    for t in list(module.parameters()) + list(module.buffers()):
        sig.append((t.data_ptr(), t._version, t.dtype, t.device))
    return tuple(sig)


def plan_for(module, builder, dtype: torch.dtype, device):
    """Cached plan of ``module`` for (dtype, device); rebuilt when any parameter changed."""
    entry = _PLANS.get(module)
    key = (dtype, str(device))
    sig = _signature(module)
    if entry is None or entry[0] != key or entry[1] != sig:
        entry = (key, sig, builder(module, dtype, device))
        _PLANS[module] = entry
    return entry[2]


def _dev(t: torch.Tensor, device, dtype=None):
    t = t.detach()
    return t.to(device=device, dtype=dtype if dtype is not None else t.dtype).contiguous()


class _Workspace:
    """Named scratch tensors.  Every buffer is row-major [rows, ...]: one allocation per name serves every batch
    size up to the largest seen (smaller batches get the leading rows: contiguous views at a stable address, so
    captured graphs stay valid).  A larger batch allocates a new buffer; the cache keeps the old one alive if a
    captured graph points into it, but it is no longer handed out."""

    def __init__(self):
        self._bufs = CaptureCache()

    def get(self, name: str, shape, dtype, device) -> torch.Tensor:
        shape = tuple(shape)
        t = self._bufs.get((name, shape[1:], dtype), lambda: torch.empty(shape, dtype=dtype, device=device),
                           lambda t: t.shape[0] >= shape[0])
        return t[: shape[0]]


# ---------------------------------------------------------------------------
# ViT backbone
# ---------------------------------------------------------------------------
def pack_embed(vit, dtype, device=None):
    """(patch_embed.proj weight [C, 3 p p] in ``dtype``, its bias, pos_embed [N, C]) as patch_embed() reads them."""
    C = vit.embed_dim
    pe = vit.patch_embed.proj
    return (_dev(pe.weight.reshape(C, -1), device, dtype), _dev(pe.bias, device, torch.float32),
            _dev(vit.pos_embed.reshape(-1, C), device, torch.float32))


def pack_block(blk, dtype, device=None) -> dict:
    """One ViT block's parameters as the kernels read them: the four weight matrices in ``dtype``, biases and LayerNorm
    parameters f32; detached, contiguous, on ``device`` (None: where they are).  VitPlan keeps the result; the training
    path (vit_train.py) packs at every forward."""
    f32 = torch.float32
    a, m = blk.attn, blk.mlp
    return dict(
        n1w=_dev(blk.norm1.weight, device, f32), n1b=_dev(blk.norm1.bias, device, f32), eps1=blk.norm1.eps,
        qkv_w=_dev(a.qkv.weight, device, dtype), qkv_b=_dev(a.qkv.bias, device, f32),
        proj_w=_dev(a.proj.weight, device, dtype), proj_b=_dev(a.proj.bias, device, f32),
        n2w=_dev(blk.norm2.weight, device, f32), n2b=_dev(blk.norm2.bias, device, f32), eps2=blk.norm2.eps,
        fc1_w=_dev(m.fc1.weight, device, dtype), fc1_b=_dev(m.fc1.bias, device, f32),
        fc2_w=_dev(m.fc2.weight, device, dtype), fc2_b=_dev(m.fc2.bias, device, f32))


def patch_embed(x, a0, xres, patch, w, bias, pos):
    """patchify, then patch_embed.proj as a GEMM, + bias, + pos_embed (row m uses pos[m % N]) -> the f32 residual
    stream xres [B*N, C]; a0 [B*N, 3 p p] is the patch matrix."""
    M, K0 = a0.shape
    C = w.shape[0]
    ops.patchify(x, a0, patch)
    ops.gemm(a0, w, xres, M=M, N=C, Kd=K0, lda=K0, ldw=K0, ldc=C, bias=bias, rowbias=pos,
             rowbias_period=pos.shape[0], epilogue=EPI_OUT_F32)


FP8_MARGIN = 1.25      # head-room of the static activation scales over the calibration amax (e4m3 saturates at 448)
# the four quantised activations of a block (LN1 output, attention output, LN2 output, GELU output) and the fp8 linear
# that reads each
_FP8_POINTS = dict(h1="qkv", ao="proj", h2="fc1", hid="fc2")


class VitPlan:
    def __init__(self, vit, dtype: torch.dtype, device, fp8: bool = False):
        self.dtype, self.device, self.fp8 = dtype, device, fp8
        pe = vit.patch_embed
        self.patch = int(pe.patch_size[0])
        self.img_size = tuple(pe.img_size)
        self.C = C = vit.embed_dim
        self.heads = vit.num_heads
        self.hd = C // self.heads
        self.N = pe.num_patches
        self.pe = pack_embed(vit, dtype, device)
        self.blocks = [pack_block(blk, dtype, device) for blk in vit.blocks]
        if fp8:
            # qkv / proj / fc1 / fc2 on fp8 MFMA: e4m3 weights, one scale per output channel (row of W); the activation
            # scales are static per tensor and come from a calibration pass on the first batch (_calibrate_fp8)
            for b, blk in zip(self.blocks, vit.blocks):
                for name, lin in (("qkv", blk.attn.qkv), ("proj", blk.attn.proj), ("fc1", blk.mlp.fc1),
                                  ("fc2", blk.mlp.fc2)):
                    b[name + "_w8"], b[name + "_sw"] = ops.quantize_rows_fp8(lin.weight.detach().to(device))
            self.fp8_calibrated = False
        self.nw = _dev(vit.norm.weight, device, torch.float32)
        self.nb = _dev(vit.norm.bias, device, torch.float32)
        self.neps = vit.norm.eps
        self.hidden = self.blocks[0]["fc1_w"].shape[0] if self.blocks else 4 * C
        # bf16 models whose head rows are not whole 128-byte lines (head_dim 80: ViT-H; 32 with N > 192) and that run the
        # streaming attention kernel: the qkv GEMM writes q / k / v head-major, so one head's rows are contiguous
        self.headmajor = (HEADMAJOR_QKV and dtype == torch.bfloat16 and not fp8 and
                          (self.hd == 80 or (self.hd == 32 and self.N > 192)))
        # one launch for attn.qkv + attention: the q, k and v rows of a head become one 192-row panel of a head-major
        # copy of qkv.weight / qkv.bias, packed once here (the parameters are constants of the plan).  The row-major
        # qkv_w stays as well (the two-kernel path on the same plan): + 3 C^2 bf16 per block, 42 MB at ViT-B, 151 MB
        # at ViT-L.  The packed copy is derived state, so the plan's first eager forward checks it: see _run_blocks.
        self.qkv_fused = (FUSE_QKV_ATTENTION and dtype == torch.bfloat16 and not fp8 and self.N == 192 and
                          self.hd == 64 and not self.headmajor and C >= 128)
        if self.qkv_fused:
            for b in self.blocks:
                b["qkv_w_hm"], b["qkv_b_hm"] = ops.pack_qkv_headmajor(b["qkv_w"], b["qkv_b"], self.heads)
        self.qkv_checked = False
        self.ws = _Workspace()
        self._chain_stream = None

    def _fuse_qkv(self) -> bool:
        return self.qkv_fused and FUSE_QKV_ATTENTION

    def _buffers(self, B: int, fused: bool = False) -> Dict[str, torch.Tensor]:
        """The workspace of a batch of B crops, by name; fp8 mode adds the e4m3 twins h8 / ao8 / hid8.  No qkv buffer
        where the fused qkv + attention launch runs."""
        dt, C = self.dtype, self.C
        cols = dict(a0=(3 * self.patch ** 2, dt), xres=(C, torch.float32), h=(C, dt), qkv=(3 * C, dt), ao=(C, dt),
                    hid=(self.hidden, dt), feats=(C, dt))
        if fused:
            del cols["qkv"]
        if self.fp8:
            cols.update(h8=(C, ops.FP8), ao8=(C, ops.FP8), hid8=(self.hidden, ops.FP8))
        return {k: self.ws.get(k, (B * self.N, n), t, self.device) for k, (n, t) in cols.items()}

    def forward_tokens(self, x: torch.Tensor) -> torch.Tensor:
        """x (B,3,H,W) f32 on the device -> tokens [B*N, C] in the compute dtype
        (= channels-last (B,gh,gw,C) feature map), final LayerNorm applied."""
        B, ch, H, W = x.shape
        if ch != 3 or (H, W) != self.img_size:
            raise AssertionError(f"Input size ({H}, {W}) doesn't match model {self.img_size}")
        with torch.cuda.device(self.device):      # kernels launch on the current stream of the plan's device
            return self._forward_tokens(x, B)

    def _forward_tokens(self, x: torch.Tensor, B: int) -> torch.Tensor:
        dual = DUAL_CHAIN and not SERIALIZE_HEAD and B % 2 == 0 and B >= DUAL_CHAIN_MIN_BATCH
        fused = self._fuse_qkv()
        bufs = self._buffers(B, fused)
        if self.fp8:
            if not self.fp8_calibrated:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("fp8 mode calibrates its activation scales on the first batch: run one eager "
                                       "forward before capturing a graph")
                self._calibrate_fp8(x, B, bufs)
            self._run_blocks(x, B, bufs, fp8=True)
        elif dual:
            # Two half-batches as two independent kernel chains on two HIP streams (row slices of the same
            # buffers, same weights).  Every kernel of the path is bulk-synchronous: all its workgroups
            # run their matrix phase together and then their store phase together, so one chain alone
            # alternates between an idle HBM and an idle matrix pipe.  The second chain starts one
            # GEMM later, so its memory phases fall into the first chain's matrix phases, and each
            # chain's tail wave is filled by the other chain's next kernel.
            if self._chain_stream is None:
                self._chain_stream = torch.cuda.Stream(device=self.device)
            cur, s2 = torch.cuda.current_stream(self.device), self._chain_stream
            Bh, Mh = B // 2, B * self.N // 2
            offset = torch.cuda.Event()
            self._run_blocks(x[:Bh], Bh, {k: t[:Mh] for k, t in bufs.items()}, offset_event=offset, fused=fused)
            s2.wait_event(offset)
            with torch.cuda.stream(s2):
                self._run_blocks(x[Bh:], Bh, {k: t[Mh:] for k, t in bufs.items()}, fused=fused)
            cur.wait_stream(s2)
        elif fused and not self.qkv_checked and not torch.cuda.is_current_stream_capturing():
            self._run_blocks(x, B, bufs, fused=True, check=True)
        else:
            self._run_blocks(x, B, bufs, fused=fused)
        return bufs["feats"]

    def _run_blocks(self, x, B, bufs, fp8=False, observe=None, offset_event=None, fused=False, check=False):
        """The launch sequence of one batch: patch embed, the blocks, the final LayerNorm into bufs["feats"].
        ``fp8``: LN and GELU write e4m3 (h8 / hid8) with the block's static scales, and qkv / fc1 / fc2 read the e4m3
        weights with their column scales; with FP8_PROJ so do attention (ao8) and proj.  ``observe(block, point, t)`` is
        called with each of the four _FP8_POINTS activations once it is enqueued (a calibration pass; it ends at the last
        block, since nothing reads its feats).  ``fused``: attn.qkv + attention as one launch (bufs has no "qkv").
        ``check`` (the plan's first eager fused walk): every block also runs the two launches, ops.linear on tile 14 and
        ops.attention, on the same h into scratch tensors, and the two outputs must be the same bits in every block; one
        synchronisation at the end, HipExtensionError otherwise (a wrong head-major copy of qkv.weight or a kernel that
        does not do on this device what the two launches do is an error, never a silent difference).  The scratch
        tensors (4 C bf16 per token) are freed when it returns."""
        fused = fused and not fp8 and observe is None
        if check:
            M = B * self.N
            qkv_ref = torch.empty((M, 3 * self.C), dtype=self.dtype, device=self.device)
            ao_ref = torch.empty((M, self.C), dtype=self.dtype, device=self.device)
            differ = torch.zeros((), dtype=torch.int64, device=self.device)
        xres, qkv = bufs["xres"], None if fused else bufs["qkv"]
        N, heads, hd = self.N, self.heads, self.hd
        q8 = "8" if fp8 else ""
        p8 = "8" if fp8 and FP8_PROJ else ""
        h, hid, ao = bufs["h" + q8], bufs["hid" + q8], bufs["ao" + p8]
        hm = (heads, hd) if self.headmajor else None
        patch_embed(x, bufs["a0"], xres, self.patch, *self.pe)
        if offset_event is not None and not self.blocks:
            offset_event.record()
        for i, b in enumerate(self.blocks):
            s = b if fp8 else {}           # static scales and column scales go with e4m3 operands only
            sp = s if p8 else {}
            ops.layernorm(xres, b["n1w"], b["n1b"], b["eps1"], h, out_scale=s.get("s_h1"))
            if i == 0 and offset_event is not None:
                offset_event.record()      # the other chain starts here: one patch-embed GEMM + LN behind
            if observe is not None:
                observe(b, "h1", h)
            if fused:
                if check:
                    ops.linear(h, b["qkv_w"], b["qkv_b"], out=qkv_ref, tile=14)
                    ops.attention(qkv_ref, ao_ref, B, N, heads, hd)
                ops.qkv_attention(h, b["qkv_w_hm"], b["qkv_b_hm"], ao, B, heads)
                if check:
                    differ += (ao.view(torch.int16) != ao_ref.view(torch.int16)).sum()
            else:
                ops.linear(h, b["qkv_w" + q8], b["qkv_b"], out=qkv, colscale=s.get("qkv_cs"), headmajor=hm)
                ops.attention(qkv, ao, B, N, heads, hd, out_scale=sp.get("s_ao"), headmajor=self.headmajor)
            if observe is not None:
                observe(b, "ao", ao)
            ops.linear(ao, b["proj_w" + p8], b["proj_b"], out=xres, residual=xres, colscale=sp.get("proj_cs"))
            ops.layernorm(xres, b["n2w"], b["n2b"], b["eps2"], h, out_scale=s.get("s_h2"))
            if observe is not None:
                observe(b, "h2", h)
            ops.linear(h, b["fc1_w" + q8], b["fc1_b"], out=hid, epilogue=EPI_GELU, colscale=s.get("fc1_cs"),
                       out_scale=s.get("s_hid"))
            if observe is not None:
                observe(b, "hid", hid)
            ops.linear(hid, b["fc2_w" + q8], b["fc2_b"], out=xres, residual=xres, colscale=s.get("fc2_cs"))
        if observe is None:
            ops.layernorm(xres, self.nw, self.nb, self.neps, bufs["feats"])
        if check:
            n = int(differ)
            if n:
                raise _lib.HipExtensionError(f"qkv_attention: {n} output elements differ from linear (tile 14) + attention "
                                             f"over {len(self.blocks)} blocks (B={B}, heads={heads}, C={self.C})")
            self.qkv_checked = True

    def _calibrate_fp8(self, x, B, bufs, margin: float = None):
        """One bf16 pass over the batch (the row-layout walk with an observer) recording amax of the four quantised
        activations of every block -> static scales margin * amax / 448, and the per-column dequantisation vectors
        (activation scale x weight-row scale) of the fp8 GEMMs.  Repeated calls (calibrate over several batches) keep
        the running maximum."""
        margin = FP8_MARGIN if margin is None else margin

        def observe(blk, point, t):
            a = max(float(t.float().abs().max()), 1e-6, blk.get("amax_" + point, 0.0))
            blk["amax_" + point] = a
            s = blk["s_" + point] = a * margin / ops.FP8_MAX
            lin = _FP8_POINTS[point]
            blk[lin + "_cs"] = (blk[lin + "_sw"] * s).contiguous()

        self._run_blocks(x, B, bufs, observe=observe)
        self.fp8_calibrated = True

    def calibrate(self, batches, margin: float = None):
        """Explicit fp8 calibration over representative batches (iterable of (B,3,H,W) device tensors): the static
        activation scales become margin * (max |activation| over all batches) / 448.  Without it the first forward
        calibrates on its own batch."""
        if not self.fp8:
            raise RuntimeError("calibrate() applies to the fp8 compute mode")
        for b in self.blocks:
            for k in [k for k in b if k.startswith("amax_")]:
                del b[k]
        with torch.cuda.device(self.device), torch.no_grad():
            for x in batches:
                x = x.detach().contiguous().float()
                self._calibrate_fp8(x, x.shape[0], self._buffers(x.shape[0]), margin)
        return self


def build_vit_plan(vit, dtype, device):
    if dtype == ops.FP8:
        return VitPlan(vit, torch.bfloat16, device, fp8=True)
    return VitPlan(vit, dtype, device)


# ---------------------------------------------------------------------------
# ProbMapHead
# ---------------------------------------------------------------------------
AUX_NAMES = ("probability", "visibility", "oks", "error")


def final_heatmap_fits(cin: int, K: int, dtype: torch.dtype) -> bool:
    """A 1x1 final layer runs as pp_final_heatmap when 64 padded input rows and the whole [K, cin] weight fit its LDS
    budget; otherwise as a pp_gemm with the heatmap epilogue."""
    es = 2 if dtype == torch.bfloat16 else 4
    return 64 * (cin * es + 16) + K * cin * es <= 150 * 1024


class HeadGeometry:
    """The layer dimensions of a ProbMapHead and the gather / scatter tables that follow from them and (B, h, w):
    what the eval plan and the training path (head_train.py) share.  deconvs / convs: one dict(k, cin, cout[, pad])
    per layer; final: dict(k, pad, cin) or None (Identity); pools: the aux stages' (kh, kw)."""

    def __init__(self, head, device):
        from torch import nn
        self.device = device
        self.C = cin = head.in_channels
        self.deconvs, self.convs = [], []
        if not isinstance(head.deconv_layers, nn.Identity):
            for dc in list(head.deconv_layers)[::3]:
                self.deconvs.append(dict(k=int(dc.kernel_size[0]), cin=cin, cout=dc.out_channels))
                cin = dc.out_channels
        if not isinstance(head.conv_layers, nn.Identity):
            for cv in list(head.conv_layers)[::3]:
                self.convs.append(dict(k=int(cv.kernel_size[0]), pad=int(cv.padding[0]), cin=cin,
                                       cout=cv.out_channels))
                cin = cv.out_channels
        fl = head.final_layer
        self.final = None if isinstance(fl, nn.Identity) else dict(k=int(fl.kernel_size[0]), pad=int(fl.padding[0]),
                                                                   cin=cin)
        # four aux branches: [conv3x3+BN, pool, relu] x n -> conv1x1 -> act; all four pool alike
        self.pools = []
        for pool in list(head.probability_layers)[2:-2:4]:
            ks = pool.kernel_size
            self.pools.append((int(ks), int(ks)) if isinstance(ks, int) else (int(ks[0]), int(ks[1])))
        self._tables = CaptureCache(8)      # batch sizes vary per frame in inference; captured entries stay
        self.grad_tables = CaptureCache(64)  # the training backward's data-gradient tables (head_train.py)

    # gather/scatter tables depend on (B, h, w) only
    def _tables_for(self, B: int, h: int, w: int) -> dict:
        return self._tables.get((B, h, w), lambda: self._build_tables(B, h, w))

    def _build_tables(self, B: int, h: int, w: int) -> dict:
        dev = self.device
        t = dict(deconv=[], conv=[], aux=[])
        hh, ww = h, w
        for d in self.deconvs:
            ro, rm = pack.deconv_tables(B, hh, ww, d["k"], d["cin"])
            t["deconv"].append((ro.to(dev), rm.to(dev), hh, ww))
            hh, ww = 2 * hh, 2 * ww
        for c in self.convs:
            t["conv"].append(pack.conv_gather_table(B, hh, ww, c["k"], c["k"], c["pad"], c["pad"], c["cin"]).to(dev)
                             if c["k"] > 1 else None)
        f = self.final
        t["final"] = (pack.conv_gather_table(B, hh, ww, f["k"], f["k"], f["pad"], f["pad"], f["cin"]).to(dev)
                      if f is not None and f["k"] > 1 else None)
        t["hm_hw"] = (hh, ww)
        ah, aw = h, w
        for i, p in enumerate(self.pools):
            stride = self.C if i == 0 else 4 * self.C
            t["aux"].append((pack.conv_gather_table(B, ah, aw, 3, 3, 1, 1, stride).to(dev), ah, aw))
            _, _, ah, aw = pack.pool_out(ah, aw, p)
        if (ah, aw) != (1, 1):
            raise ValueError(
                f"alt_head_kernel_sizes {self.pools} reduce a {h}x{w} feature map to {ah}x{aw}; the aux "
                "branches must end at 1x1 (Codec.decode reshapes them to (B,1,K), reference codec.py:254-257)")
        return t


class HeadPlan(HeadGeometry):
    def __init__(self, head, dtype: torch.dtype, device):
        from torch import nn
        super().__init__(head, device)
        self.dtype = dtype
        self.K = head.out_channels
        self.temperature = float(head.temperature)
        # normalize != None: Sparsemax over H*W, * normalize, clamp (head.py:237-245,526-532) as pp_sparsemax_rows on
        # the unclamped logits; the third-party library is not in the reference checkout -> parity unpinned
        self.normalize = None if head.normalize is None else float(head.normalize)
        # --- heatmap branch: deconvs (+BN+ReLU), optional convs (+BN+ReLU), final conv
        layers = [] if isinstance(head.deconv_layers, nn.Identity) else list(head.deconv_layers)
        for d, dc, bn in zip(self.deconvs, layers[::3], layers[1::3]):
            wf, bf = pack.fold_bn(dc.weight.detach().float().cpu(), None, bn.weight.detach().cpu(),
                                  bn.bias.detach().cpu(), bn.running_mean.cpu(), bn.running_var.cpu(),
                                  bn.eps, out_dim=1)
            d.update(w=_dev(pack.pack_deconv_parities(wf, d["k"]), device, dtype), b=_dev(bf, device, torch.float32))
        layers = [] if isinstance(head.conv_layers, nn.Identity) else list(head.conv_layers)
        for c, cv, bn in zip(self.convs, layers[::3], layers[1::3]):
            wf, bf = pack.fold_bn(cv.weight.detach().float().cpu(),
                                  None if cv.bias is None else cv.bias.detach().cpu(),
                                  bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.running_mean.cpu(),
                                  bn.running_var.cpu(), bn.eps)
            c.update(w=_dev(pack.conv_taps_major(wf), device, dtype), b=_dev(bf, device, torch.float32))
        widths = [self.C] + [d["cout"] for d in self.deconvs] + [c["cout"] for c in self.convs]
        if self.final is None:
            # final_layer_kernel_size=None (head.py:234-235): the last conv / deconv layer's (ReLU'd) channels ARE the maps
            if widths[-1] != self.K:
                raise ValueError(f"final_layer_kernel_size=None: the heatmap branch ends with {widths[-1]} channels but "
                                 f"the head has out_channels={self.K} (Codec.decode and the aux branches expect K maps)")
        else:
            fl = head.final_layer
            self.final.update(w=_dev(pack.conv_taps_major(fl.weight.detach().float().cpu()), device, dtype),
                              b=_dev(fl.bias.detach().float(), device, torch.float32))
        # the implicit-GEMM layers walk their input one K-tile (128 bytes of channels) at a time inside a tap: every layer
        # INPUT width of the heatmap branch (and the aux branches' C) must be a whole number of K-tiles
        gran = 64 if dtype == torch.bfloat16 else 32
        consumed = widths[: len(self.deconvs) + len(self.convs) + (1 if self.final is not None else 0)]
        bad = [w for w in consumed if w % gran]
        if bad:
            raise ValueError(f"ProbMapHead on the HIP path ({dtype}): layer input widths {bad} are not multiples of {gran} "
                             f"channels (in_channels / deconv_out_channels / conv_out_channels feeding another layer); "
                             "the reference's own configurations use 256-channel layers")
        # --- four aux branches: [conv3x3+BN, pool, relu] x n -> conv1x1 -> act
        n = len(self.pools)
        C = self.C
        stage_w = [[] for _ in range(n)]
        stage_b = [[] for _ in range(n)]
        tail_w, tail_b = [], []
        for name in AUX_NAMES:
            layers = list(getattr(head, name + "_layers"))
            assert len(layers) == 4 * n + 2
            for i in range(n):
                cv, bn = layers[4 * i], layers[4 * i + 1]
                wf, bf = pack.fold_bn(cv.weight.detach().float().cpu(), cv.bias.detach().cpu(),
                                      bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.running_mean.cpu(),
                                      bn.running_var.cpu(), bn.eps)
                stage_w[i].append(pack.conv_taps_major(wf))
                stage_b[i].append(bf)
            last = layers[4 * n]
            tail_w.append(last.weight.detach().float().cpu().reshape(self.K, C))
            tail_b.append(last.bias.detach().float().cpu())
        # stage 0 shares its input across branches -> one GEMM with N = 4C; later stages batch = 4
        self.aux_w = [_dev(torch.cat(stage_w[0], 0), device, dtype)] + \
                     [_dev(torch.stack(stage_w[i]), device, dtype) for i in range(1, n)]
        self.aux_b = [_dev(torch.cat(stage_b[0], 0), device, torch.float32)] + \
                     [_dev(torch.stack(stage_b[i]), device, torch.float32) for i in range(1, n)]
        self.tail_w = _dev(torch.stack(tail_w), device, dtype)
        self.tail_b = _dev(torch.stack(tail_b), device, torch.float32)
        self.ws = _Workspace()
        self._aux_stream = None

    def forward(self, feats: torch.Tensor, B: int, h: int, w: int):
        """feats: channels-last rows [B*h*w, C] in the compute dtype.
        Returns (heatmaps (B,K,Hh,Wh) f32, prob, vis, oks, err (B,K,1,1) f32)."""
        with torch.cuda.device(self.device):      # kernels launch on the current stream of the plan's device
            return self._forward(feats, B, h, w)

    def _forward(self, feats: torch.Tensor, B: int, h: int, w: int):
        dev, K = self.device, self.K
        tb = self._tables_for(B, h, w)
        # ---- aux branches on a second HIP stream: after their first conv they are long-K GEMMs over a
        # few rows (M = B*16, B*4) that cannot fill 256 CUs; the independent deconvolution branch fills
        # the idle CUs meanwhile.  Fork/join by events, so the pair is graph-capturable.
        if self._aux_stream is None:
            self._aux_stream = torch.cuda.Stream(device=dev)
        aux = torch.empty((4, B, K), dtype=torch.float32, device=dev)
        heat = torch.empty((B, K, h * 2 ** len(self.deconvs), w * 2 ** len(self.deconvs)), dtype=torch.float32,
                           device=dev)
        aux_stream = torch.cuda.current_stream(dev) if SERIALIZE_HEAD else self._aux_stream
        aux_stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(aux_stream):
            self._aux_branch(feats, B, h, w, tb, aux)
        self._heatmap_branch(feats, B, h, w, tb, heat)
        # ---- join the aux-branch stream (forked above)
        torch.cuda.current_stream(dev).wait_stream(aux_stream)
        return (heat, *(aux[i].reshape(B, K, 1, 1) for i in range(4)))

    def _aux_branch(self, feats, B, h, w, tb, aux):
        dev, dt, C = self.device, self.dtype, self.C
        g = self.ws.get
        a, ah, aw = feats, h, w
        for i, (p, (ro, _, _)) in enumerate(zip(self.pools, tb["aux"])):
            M = B * ah * aw
            kh, kw, oh, ow = pack.pool_out(ah, aw, p)
            pooled = g(f"aux_pool{i}", (B * oh * ow, 4 * C), dt, dev)
            split = head_calls.aux_split(i) if i > 0 and SPLITK_AUX else 1
            if split > 1:
                # rows leading ([split * M, 4C], partial s = rows [s * M, (s + 1) * M)): the workspace key does
                # not hold M, so one allocation serves every batch size up to the largest seen
                parts = g(f"aux_part{i}", (split * M, 4 * C), torch.float32, dev).view(split, M, 4 * C)
                ops.gemm(a, self.aux_w[i], parts, **head_calls.aux_stage(M, C, split=split), rowoff=ro,
                         epilogue=EPI_OUT_F32)
                ops.maxpool_relu_sum(parts, self.aux_b[i].reshape(-1), pooled, B, ah, aw, 4 * C, kh, kw)
            else:
                conv = g(f"aux_conv{i}", (M, 4 * C), dt, dev)
                call = head_calls.aux_stage0(M, C) if i == 0 else head_calls.aux_stage(M, C)
                ops.gemm(a, self.aux_w[i], conv, **call, bias=self.aux_b[i], rowoff=ro)
                ops.maxpool_relu(conv, pooled, B, ah, aw, 4 * C, kh, kw)
            a, ah, aw = pooled, oh, ow
        ops.aux_tail(a, self.tail_w, self.tail_b, aux, B, C, self.K)

    def _heatmap_branch(self, feats, B, h, w, tb, heat):
        dev, dt, K = self.device, self.dtype, self.K
        g = self.ws.get
        x, hh, ww, cin = feats, h, w, self.C
        f = self.final
        clamp = self.normalize is None
        fused_final = final_done = False
        for li, (d, (ro, rm, _, _)) in enumerate(zip(self.deconvs, tb["deconv"])):
            M = B * hh * ww
            ends = li == len(self.deconvs) - 1 and not self.convs
            if (FUSE_FINAL and ends and f is not None and dt == torch.bfloat16 and d["cout"] == 256 and f["k"] == 1
                    and K <= 32):
                # the last deconvolution's epilogue applies the final 1x1 layer itself: its 256-channel output
                # (100 MB at bs 64) is never stored, and the final-layer launch is gone
                out, fused_final = heat, True
                tail = dict(fuse_final=(f["w"], f["b"], K, 4 * hh * ww, self.temperature, clamp))
            elif f is None and ends:
                # Identity final layer: this layer's ReLU'd outputs are the maps -> /T, clamp, NCHW store in its epilogue
                out, final_done = heat, True
                tail = dict(heatmap=(K, 4 * hh * ww, self.temperature, clamp))
            else:
                out, tail = g(f"deconv{li}", (4 * M, d["cout"]), dt, dev), {}
            ops.gemm(x, d["w"], out, **head_calls.deconv(M, cin, d["cout"]), bias=d["b"], rowoff=ro, out_rowmap=rm,
                     epilogue=EPI_RELU, **tail)
            x, hh, ww, cin = out, 2 * hh, 2 * ww, d["cout"]
        for li, (c, ro) in enumerate(zip(self.convs, tb["conv"])):
            M = B * hh * ww
            if f is None and li == len(self.convs) - 1:
                out, final_done = heat, True
                tail = dict(heatmap=(K, hh * ww, self.temperature, clamp))
            else:
                out, tail = g(f"conv{li}", (M, c["cout"]), dt, dev), {}
            ops.gemm(x, c["w"], out, **head_calls.conv(M, cin, c["cout"], c["k"]), bias=c["b"], rowoff=ro,
                     epilogue=EPI_RELU, **tail)
            x, cin = out, c["cout"]
        assert heat.shape == (B, K, hh, ww)
        if f is None and not final_done:
            # no deconv, no conv, no final layer: the maps are the input features themselves (degenerate but constructible)
            nchw = torch.empty((B, K, hh, ww), dtype=torch.float32, device=dev)
            ops.tokens_to_nchw(x, nchw, B, hh * ww, K)
            heat.copy_(nchw / self.temperature)
            if clamp:
                heat.clamp_(0, 1)
        if fused_final or f is None:
            pass
        elif f["k"] == 1 and final_heatmap_fits(cin, K, dt):
            ops.final_heatmap(x, f["w"], f["b"], heat, B, hh * ww, cin, K, self.temperature, clamp=clamp)
        else:
            ops.gemm(x, f["w"], heat, **head_calls.conv(B * hh * ww, cin, K, f["k"]), bias=f["b"], rowoff=tb["final"],
                     heatmap=(K, hh * ww, self.temperature, clamp))
        if not clamp:
            ops.sparsemax_rows(heat.view(B * K, hh * ww), self.normalize)


def build_head_plan(head, dtype, device):
    return HeadPlan(head, dtype, device)
