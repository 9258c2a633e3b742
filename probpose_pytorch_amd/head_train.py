"""Training ProbMapHead on the HIP path (``ProbMapHead(differentiable=True)`` in ``.train()`` mode).

The forward does what the reference head does in train mode (head.py:487-594): every BatchNorm normalises with the
batch mean and biased variance and updates its running statistics; the (de)convolutions write their pre-BN outputs in
f32 and keep them for the backward.  One once-differentiable ``torch.autograd.Function`` per head call; its backward
launches only what the trainable parameters and ``x.requires_grad`` need, reads the upstream gradients on the device
and does no host sync.  The weights are packed from the parameters on the device at every call (no host copy, no
rebuild of the eval ``HeadPlan``); the gather / scatter tables are ``engine.HeadGeometry``'s, as in eval.
"""
from __future__ import annotations

import weakref
from typing import Dict, List

import torch
from torch import nn

from . import _lib, engine, ops, pack
from .ops import EPI_OUT_F32

AUX_NAMES = engine.AUX_NAMES
KTILE = 64         # the heatmap gradient's channel pitch is a whole number of pp_gemm K-tiles in both compute dtypes


def check_trainable(head) -> None:
    """Raise NotImplementedError naming the piece of ``head`` the training path does not cover."""
    if head.compute_dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"ProbMapHead training: compute dtype {head.compute_dtype} (float32 and bfloat16 "
                                  "are supported)")
    if not isinstance(head.conv_layers, nn.Identity):
        raise NotImplementedError("ProbMapHead training: conv_out_channels (a conv stack after the deconvolutions)")
    if isinstance(head.deconv_layers, nn.Identity):
        raise NotImplementedError("ProbMapHead training: deconv_out_channels=() (no deconvolution layers)")
    for m in head.deconv_layers:
        if isinstance(m, nn.ConvTranspose2d) and int(m.kernel_size[0]) != 4:
            raise NotImplementedError(f"ProbMapHead training: deconvolution kernel {int(m.kernel_size[0])} "
                                      "(kernel 4 is supported)")
    if isinstance(head.final_layer, nn.Identity):
        raise NotImplementedError("ProbMapHead training: final_layer_kernel_size=None")
    if int(head.final_layer.kernel_size[0]) != 1:
        raise NotImplementedError(f"ProbMapHead training: final_layer_kernel_size={int(head.final_layer.kernel_size[0])} "
                                  "(1 is supported)")
    for m in head.modules():
        if isinstance(m, nn.BatchNorm2d) and m.track_running_stats and m.momentum is None:
            raise NotImplementedError("ProbMapHead training: BatchNorm2d(momentum=None) (cumulative moving average)")


def head_parameters(head) -> List[nn.Parameter]:
    """The head's parameters in the order the autograd node takes them."""
    ps = []
    layers = list(head.deconv_layers)
    for i in range(0, len(layers), 3):
        ps += [layers[i].weight, layers[i + 1].weight, layers[i + 1].bias]
    ps += [head.final_layer.weight, head.final_layer.bias]
    for name in AUX_NAMES:
        ps += list(getattr(head, name + "_layers").parameters())
    return ps


class _Geometry(engine.HeadGeometry):
    """The head's layer dimensions and tables, plus what only the backward reads: the deconvolution's parity index and
    a cache of its data-gradient tables."""

    def __init__(self, head, device):
        super().__init__(head, device)
        self._extra: Dict[tuple, object] = {}
        self.KY, self.KX = (t.to(device) for t in pack.deconv_parity_index(4))

    def extra(self, key, make):
        t = self._extra.get(key)
        if t is None:
            if len(self._extra) >= 64:
                self._extra.pop(next(iter(self._extra)))
            t = self._extra[key] = make()
        return t


_GEOM: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _geometry(head, device) -> _Geometry:
    g = _GEOM.get(head)
    if g is None or g.device != device:
        g = _GEOM[head] = _Geometry(head, device)
    return g


def _bn_stats(bn, y, M, Cc, gammas, betas, rms, rvs):
    """Batch statistics of y [M, Cc] for one BN (or four concatenated aux BNs); updates the running statistics."""
    if M <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {M} per channel")
    dev = y.device
    st = torch.empty((4, Cc), dtype=torch.float32, device=dev)
    ws = torch.empty(ops.bn_workspace_bytes(M, Cc), dtype=torch.uint8, device=dev)
    cat = (lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)) if gammas else None
    gamma = cat([g.detach() for g in gammas]) if gammas[0] is not None else None
    beta = cat([b.detach() for b in betas]) if betas[0] is not None else None
    track = rms[0] is not None
    rm = cat(rms) if track else None
    rv = cat(rvs) if track else None
    ops.bn_train_stats(y, M, Cc, gamma, beta, bn.eps, bn.momentum if track else 0.0, rm, rv, st[0], st[1], st[2],
                       st[3], ws)
    if track:
        if len(rms) > 1:
            n = Cc // len(rms)
            for i, (a, b) in enumerate(zip(rms, rvs)):
                a.copy_(rm[i * n:(i + 1) * n])
                b.copy_(rv[i * n:(i + 1) * n])
    return st, gamma


def _bump(bns):
    for bn in bns:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)


def _wgrad(dY, A, dW, **kw):
    n = ops.wgrad_workspace_floats(kw["M"], kw["N"], kw["Kd"], kw.get("batch", 1))
    parts = torch.empty(n, dtype=torch.float32, device=dY.device) if n else None
    ops.wgrad(dY, A, dW, parts=parts, **kw)


def _runs(flags):
    """Maximal runs [b0, b1) of True in flags."""
    out, b0 = [], None
    for i, f in enumerate(list(flags) + [False]):
        if f and b0 is None:
            b0 = i
        elif not f and b0 is not None:
            out.append((b0, i))
            b0 = None
    return out


class _HeadTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, x, is_nchw, geom, *params):
        dt = head.compute_dtype
        dev = x.device
        B, C, h, w = geom
        if is_nchw:
            tokens = torch.empty((B * h * w, C), dtype=dt, device=dev)
            ops.nchw_to_tokens(x.detach().contiguous().float(), tokens, B, C, h * w)
        else:
            tokens = x
        geo = _geometry(head, dev)
        tb = geo._tables_for(B, h, w)
        K = head.out_channels
        S = ctx.saved = dict(B=B, h=h, w=w, tokens=tokens, nchw=is_nchw)
        # ---- heatmap branch: deconv -> train BN -> ReLU, final 1x1, /T, (Sparsemax, * normalize), clamp
        layers = list(head.deconv_layers)
        xin, dec = tokens, []
        for li, (d, (ro, rm, hh, ww)) in enumerate(zip(geo.deconvs, tb["deconv"])):
            dc, bn = layers[3 * li], layers[3 * li + 1]
            cin, cout = d["cin"], d["cout"]
            M = B * hh * ww
            wp = dc.weight.detach().permute(1, 2, 3, 0)[:, geo.KY, geo.KX, :].permute(1, 0, 2, 3)
            wp = wp.reshape(4, cout, 4 * cin).to(dt).contiguous()
            y = torch.empty((4 * M, cout), dtype=torch.float32, device=dev)
            ops.gemm(xin, wp, y, M=M, N=cout, Kd=4 * cin, lda=cin, ldw=4 * cin, ldc=cout, rowoff=ro, seg_len=cin,
                     out_rowmap=rm, batch=4, strideW=cout * 4 * cin, strideRowoff=4 * M, strideRowmap=M,
                     epilogue=EPI_OUT_F32)
            st, gamma = _bn_stats(bn, y, 4 * M, cout, [bn.weight], [bn.bias], [bn.running_mean], [bn.running_var])
            xo = torch.empty((4 * M, cout), dtype=dt, device=dev)
            ops.bn_apply_relu(y, 4 * M, cout, st[2], st[3], xo)
            dec.append(dict(x=xin, y=y, st=st, gamma=gamma, ro=ro, rm=rm, hh=hh, ww=ww, cin=cin, cout=cout))
            xin = xo
        _bump([layers[3 * li + 1] for li in range(len(geo.deconvs))])
        HH, WW = tb["hm_hw"]
        HW = HH * WW
        cin = geo.final["cin"]
        fw = head.final_layer.weight.detach().reshape(K, cin).to(dt).contiguous()
        fb = head.final_layer.bias.detach().float().contiguous()
        v = torch.empty((B, K, HH, WW), dtype=torch.float32, device=dev)
        T = float(head.temperature)
        if engine.final_heatmap_fits(cin, K, dt):
            ops.final_heatmap(xin, fw, fb, v, B, HW, cin, K, T, clamp=False)
        else:
            ops.gemm(xin, fw, v, M=B * HW, N=K, Kd=cin, lda=cin, ldw=cin, ldc=K, bias=fb, heatmap=(K, HW, T, False))
        scale = 1.0 if head.normalize is None else float(head.normalize)
        if head.normalize is not None:
            ops.sparsemax_rows(v.view(B * K, HW), 1.0)       # v <- Sparsemax(logits / T), kept for the backward
        heat = ops.heat_clamp(v, torch.empty_like(v), scale)
        S.update(dec=dec, feat=xin, p=v, HW=HW, HH=HH, WW=WW, scale=scale, fw=fw)
        # ---- aux branches: [conv3x3 -> train BN -> MaxPool -> ReLU] x n -> conv1x1 -> Sigmoid / ReLU
        seqs = [list(getattr(head, n + "_layers")) for n in AUX_NAMES]
        a, ah, aw = tokens, h, w
        aux_st = []
        for i, (p, (ro, _, _)) in enumerate(zip(geo.pools, tb["aux"])):
            M = B * ah * aw
            convs = [s[4 * i] for s in seqs]
            bns = [s[4 * i + 1] for s in seqs]
            y = torch.empty((M, 4 * C), dtype=torch.float32, device=dev)
            if i == 0:
                w0 = torch.cat([pack.conv_taps_major(cv.weight.detach()) for cv in convs]).to(dt).contiguous()
                b0 = torch.cat([cv.bias.detach() for cv in convs]).float().contiguous()
                ops.gemm(a, w0, y, M=M, N=4 * C, Kd=9 * C, lda=C, ldw=9 * C, ldc=4 * C, bias=b0, rowoff=ro, seg_len=C,
                         epilogue=EPI_OUT_F32)
            else:
                wi = torch.stack([pack.conv_taps_major(cv.weight.detach()) for cv in convs]).to(dt).contiguous()
                bi = torch.stack([cv.bias.detach() for cv in convs]).float().contiguous()
                ops.gemm(a, wi, y, M=M, N=C, Kd=9 * C, lda=4 * C, ldw=9 * C, ldc=4 * C, bias=bi, rowoff=ro,
                         seg_len=C, batch=4, strideA=C, strideW=C * 9 * C, strideC=C, strideBias=C,
                         epilogue=EPI_OUT_F32)
            st, gamma = _bn_stats(bns[0], y, M, 4 * C, [b.weight for b in bns], [b.bias for b in bns],
                                  [b.running_mean for b in bns], [b.running_var for b in bns])
            _bump(bns)
            kh, kw, oh, ow = pack.pool_out(ah, aw, p)
            pooled = torch.empty((B * oh * ow, 4 * C), dtype=dt, device=dev)
            argmax = torch.empty((B * oh * ow, 4 * C), dtype=torch.int32, device=dev)
            ops.bn_pool_relu(y, B, ah, aw, 4 * C, kh, kw, st[2], st[3], pooled, argmax)
            aux_st.append(dict(x=a, y=y, st=st, gamma=gamma, ro=ro, ah=ah, aw=aw, kh=kh, kw=kw, argmax=argmax))
            a, ah, aw = pooled, oh, ow
        tw = torch.stack([s[-2].weight.detach().reshape(K, C) for s in seqs]).to(dt).contiguous()
        tbias = torch.stack([s[-2].bias.detach() for s in seqs]).float().contiguous()
        aux = torch.empty((4, B, K), dtype=torch.float32, device=dev)
        ops.aux_tail(a, tw, tbias, aux, B, C, K)
        S.update(aux=aux_st, pooled=a, tw=tw, aux_out=aux)
        ctx.head = head
        ctx.set_materialize_grads(False)
        outs = [heat] + [aux[i].reshape(B, K, 1, 1).clone() for i in range(4)]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_heat, g_prob, g_vis, g_oks, g_err):
        head, S = ctx.head, ctx.saved
        need = ctx.needs_input_grad
        params = head_parameters(head)
        pidx = {id(p): i for i, p in enumerate(params)}
        grads = [None] * len(params)
        x_needs = need[1]          # NCHW x, or channels-last tokens that carry a gradient (a training backbone)

        def wants(p):
            return p is not None and need[4 + pidx[id(p)]]

        def put(p, g):
            if wants(p):
                grads[pidx[id(p)]] = g.reshape(p.shape).to(p.dtype)

        dt = head.compute_dtype
        B, h, w = S["B"], S["h"], S["w"]
        C, K = head.in_channels, head.out_channels
        dev = S["tokens"].device
        geo = _geometry(head, dev)
        layers = list(head.deconv_layers)
        gtok = None
        # ---- heatmap branch
        dec = S["dec"]
        dec_need = [any(wants(p) for p in (layers[3 * i].weight, layers[3 * i + 1].weight, layers[3 * i + 1].bias))
                    for i in range(len(dec))]
        below = [x_needs or any(dec_need[:i]) for i in range(len(dec) + 1)]     # below[i]: layer i's input needs grad
        fl = head.final_layer
        if g_heat is not None and (wants(fl.weight) or wants(fl.bias) or below[len(dec)]):
            HW, M = S["HW"], B * S["HW"]
            KPAD = -(-K // KTILE) * KTILE
            dz = torch.empty((M, KPAD), dtype=dt, device=dev)
            ops.heat_tail_backward(S["p"], g_heat.contiguous().float(), B, K, HW, S["scale"],
                                   head.normalize is not None, float(head.temperature), dz)
            feat, cin = S["feat"], geo.final["cin"]
            if wants(fl.weight) or wants(fl.bias):
                dWf = torch.empty((K, cin), dtype=torch.float32, device=dev)
                dbf = torch.empty((K,), dtype=torch.float32, device=dev)
                _wgrad(dz, feat, dWf, M=M, N=K, Kd=cin, ldd=KPAD, lda=cin, dB=dbf)
                put(fl.weight, dWf)
                put(fl.bias, dbf)
            if below[len(dec)]:
                wt = torch.zeros((cin, KPAD), dtype=dt, device=dev)
                wt[:, :K] = S["fw"].t()
                gf = torch.empty((M, cin), dtype=torch.float32, device=dev)
                ops.gemm(dz, wt, gf, M=M, N=cin, Kd=KPAD, lda=KPAD, ldw=KPAD, ldc=cin, epilogue=EPI_OUT_F32)
                for li in range(len(dec) - 1, -1, -1):
                    d = dec[li]
                    dc, bn = layers[3 * li], layers[3 * li + 1]
                    M = B * d["hh"] * d["ww"]
                    cin, cout = d["cin"], d["cout"]
                    dY = torch.empty((4 * M, cout), dtype=dt, device=dev)
                    dgb = torch.empty((2, cout), dtype=torch.float32, device=dev)
                    ws = torch.empty(ops.bn_workspace_bytes(4 * M, cout), dtype=torch.uint8, device=dev)
                    st = d["st"]
                    ops.bn_train_backward(gf, d["y"], 4 * M, cout, st[0], st[1], d["gamma"], dY, ws, mode=1,
                                          scale=st[2], shift=st[3], dgamma=dgb[0], dbeta=dgb[1])
                    put(bn.weight, dgb[0])
                    put(bn.bias, dgb[1])
                    if wants(dc.weight):
                        dwp = torch.empty((4, cout, 4 * cin), dtype=torch.float32, device=dev)
                        _wgrad(dY, d["x"], dwp, M=M, N=cout, Kd=4 * cin, ldd=cout, rowoff=d["ro"], seg_len=cin,
                               dy_rowmap=d["rm"], batch=4, strideRowoff=4 * M, strideRowmap=M,
                               strideDW=cout * 4 * cin)
                        dw = torch.empty((cout, 4, 4, cin), dtype=torch.float32, device=dev)
                        dw[:, geo.KY, geo.KX, :] = dwp.view(4, cout, 4, cin).permute(1, 0, 2, 3)
                        put(dc.weight, dw.permute(3, 0, 1, 2))
                    if not below[li]:
                        break
                    tab = geo.extra(("dgrad", B, d["hh"], d["ww"], cout),
                                    lambda: pack.deconv_data_grad_table(B, d["hh"], d["ww"], 4, cout).to(dev))
                    wt = pack.deconv_data_grad_weights(dc.weight.detach()).to(dt).contiguous()
                    gf = torch.empty((M, cin), dtype=torch.float32, device=dev)
                    ops.gemm(dY, wt, gf, M=M, N=cin, Kd=16 * cout, lda=cout, ldw=16 * cout, ldc=cin, rowoff=tab,
                             seg_len=cout, epilogue=EPI_OUT_F32)
                if x_needs:
                    gtok = gf
        # ---- aux branches
        seqs = [list(getattr(head, n + "_layers")) for n in AUX_NAMES]
        gs = (g_prob, g_vis, g_oks, g_err)
        into_x = [x_needs and not head.detach_probability, x_needs and not head.detach_visibility, False, False]
        aux = S["aux"]
        n = len(aux)
        stage_need = [[any(wants(p) for p in (s[4 * i].weight, s[4 * i].bias, s[4 * i + 1].weight,
                                              s[4 * i + 1].bias)) for s in seqs] for i in range(n)]
        tail_need = [wants(s[-2].weight) or wants(s[-2].bias) for s in seqs]
        abelow = [any(any(stage_need[j]) for j in range(i)) or (any(into_x) and i >= 0) for i in range(n + 1)]
        if any(g is not None for g in gs) and (any(tail_need) or abelow[n]):
            gaux = torch.stack([g.reshape(B, K).float() if g is not None else
                                torch.zeros((B, K), dtype=torch.float32, device=dev) for g in gs]).contiguous()
            dWt = torch.empty((4, K, C), dtype=torch.float32, device=dev) if any(tail_need) else None
            dbt = torch.empty((4, K), dtype=torch.float32, device=dev) if any(tail_need) else None
            dpool = torch.empty((B, 4 * C), dtype=torch.float32, device=dev) if abelow[n] else None
            ops.aux_tail_backward(S["pooled"], S["tw"], S["aux_out"], gaux, B, C, K, dWt, dbt, dpool)
            for bi, s in enumerate(seqs):
                if tail_need[bi]:
                    put(s[-2].weight, dWt[bi])
                    put(s[-2].bias, dbt[bi])
            for i in range(n - 1, -1, -1):
                if not abelow[i + 1]:
                    break
                a = aux[i]
                M = B * a["ah"] * a["aw"]
                st = a["st"]
                dY = torch.empty((M, 4 * C), dtype=dt, device=dev)
                dgb = torch.empty((2, 4 * C), dtype=torch.float32, device=dev)
                ws = torch.empty(ops.bn_workspace_bytes(M, 4 * C), dtype=torch.uint8, device=dev)
                ops.bn_train_backward(dpool, a["y"], M, 4 * C, st[0], st[1], a["gamma"], dY, ws, mode=2,
                                      argmax=a["argmax"], pool=(B, a["ah"], a["aw"], a["kh"], a["kw"]),
                                      dgamma=dgb[0], dbeta=dgb[1])
                dW = torch.empty((4, C, 9 * C), dtype=torch.float32, device=dev)
                dB = torch.empty((4, C), dtype=torch.float32, device=dev)
                wneed = [wants(s[4 * i].weight) or wants(s[4 * i].bias) for s in seqs]
                for b0, b1 in _runs(wneed):
                    if i == 0:
                        _wgrad(dY[:, b0 * C:], a["x"], dW[b0:b1].view(-1, 9 * C), M=M, N=(b1 - b0) * C, Kd=9 * C,
                               ldd=4 * C, rowoff=a["ro"], seg_len=C, dB=dB[b0:b1].view(-1))
                    else:
                        _wgrad(dY[:, b0 * C:], a["x"][:, b0 * C:], dW[b0:b1], M=M, N=C, Kd=9 * C, ldd=4 * C,
                               rowoff=a["ro"], seg_len=C, batch=b1 - b0, strideDY=C, strideA=C, strideDW=C * 9 * C,
                               dB=dB[b0:b1], strideDB=C)
                for bi, s in enumerate(seqs):
                    cv, bn = s[4 * i], s[4 * i + 1]
                    if wneed[bi]:
                        put(cv.weight, dW[bi].view(C, 3, 3, C).permute(0, 3, 1, 2))
                        put(cv.bias, dB[bi])
                    put(bn.weight, dgb[0, bi * C:(bi + 1) * C])
                    put(bn.bias, dgb[1, bi * C:(bi + 1) * C])
                if i > 0 and abelow[i]:
                    wt = torch.stack([pack.conv3x3_data_grad_weights(s[4 * i].weight.detach()) for s in seqs])
                    wt = wt.to(dt).contiguous()
                    dpool = torch.empty((M, 4 * C), dtype=torch.float32, device=dev)
                    ops.gemm(dY, wt, dpool, M=M, N=C, Kd=9 * C, lda=4 * C, ldw=9 * C, ldc=4 * C, rowoff=a["ro"],
                             seg_len=C, batch=4, strideA=C, strideW=C * 9 * C, strideC=C, epilogue=EPI_OUT_F32)
                elif i == 0 and any(into_x):
                    brs = [bi for bi in range(4) if into_x[bi]]
                    tab = geo.extra(("aux0", B, h, w, tuple(brs)), lambda: _aux0_dgrad_table(B, h, w, C, brs, dev))
                    wt = torch.stack([pack.conv3x3_data_grad_weights(seqs[bi][0].weight.detach()).view(C, 9, C)
                                      for bi in brs], dim=2).reshape(C, 9 * len(brs) * C).to(dt).contiguous()
                    if gtok is None:
                        gtok = torch.empty((M, C), dtype=torch.float32, device=dev)
                        ops.gemm(dY, wt, gtok, M=M, N=C, Kd=9 * len(brs) * C, lda=4 * C, ldw=9 * len(brs) * C,
                                 ldc=C, rowoff=tab, seg_len=C, epilogue=EPI_OUT_F32)
                    else:
                        ops.gemm(dY, wt, gtok, M=M, N=C, Kd=9 * len(brs) * C, lda=4 * C, ldw=9 * len(brs) * C,
                                 ldc=C, rowoff=tab, seg_len=C, residual=gtok, epilogue=EPI_OUT_F32)
        gx = None
        if x_needs and not S["nchw"]:
            # the token gradient as it is, f32 [B*h*w, C] (autograd casts it to the tokens' dtype)
            gx = gtok if gtok is not None else torch.zeros((B * h * w, C), dtype=torch.float32, device=dev)
        elif x_needs:
            if gtok is None:
                gx = torch.zeros((B, C, h, w), dtype=torch.float32, device=dev)
            else:
                gx = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
                ops.tokens_to_nchw(gtok, gx, B, h * w, C)
        return (None, gx, None, None, *grads)


def _aux0_dgrad_table(B, h, w, C, brs, dev):
    """Rows (tap, branch) of the first aux stage's data gradient: dY [M, 4C] gathered at the flipped 3x3 taps, the
    branch's C columns."""
    base = pack.conv_gather_table(B, h, w, 3, 3, 1, 1, 4 * C)
    segs = []
    for t in range(9):
        for bi in brs:
            segs.append(torch.where(base[t] >= 0, base[t] + bi * C, base[t]))
    return torch.stack(segs).contiguous().to(dev)


def train_forward(head, x: torch.Tensor = None, tokens: torch.Tensor = None, geom=None):
    """The train-mode forward of ``head``: from an NCHW feature map ``x`` or from channels-last ``tokens`` [B*h*w, C]
    in the compute dtype, geom = (B, h, w); the gradient reaches either when it requires grad."""
    check_trainable(head)
    params = head_parameters(head)
    if x is not None:
        _lib.require_device(x)
        B, C, h, w = x.shape
        if C != head.in_channels:
            raise ValueError(f"ProbMapHead: expected {head.in_channels} channels, got {C}")
        inp, is_nchw, shape = x, True, (B, C, h, w)
        dev = x.device
    else:
        _lib.require_device(tokens)
        B, h, w = geom
        if tokens.dtype != head.compute_dtype:
            raise TypeError(f"tokens are {tokens.dtype}, the head computes in {head.compute_dtype}")
        inp = tokens if tokens.requires_grad else tokens.detach()
        is_nchw, shape = False, (B, head.in_channels, h, w)
        dev = tokens.device
    for p in params:
        if p.device != dev:
            raise ValueError(f"ProbMapHead parameters are on {p.device}, the input on {dev}: move the head first")
    with torch.cuda.device(dev):
        return _HeadTrainFn.apply(head, inp, is_nchw, shape, *params)
