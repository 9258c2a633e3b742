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
from typing import List

import torch
from torch import nn

from . import _lib, engine, head_calls, ops, pack
from .head_calls import KTILE  # noqa: F401  (the heatmap gradient's channel pitch; tests read it here)
from .ops import EPI_OUT_F32


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
    for name in engine.AUX_NAMES:
        ps += list(getattr(head, name + "_layers").parameters())
    return ps


_GEOM: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _geometry(head, device) -> engine.HeadGeometry:
    g = _GEOM.get(head)
    if g is None or g.device != device:
        g = _GEOM[head] = engine.HeadGeometry(head, device)
    return g


def _bn_stats(bn, y, M, Cc, gammas, betas, rms, rvs):
    """Batch statistics of y [M, Cc] for one BN (or four concatenated aux BNs); updates the running statistics."""
    if M <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {M} per channel")
    dev = y.device
    st = torch.empty((4, Cc), dtype=torch.float32, device=dev)
    ws = torch.empty(ops.bn_workspace_bytes(M, Cc), dtype=torch.uint8, device=dev)

    def cat(ts):
        return ts[0] if len(ts) == 1 else torch.cat(ts)

    gamma = cat([g.detach() for g in gammas]) if gammas[0] is not None else None
    beta = cat([b.detach() for b in betas]) if betas[0] is not None else None
    track = rms[0] is not None
    rm = cat(rms) if track else None
    rv = cat(rvs) if track else None
    ops.bn_train_stats(y, M, Cc, gamma, beta, bn.eps, bn.momentum if track else 0.0, rm, rv, st[0], st[1], st[2],
                       st[3], ws)
    if track and len(rms) > 1:
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
            wp = pack.pack_deconv_parities(dc.weight.detach(), 4).to(dt).contiguous()
            y = torch.empty((4 * M, cout), dtype=torch.float32, device=dev)
            ops.gemm(xin, wp, y, **head_calls.deconv(M, cin, cout), rowoff=ro, out_rowmap=rm, epilogue=EPI_OUT_F32)
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
            ops.gemm(xin, fw, v, **head_calls.conv(B * HW, cin, K, 1), bias=fb, heatmap=(K, HW, T, False))
        scale = 1.0 if head.normalize is None else float(head.normalize)
        if head.normalize is not None:
            ops.sparsemax_rows(v.view(B * K, HW), 1.0)       # v <- Sparsemax(logits / T), kept for the backward
        heat = ops.heat_clamp(v, torch.empty_like(v), scale)
        S.update(dec=dec, feat=xin, p=v, HW=HW, HH=HH, WW=WW, scale=scale, fw=fw)
        # ---- aux branches: [conv3x3 -> train BN -> MaxPool -> ReLU] x n -> conv1x1 -> Sigmoid / ReLU
        seqs = [list(getattr(head, n + "_layers")) for n in engine.AUX_NAMES]
        a, ah, aw = tokens, h, w
        aux_st = []
        for i, (p, (ro, _, _)) in enumerate(zip(geo.pools, tb["aux"])):
            M = B * ah * aw
            convs = [s[4 * i] for s in seqs]
            bns = [s[4 * i + 1] for s in seqs]
            y = torch.empty((M, 4 * C), dtype=torch.float32, device=dev)
            # stage 0 shares its input: the branches' weights one under the other; later stages: batch entries
            join, call = (torch.cat, head_calls.aux_stage0) if i == 0 else (torch.stack, head_calls.aux_stage)
            wi = join([pack.conv_taps_major(cv.weight.detach()) for cv in convs]).to(dt).contiguous()
            bi = join([cv.bias.detach() for cv in convs]).float().contiguous()
            ops.gemm(a, wi, y, **call(M, C), bias=bi, rowoff=ro, epilogue=EPI_OUT_F32)
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
        return (heat, *(aux[i].reshape(B, K, 1, 1).clone() for i in range(4)))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_heat, g_prob, g_vis, g_oks, g_err):
        head, S = ctx.head, ctx.saved
        need = ctx.needs_input_grad
        params = head_parameters(head)
        pidx = {id(p): i for i, p in enumerate(params)}
        grads = [None] * len(params)
        x_needs = need[1]          # NCHW x, or channels-last tokens that carry a gradient (a training backbone)
        dt, f32, dev = head.compute_dtype, torch.float32, S["tokens"].device
        B, h, w, C, K = S["B"], S["h"], S["w"], head.in_channels, head.out_channels
        geo = _geometry(head, dev)

        def wants(*ps):
            return any(p is not None and need[4 + pidx[id(p)]] for p in ps)

        def put(p, g):
            if wants(p):
                grads[pidx[id(p)]] = g.reshape(p.shape).to(p.dtype)

        def bn_backward(g, s, M, Cc, bns, **mode):
            """dY (compute dtype) of a train-mode BN under the gradient g of what follows it; puts the BNs' gradients."""
            dY = torch.empty((M, Cc), dtype=dt, device=dev)
            dgb = torch.empty((2, Cc), dtype=f32, device=dev)
            ws = torch.empty(ops.bn_workspace_bytes(M, Cc), dtype=torch.uint8, device=dev)
            st = s["st"]
            ops.bn_train_backward(g, s["y"], M, Cc, st[0], st[1], s["gamma"], dY, ws, dgamma=dgb[0], dbeta=dgb[1], **mode)
            n = Cc // len(bns)
            for bi, bn in enumerate(bns):
                put(bn.weight, dgb[0, bi * n:(bi + 1) * n])
                put(bn.bias, dgb[1, bi * n:(bi + 1) * n])
            return dY

        def heatmap_backward():
            """The heatmap branch, final layer down to the tokens: their f32 gradient [B*h*w, C], or None when x needs
            none (or no heatmap gradient came in)."""
            layers = list(head.deconv_layers)
            dec = S["dec"]
            n = len(dec)
            dec_need = [wants(layers[3 * i].weight, layers[3 * i + 1].weight, layers[3 * i + 1].bias) for i in range(n)]
            below = [x_needs or any(dec_need[:i]) for i in range(n + 1)]     # below[i]: layer i's input needs grad
            fl = head.final_layer
            if g_heat is None or not (wants(fl.weight, fl.bias) or below[n]):
                return None
            HW, M = S["HW"], B * S["HW"]
            cin = geo.final["cin"]
            KPAD = head_calls.kpad(K)
            dz = torch.empty((M, KPAD), dtype=dt, device=dev)
            ops.heat_tail_backward(S["p"], g_heat.contiguous().float(), B, K, HW, S["scale"],
                                   head.normalize is not None, float(head.temperature), dz)
            if wants(fl.weight, fl.bias):
                dWf = torch.empty((K, cin), dtype=f32, device=dev)
                dbf = torch.empty((K,), dtype=f32, device=dev)
                _wgrad(dz, S["feat"], dWf, **dict(head_calls.wgrad_of(head_calls.conv(M, cin, K, 1)), ldd=KPAD), dB=dbf)
                put(fl.weight, dWf)
                put(fl.bias, dbf)
            if not below[n]:
                return None
            wt = torch.zeros((cin, KPAD), dtype=dt, device=dev)
            wt[:, :K] = S["fw"].t()
            gf = torch.empty((M, cin), dtype=f32, device=dev)
            ops.gemm(dz, wt, gf, **head_calls.final_dgrad(M, cin, K), epilogue=EPI_OUT_F32)
            for li in range(n - 1, -1, -1):
                d = dec[li]
                dc, bn = layers[3 * li], layers[3 * li + 1]
                M = B * d["hh"] * d["ww"]
                cin, cout = d["cin"], d["cout"]
                dY = bn_backward(gf, d, 4 * M, cout, [bn], mode=1, scale=d["st"][2], shift=d["st"][3])
                if wants(dc.weight):
                    dwp = torch.empty((4, cout, 4 * cin), dtype=f32, device=dev)
                    _wgrad(dY, d["x"], dwp, **head_calls.wgrad_of(head_calls.deconv(M, cin, cout)), rowoff=d["ro"],
                           dy_rowmap=d["rm"])
                    put(dc.weight, pack.unpack_deconv_parities(dwp))
                if not below[li]:
                    break
                tab = geo.grad_tables.get(("dgrad", B, d["hh"], d["ww"], cout),
                                          lambda: pack.deconv_data_grad_table(B, d["hh"], d["ww"], 4, cout).to(dev))
                wt = pack.deconv_data_grad_weights(dc.weight.detach()).to(dt).contiguous()
                gf = torch.empty((M, cin), dtype=f32, device=dev)
                ops.gemm(dY, wt, gf, **head_calls.deconv_dgrad(M, cin, cout), rowoff=tab, epilogue=EPI_OUT_F32)
            return gf if x_needs else None

        def aux_backward(gtok):
            """The four aux branches, tails down to the first stage; the branches that reach x add their token gradient
            to gtok (or write it, gtok None).  Returns the tokens' gradient so far."""
            seqs = [list(getattr(head, n + "_layers")) for n in engine.AUX_NAMES]
            gs = (g_prob, g_vis, g_oks, g_err)
            into_x = [x_needs and not head.detach_probability, x_needs and not head.detach_visibility, False, False]
            aux = S["aux"]
            n = len(aux)
            stage_need = [[wants(s[4 * i].weight, s[4 * i].bias, s[4 * i + 1].weight, s[4 * i + 1].bias) for s in seqs]
                          for i in range(n)]
            tail_need = [wants(s[-2].weight, s[-2].bias) for s in seqs]
            below = [any(any(stage_need[j]) for j in range(i)) or any(into_x) for i in range(n + 1)]
            if all(g is None for g in gs) or not (any(tail_need) or below[n]):
                return gtok
            gaux = torch.stack([g.reshape(B, K).float() if g is not None else
                                torch.zeros((B, K), dtype=f32, device=dev) for g in gs]).contiguous()
            dWt = torch.empty((4, K, C), dtype=f32, device=dev) if any(tail_need) else None
            dbt = torch.empty((4, K), dtype=f32, device=dev) if any(tail_need) else None
            dpool = torch.empty((B, 4 * C), dtype=f32, device=dev) if below[n] else None
            ops.aux_tail_backward(S["pooled"], S["tw"], S["aux_out"], gaux, B, C, K, dWt, dbt, dpool)
            for bi, s in enumerate(seqs if any(tail_need) else ()):
                put(s[-2].weight, dWt[bi])
                put(s[-2].bias, dbt[bi])
            for i in range(n - 1, -1, -1):
                if not below[i + 1]:
                    break
                a = aux[i]
                M = B * a["ah"] * a["aw"]
                convs = [s[4 * i] for s in seqs]
                dY = bn_backward(dpool, a, M, 4 * C, [s[4 * i + 1] for s in seqs], mode=2, argmax=a["argmax"],
                                 pool=(B, a["ah"], a["aw"], a["kh"], a["kw"]))
                dW = torch.empty((4, C, 9 * C), dtype=f32, device=dev)
                dB = torch.empty((4, C), dtype=f32, device=dev)
                wneed = [wants(cv.weight, cv.bias) for cv in convs]
                for b0, b1 in _runs(wneed):         # the branches [b0, b1): the stage's descriptor with b1 - b0 branches
                    call = head_calls.aux_stage0 if i == 0 else head_calls.aux_stage
                    _wgrad(dY[:, b0 * C:], a["x"] if i == 0 else a["x"][:, b0 * C:], dW[b0:b1], dB=dB[b0:b1],
                           rowoff=a["ro"], **head_calls.wgrad_of(call(M, C, b1 - b0)))
                for bi, cv in enumerate(convs):
                    put(cv.weight, dW[bi].view(C, 3, 3, C).permute(0, 3, 1, 2))
                    put(cv.bias, dB[bi])
                if i > 0 and below[i]:
                    # the data gradient has the forward's dimensions: the same descriptor over flipped weights
                    wt = torch.stack([pack.conv3x3_data_grad_weights(cv.weight.detach()) for cv in convs])
                    wt = wt.to(dt).contiguous()
                    dpool = torch.empty((M, 4 * C), dtype=f32, device=dev)
                    ops.gemm(dY, wt, dpool, **head_calls.aux_stage(M, C), rowoff=a["ro"], epilogue=EPI_OUT_F32)
                elif i == 0 and any(into_x):
                    brs = [bi for bi in range(4) if into_x[bi]]
                    tab = geo.grad_tables.get(("aux0", B, h, w, tuple(brs)),
                                              lambda: _aux0_dgrad_table(B, h, w, C, brs, dev))
                    wt = torch.stack([pack.conv3x3_data_grad_weights(convs[bi].weight.detach()).view(C, 9, C)
                                      for bi in brs], dim=2).reshape(C, 9 * len(brs) * C).to(dt).contiguous()
                    out = gtok if gtok is not None else torch.empty((M, C), dtype=f32, device=dev)
                    ops.gemm(dY, wt, out, **head_calls.aux0_dgrad(M, C, len(brs)), rowoff=tab, residual=gtok,
                             epilogue=EPI_OUT_F32)       # added to the heatmap branch's token gradient in place
                    gtok = out
            return gtok

        gtok = aux_backward(heatmap_backward())
        gx = None
        if x_needs and not S["nchw"]:
            # the token gradient as it is, f32 [B*h*w, C] (autograd casts it to the tokens' dtype)
            gx = gtok if gtok is not None else torch.zeros((B * h * w, C), dtype=f32, device=dev)
        elif x_needs:
            if gtok is None:
                gx = torch.zeros((B, C, h, w), dtype=f32, device=dev)
            else:
                gx = torch.empty((B, C, h, w), dtype=f32, device=dev)
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
    inp = x if x is not None else tokens
    _lib.require_device(inp)
    if x is not None:
        B, C, h, w = x.shape
        if C != head.in_channels:
            raise ValueError(f"ProbMapHead: expected {head.in_channels} channels, got {C}")
    else:
        B, h, w = geom
        if tokens.dtype != head.compute_dtype:
            raise TypeError(f"tokens are {tokens.dtype}, the head computes in {head.compute_dtype}")
        inp = tokens if tokens.requires_grad else tokens.detach()
    params = head_parameters(head)
    for p in params:
        if p.device != inp.device:
            raise ValueError(f"ProbMapHead parameters are on {p.device}, the input on {inp.device}: move the head first")
    with torch.cuda.device(inp.device):
        return _HeadTrainFn.apply(head, inp, x is not None, (B, head.in_channels, h, w), *params)
