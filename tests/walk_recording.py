"""Recording of the launches of a forward: every wrapper of probpose_pytorch_amd.ops that engine.VitPlan and
engine.HeadPlan call is replaced, by attribute on the module, with one that notes what the launch was handed.

A record is the list of launches in host order, one dict per launch:
  op       "patchify" | "patch_embed" | "gemm" | "linear" | "layernorm" | "attention" | "qkv_attention" | "maxpool_relu"
           | "maxpool_relu_sum" | "aux_tail" | "final_heatmap" | "sparsemax_rows" | "tokens_to_nchw"
           (an ops.gemm call outside ops.linear is "patch_embed" when it carries a rowbias, "gemm" otherwise)
  args     name -> tensor as the launch read it (cloned before the call)
  scalars  every other argument as passed; for ops.gemm the whole keyword set (dimensions, pitches, strides,
           epilogue, heatmap / headmajor tuples; fuse_final as (K, HW, temperature, clamp), its two tensors in args as
           final_w / final_b), so that gemm_kw(e) is what gemm_reference.expected_output takes
  out      the output after the call (cloned)
  ptrs     name -> address of every tensor argument and of "out"
  meta     name -> (dtype, shape)
The clones are enqueued on whatever stream is current where the launch is made (the head's aux branch and the second
chain of engine.DUAL_CHAIN run on streams of their own), so each sees its launch's operands in stream order; the
caller synchronises the device once after the forward and before it reads anything."""
import contextlib

import torch

VIT_OPS = ("layernorm", "linear", "attention", "gemm")          # what the fp8 walk's comparator knows
ALL_OPS = VIT_OPS + ("patchify", "qkv_attention", "maxpool_relu", "maxpool_relu_sum", "aux_tail", "final_heatmap",
                     "sparsemax_rows", "tokens_to_nchw")
GEMM_TENSORS = ("A", "W", "bias", "residual", "rowbias", "rowoff", "out_rowmap", "colscale")


def gemm_kw(e) -> dict:
    """The keyword set of a recorded ops.gemm launch as gemm_reference.expected_output reads it (no fuse_final)."""
    kw = dict(e["scalars"])
    kw.pop("fuse_final", None)
    kw.pop("tile", None)
    kw.update({k: e["args"][k] for k in GEMM_TENSORS if k in e["args"]})
    kw["out"] = e["out"]
    return kw


@contextlib.contextmanager
def recording(ops, names=ALL_OPS):
    """Wrap ops.<name> for every name in `names`; yields the record (a list that fills as launches are made)."""
    rec = []
    real = {k: getattr(ops, k) for k in names}
    inside_linear = [False]

    def entry(op, args, scalars, out, call):
        assert all(t.is_contiguous() for t in args.values() if t is not None) and out.is_contiguous()
        e = dict(op=op, args={k: t.clone() for k, t in args.items() if t is not None}, scalars=scalars,
                 ptrs={k: t.data_ptr() for k, t in dict(args, out=out).items() if t is not None},
                 meta={k: (t.dtype, tuple(t.shape)) for k, t in dict(args, out=out).items() if t is not None})
        r = call()
        e["out"] = out.clone()
        rec.append(e)
        return r

    def layernorm(x, gamma, beta, eps, out, out_scale=None):
        return entry("layernorm", dict(x=x, gamma=gamma, beta=beta), dict(eps=eps, out_scale=out_scale), out,
                     lambda: real["layernorm"](x, gamma, beta, eps, out, out_scale=out_scale))

    def linear(x, w, bias=None, *, out=None, epilogue=0, residual=None, colscale=None, out_scale=None, headmajor=None,
               tile=0, **kw):
        assert out is not None and not kw, "the walk hands every linear its output buffer"

        def call():
            inside_linear[0] = True
            try:
                return real["linear"](x, w, bias, out=out, epilogue=epilogue, residual=residual, colscale=colscale,
                                      out_scale=out_scale, headmajor=headmajor, tile=tile)
            finally:
                inside_linear[0] = False
        return entry("linear", dict(x=x, w=w, bias=bias, residual=residual, colscale=colscale),
                     dict(epilogue=epilogue, out_scale=out_scale, headmajor=headmajor, tile=tile), out, call)

    def attention(qkv, out, B, N, heads, hd, out_scale=None, headmajor=False):
        return entry("attention", dict(qkv=qkv), dict(B=B, N=N, heads=heads, hd=hd, out_scale=out_scale,
                                                      headmajor=headmajor), out,
                     lambda: real["attention"](qkv, out, B, N, heads, hd, out_scale=out_scale, headmajor=headmajor))

    def gemm(A, W, out, **kw):
        if inside_linear[0]:
            return real["gemm"](A, W, out, **kw)
        if "patchify" not in names:
            assert kw.get("rowbias") is not None, "a GEMM outside ops.linear that is not the patch embedding"
        args = dict(A=A, W=W, **{k: kw[k] for k in GEMM_TENSORS[2:] if kw.get(k) is not None})
        scalars = {k: v for k, v in kw.items() if k not in GEMM_TENSORS and k != "fuse_final"}
        if kw.get("fuse_final") is not None:
            args["final_w"], args["final_b"] = kw["fuse_final"][:2]
            scalars["fuse_final"] = tuple(kw["fuse_final"][2:])
        return entry("patch_embed" if kw.get("rowbias") is not None else "gemm", args, scalars, out,
                     lambda: real["gemm"](A, W, out, **kw))

    def qkv_attention(h, w_hm, b_hm, out, B, heads):
        return entry("qkv_attention", dict(h=h, w_hm=w_hm, b_hm=b_hm), dict(B=B, heads=heads), out,
                     lambda: real["qkv_attention"](h, w_hm, b_hm, out, B, heads))

    def patchify(x, out, patch):
        return entry("patchify", dict(x=x), dict(patch=patch), out, lambda: real["patchify"](x, out, patch))

    def maxpool_relu(x, out, B, h, w, Cc, kh, kw):
        return entry("maxpool_relu", dict(x=x), dict(B=B, h=h, w=w, Cc=Cc, kh=kh, kw=kw), out,
                     lambda: real["maxpool_relu"](x, out, B, h, w, Cc, kh, kw))

    def maxpool_relu_sum(parts, bias, out, B, h, w, Cc, kh, kw):
        return entry("maxpool_relu_sum", dict(parts=parts, bias=bias), dict(B=B, h=h, w=w, Cc=Cc, kh=kh, kw=kw), out,
                     lambda: real["maxpool_relu_sum"](parts, bias, out, B, h, w, Cc, kh, kw))

    def aux_tail(x, w, bias, out, B, Cc, K):
        return entry("aux_tail", dict(x=x, w=w, bias=bias), dict(B=B, Cc=Cc, K=K), out,
                     lambda: real["aux_tail"](x, w, bias, out, B, Cc, K))

    def final_heatmap(x, w, bias, out, B, HW, Cin, K, temperature, clamp=True):
        return entry("final_heatmap", dict(x=x, w=w, bias=bias),
                     dict(B=B, HW=HW, Cin=Cin, K=K, temperature=temperature, clamp=clamp), out,
                     lambda: real["final_heatmap"](x, w, bias, out, B, HW, Cin, K, temperature, clamp=clamp))

    def sparsemax_rows(x, scale):                          # in place: "x" is the input, "out" the same buffer afterwards
        return entry("sparsemax_rows", dict(x=x), dict(scale=scale), x, lambda: real["sparsemax_rows"](x, scale))

    def tokens_to_nchw(x, out, B, N, Cc):
        return entry("tokens_to_nchw", dict(x=x), dict(B=B, N=N, Cc=Cc), out,
                     lambda: real["tokens_to_nchw"](x, out, B, N, Cc))

    wrappers = dict(layernorm=layernorm, linear=linear, attention=attention, gemm=gemm, qkv_attention=qkv_attention,
                    patchify=patchify, maxpool_relu=maxpool_relu, maxpool_relu_sum=maxpool_relu_sum, aux_tail=aux_tail,
                    final_heatmap=final_heatmap, sparsemax_rows=sparsemax_rows, tokens_to_nchw=tokens_to_nchw)
    try:
        for k in names:
            setattr(ops, k, wrappers[k])
        yield rec
    finally:
        for k, f in real.items():
            setattr(ops, k, f)
