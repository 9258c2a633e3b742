#!/usr/bin/env python3
"""A/B of the qkv projection + attention of one ViT block (bf16, N = 192, head_dim 64): ops.linear on the autotuned tile
followed by ops.attention, against the one launch of ops.qkv_attention.  One process, random h and weights, HIP events,
7 interleaved rounds of 10 launches, medians; also whether the two outputs are bit-equal.
With two builds named (`shipped`, or a lib/exp/*.so of tools/build_exp.sh) it times pp_qkv_attention_bf16 of the one
against the other instead, same method, and checks that their outputs are the same bits; two builds of one source give
the spread.
usage: qkv_attention_ab.py [<build a> <build b>] [> profiles/qkv_attention_ab.txt]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from probpose_pytorch_amd import _lib, ops

ROUNDS, LAUNCHES = 7, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = sys.argv[1:3]
if len(BUILDS) not in (0, 2) or len(set(BUILDS)) != len(BUILDS):
    sys.exit(__doc__)


def load(name):
    L = ctypes.CDLL(_lib.LIB_PATH if name == "shipped" else os.path.join(ROOT, "probpose_pytorch_amd", "lib", "exp", name))
    L.pp_qkv_attention_bf16.restype, L.pp_qkv_attention_bf16.argtypes = _lib._SIGNATURES["pp_qkv_attention_bf16"]
    return L


def timed(fn):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES * 1e3


def median(v):
    return sorted(v)[len(v) // 2]


print(f"{torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} interleaved rounds of {LAUNCHES} launches")
for name, B, heads in [("vit_b bs64", 64, 12), ("vit_l bs256", 256, 16)]:
    C, N = heads * 64, 192
    gen = torch.Generator(device="cuda").manual_seed(B + heads)
    h = torch.randn((B * N, C), device="cuda", generator=gen).to(torch.bfloat16)
    w = (torch.randn((3 * C, C), device="cuda", generator=gen) * C ** -0.5).to(torch.bfloat16)
    b = torch.randn((3 * C,), device="cuda", generator=gen) * 0.5
    w_hm, b_hm = ops.pack_qkv_headmajor(w, b, heads)
    qkv = torch.empty((B * N, 3 * C), dtype=torch.bfloat16, device="cuda")
    out2, out1 = (torch.empty((B * N, C), dtype=torch.bfloat16, device="cuda") for _ in range(2))
    ops.AUTOTUNE = True
    ops.linear(h, w, b, out=qkv)                                  # times the candidate tiles, keeps the winner
    ops.AUTOTUNE = False
    tile = next(iter(ops._TUNE_CACHE.values()))
    ops._TUNE_CACHE.clear()
    if BUILDS:
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        outs = {k: torch.zeros_like(out1) for k in BUILDS}
        calls = {k: (lambda L=load(k), o=outs[k]: L.pp_qkv_attention_bf16(h.data_ptr(), w_hm.data_ptr(), b_hm.data_ptr(),
                                                                            o.data_ptr(), B, heads, C, st)) for k in BUILDS}
        assert all(c() == 0 for c in calls.values())
        times = {k: [] for k in BUILDS}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        torch.cuda.synchronize()
        same = torch.equal(*(o.view(torch.int16) for o in outs.values()))
        print(f"{name}: B={B} heads={heads} C={C}, pp_qkv_attention_bf16")
        for k, v in times.items():
            print(f"  {k:22s} {median(v):8.2f}   (min {min(v):.2f}, max {max(v):.2f})")
        a, b_ = (median(times[k]) for k in BUILDS)
        print(f"  {BUILDS[1]} against {BUILDS[0]}: {b_ - a:+.2f} us ({(b_ / a - 1) * 100:+.2f} %); outputs bit-equal: {same}")
        continue
    runs = {
        f"linear (tile {tile})": lambda: ops.linear(h, w, b, out=qkv, tile=tile),
        "attention": lambda: ops.attention(qkv, out2, B, N, heads, 64),
        "linear + attention": lambda: (ops.linear(h, w, b, out=qkv, tile=tile), ops.attention(qkv, out2, B, N, heads, 64)),
        "linear (tile 14)": lambda: ops.linear(h, w, b, out=qkv, tile=14),
        "qkv_attention": lambda: ops.qkv_attention(h, w_hm, b_hm, out1, B, heads),
    }
    times = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    runs["linear + attention"]()
    runs["qkv_attention"]()
    torch.cuda.synchronize()
    same = torch.equal(out1.view(torch.int16), out2.view(torch.int16))
    print(f"{name}: B={B} heads={heads} C={C}")
    for k, v in times.items():
        print(f"  {k:22s} {median(v):8.2f}   (min {min(v):.2f}, max {max(v):.2f})")
    two, one = median(times["linear + attention"]), median(times["qkv_attention"])
    print(f"  one launch against two: {one - two:+.2f} us ({(one / two - 1) * 100:+.1f} %); outputs bit-equal: {same}")
