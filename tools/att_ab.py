#!/usr/bin/env python3
"""A/B of the attention entry points between two builds of the library, interleaved in one process: nine rounds of 20
launches per build and shape, medians, torch.equal on the outputs.  A build is `shipped` (the package's library) or the
name of a lib/exp/*.so (tools/build_exp.sh); two builds of the same source give the spread a real difference has to
exceed.  The shapes reach all ten older kernel forms (which (N, head_dim) selects which: ATT_FORMS / _att_cases() in
tests/test_attention_layernorm_forms_gpu.py), the e4m3 output and the head-major layout.
usage: att_ab.py <build a> <build b>      e.g.  att_ab.py parent_a.so parent_b.so;  att_ab.py parent_a.so shipped"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from probpose_pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, LAUNCHES = 9, 20
_i, _vp = C.c_int, C.c_void_p


def load(name):
    L = C.CDLL(_lib.LIB_PATH if name == "shipped" else os.path.join(ROOT, "probpose_pytorch_amd", "lib", "exp", name))
    for fn, args in (("pp_attention", [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
                     ("pp_attention_fp8out", [_vp, _vp, _i, _i, _i, _i, C.c_float, _vp]),
                     ("pp_attention_headmajor", [_vp, _vp, _i, _i, _i, _i, _vp])):
        getattr(L, fn).restype, getattr(L, fn).argtypes = _i, args
    return L


# (name, the form it runs, entry, B, N, heads, hd); entry: bf16 = pp_attention, e4m3 = pp_attention_fp8out, hm = headmajor
SHAPES = [
    ("vit_b bs64", "mfma<64,true>", "bf16", 64, 192, 12, 64),
    ("vit_l bs256", "mfma<64,true>", "bf16", 256, 192, 16, 64),
    ("ragged N = 50, hd 64", "mfma<64,false>", "bf16", 1, 50, 4, 64),
    ("vit_s bs64 (hd 32)", "mfma<32,true>", "bf16", 64, 192, 12, 32),
    ("N = 150, hd 32", "mfma<32,false>", "bf16", 64, 150, 12, 32),
    ("vit_h 384x288 bs128 (hd 80)", "stream<80,3,3,32>", "bf16", 128, 432, 16, 80),
    ("ragged N = 433, hd 80", "stream<80,4,2,64>", "bf16", 8, 433, 16, 80),
    ("vit_l 384x288 bs64 (hd 64)", "stream<64,3,3,32>", "bf16", 64, 432, 16, 64),
    ("N = 500, hd 64", "stream<64,4,2,64>", "bf16", 32, 500, 16, 64),
    ("N = 432, hd 32", "stream<32,3,3,32>", "bf16", 32, 432, 12, 32),
    ("ragged N = 200, hd 32", "stream<32,4,2,64>", "bf16", 2, 200, 2, 32),
    ("vit_b bs64, e4m3 out", "mfma<64,true>", "e4m3", 64, 192, 12, 64),
    ("vit_l 384x288 bs64, e4m3 out", "stream<64,3,3,32>", "e4m3", 64, 432, 16, 64),
    ("vit_h 384x288 bs128, head-major", "stream<80,3,3,32>", "hm", 128, 432, 16, 80),
]


def main():
    names = sys.argv[1:3]
    if len(names) != 2 or names[0] == names[1]:
        sys.exit(__doc__)
    libs = {n: load(n) for n in names}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"{torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} interleaved rounds of {LAUNCHES} launches")
    print(f"{'shape':34s} {'form':18s} {names[0]:>14s} {names[1]:>14s}   b / a - 1   outputs identical")
    worst, all_same = 0.0, True
    for name, form, entry, B, N, heads, hd in SHAPES:
        Cc = heads * hd
        qkv = torch.randn((B * N, 3 * Cc), device="cuda").to(torch.bfloat16)
        odt = torch.uint8 if entry == "e4m3" else torch.bfloat16
        outs = {k: torch.zeros((B * N, Cc), dtype=odt, device="cuda") for k in libs}
        times = {k: [] for k in libs}
        for _ in range(ROUNDS):
            for k, L in libs.items():
                q, o = qkv.data_ptr(), outs[k].data_ptr()
                call = {"bf16": lambda: L.pp_attention(q, o, B, N, heads, hd, 1, st),
                        "e4m3": lambda: L.pp_attention_fp8out(q, o, B, N, heads, hd, 16.0, st),
                        "hm": lambda: L.pp_attention_headmajor(q, o, B, N, heads, hd, st)}[entry]
                assert call() == 0
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(LAUNCHES):
                    call()
                e.record()
                e.synchronize()
                times[k].append(s.elapsed_time(e) / LAUNCHES * 1e3)
        a, b = (outs[k].view(torch.uint8 if entry == "e4m3" else torch.int16) for k in names)
        same = torch.equal(a, b)
        all_same &= same
        if not same:
            bad = (a != b).nonzero()
            print("   differing elements:", bad.shape[0], "first", bad[:6].tolist(), "rows", sorted(set(bad[:, 0].tolist()))[:12],
                  "cols", sorted(set(bad[:, 1].tolist()))[:24])
        ma, mb = (sorted(times[k])[ROUNDS // 2] for k in names)
        worst = max(worst, abs(mb / ma - 1))
        print(f"{name:34s} {form:18s} {ma:14.2f} {mb:14.2f}   {(mb / ma - 1) * 100:+8.2f} %   {same}")
    print(f"largest relative difference of the medians: {worst * 100:.2f} %; all outputs identical: {all_same}")


if __name__ == "__main__":
    main()
