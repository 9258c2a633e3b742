"""Mint tests/golden/head_grad.npz: one train-mode step of the REFERENCE ProbMapHead (probpose/head.py, unmodified,
``.train()``, float64 on the CPU) for three small constructions, with seeded weights (synthetic_head_state, or the
reference's own initialisation), inputs and upstream gradients:
  T1  C = 64, K = 5, 8x6 features, pools [(4, 3), (2, 2)], deconvolutions (64, 64), synthetic weights
  T2  as T1 with detach_probability=False and an input that requires grad (seed 42)
  T3  as T1 with freeze_error=True and the reference's initialisation (N(0, 0.001) convolutions, unit BatchNorm)
  T4  as T1 with an input that requires grad (the default detaches: only the heatmap branch reaches it)
It records the outputs, every parameter gradient, the input gradient and the running statistics after the step.
Arrays of at most 256 elements are stored whole; larger ones as their sum, their absolute sum and every 251st element.
The weights, inputs and upstream gradients are not stored: the tests rebuild them from the seeds (the upstream
gradients are float64 torch.randn of the five outputs' shapes, in order, from torch.Generator().manual_seed(seed + 200)).
cv2 is registered as an empty stub exactly as in make_goldens.py (imported by the reference package, unused here).
Run once:  cd /tmp && python <repo>/tests/golden/make_goldens_head_grad.py <reference checkout>"""
import importlib.util
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(f"usage: python {sys.argv[0]} <reference checkout>")
REF = os.path.abspath(sys.argv[1])

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, REF)
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
import probpose  # noqa: E402

assert all(os.path.abspath(p).startswith(REF) for p in probpose.__path__)
from probpose.head import ProbMapHead  # noqa: E402

CASES = {
    # name: (C, K, pools, hw, deconv_out, seed, kwargs, synthetic weights, x requires grad)
    "T1": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 41, {}, True, False),
    "T2": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 42, {"detach_probability": False}, True, True),
    "T3": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 43, {"freeze_error": True}, False, False),
    "T4": (64, 5, [(4, 3), (2, 2)], (8, 6), (64, 64), 44, {}, True, True),
}
WHOLE = 256
STEP = 251


def store(out, key, t):
    a = t.detach().double().numpy()
    if a.size <= WHOLE:
        out[key] = a
    else:
        out[key + "#sum"] = np.array(a.sum())
        out[key + "#abssum"] = np.array(np.abs(a).sum())
        out[key + "#sample"] = a.reshape(-1)[::STEP].copy()


def load_syn():
    spec = importlib.util.spec_from_file_location("pp_synthetic_for_goldens",
                                                  os.path.join(REPO, "probpose_pytorch_amd", "synthetic.py"))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    return syn


def case_state(name):
    """(head construction args, state_dict, x, upstream gradients) of a case, from its seeds alone."""
    syn = load_syn()
    C, K, pools, (h, w), dec, seed, kw, synthetic, xg = CASES[name]
    torch.manual_seed(seed)
    head = ProbMapHead(C, K, pools, dec, (4,) * len(dec), final_layer_kernel_size=1, **kw)
    if synthetic:
        head.load_state_dict(syn.synthetic_head_state(C, K, n_pools=len(pools), deconv_out=dec, seed=seed),
                             strict=False)
    feats = syn.synthetic_features(2, C, h, w, seed=seed + 100)
    return head, feats


def main():
    out = {}
    for name, (C, K, pools, (h, w), dec, seed, kw, synthetic, xg) in CASES.items():
        head, feats = case_state(name)
        head = head.double().train()
        x = feats.double().clone().requires_grad_(xg)
        outs = head(x)
        g = torch.Generator().manual_seed(seed + 200)
        ups = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
        torch.autograd.backward([o for o in outs if o.requires_grad], [u for o, u in zip(outs, ups) if o.requires_grad])
        for i, o in enumerate(outs):
            store(out, f"{name}/out{i}", o)
        for k, p in head.named_parameters():
            if p.grad is not None:
                store(out, f"{name}/grad/{k}", p.grad)
            else:
                out[f"{name}/nograd/{k}"] = np.array(1)
        if xg:
            store(out, f"{name}/xgrad", x.grad)
        for k, b in head.named_buffers():
            store(out, f"{name}/run/{k}", b)
        print(name, "heat range", float(outs[0].min()), float(outs[0].max()))
    np.savez_compressed(os.path.join(HERE, "head_grad.npz"), **out)


if __name__ == "__main__":
    main()
