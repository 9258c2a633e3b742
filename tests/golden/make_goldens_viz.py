"""Mint tests/golden/viz.npz by running the reference's own overlay_heatmap_on_image (reference viz.py:4-38) in this
container, on the inputs of tests/viz_reference.py::golden_inputs: maps on which the reference cannot wrap (disjoint
supports above its 0.01 threshold, or per-channel colour sums of at most 1, asserted here), holding 1.0, NaN, -0.5, 1.5,
float32(0.01) and its neighbours.  The image is passed as int64 so that the reference's np.clip is effective.  cv2 is
registered as an empty stub exactly as in make_goldens.py.  Run once, from a directory outside this repository, with
the reference's checkout as the argument:
    python <this repository>/tests/golden/make_goldens_viz.py <reference checkout>
Only outputs (and the seed) are stored; the tests regenerate the inputs from the seed."""
import importlib.util
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1])             # the reference's checkout: the directory that holds probpose/

import numpy as np  # noqa: E402

spec = importlib.util.spec_from_file_location("viz_reference", os.path.join(REPO, "tests", "viz_reference.py"))
VR = importlib.util.module_from_spec(spec)
spec.loader.exec_module(VR)

sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, REF)
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
import probpose  # noqa: E402

assert all(os.path.abspath(p).startswith(REF) for p in probpose.__path__)
from matplotlib import cm  # noqa: E402
from probpose.viz import overlay_heatmap_on_image  # noqa: E402


def main():
    out = {}
    for name in ("jet", "inferno"):
        images, maps = VR.golden_inputs(name)
        got = []
        for image, hm in zip(images, maps):
            with warnings.catch_warnings(), np.errstate(invalid="ignore"):
                warnings.simplefilter("ignore")
                coloured = np.stack([cm.get_cmap(name)(m)[:, :, :3] * (~(m < 0.01))[..., None] for m in hm])
                assert coloured.sum(axis=0).max() <= 1.0, "the reference would wrap on these maps"
                got.append(overlay_heatmap_on_image(image.astype(np.int64), hm, name))
        out[name] = np.stack(got)
        assert out[name].dtype == np.uint8 and out[name].shape == images.shape
    np.savez_compressed(os.path.join(HERE, "viz.npz"), seed=VR.GOLDEN_SEED, **out)
    print("viz.npz:", {k: (v.shape, v.dtype, int((v != VR.golden_inputs(k)[0]).sum())) for k, v in out.items()})


if __name__ == "__main__":
    main()
