"""Mint colormaps.json, next to this file, from the installed matplotlib: the float64 [256, 3] lookup tables of ``jet``
and ``inferno`` that ``Colormap.__call__`` indexes.  They are matplotlib's data, written as text (the repr of a float64
reads back as the same float64); the package reads the file and never imports matplotlib.  Run once:
    python probpose_pytorch_amd/data/make_colormaps.py
tests/test_viz_reference.py holds the file to the installed matplotlib bit for bit."""
import json
import os

import matplotlib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("jet", "inferno")


def table(name: str) -> np.ndarray:
    cmap = matplotlib.colormaps[name]
    assert cmap.N == 256
    cmap(0.0)                                   # builds the table of a segmented map (jet)
    return np.ascontiguousarray(cmap._lut[:256, :3], dtype=np.float64)


if __name__ == "__main__":
    with open(os.path.join(HERE, "colormaps.json"), "w") as f:
        json.dump({n: table(n).tolist() for n in NAMES}, f, indent=0)
    print("colormaps.json from matplotlib", matplotlib.__version__)
