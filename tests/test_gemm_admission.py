"""pp_gemm admits and refuses exactly the calls recorded in tests/golden/gemm_admission.json (CPU only).

pp_gemm's checks all run before its first HIP call, so without a GPU a refused call fails with a "pp_gemm:" message
and an admitted one fails inside the runtime.  The matrix (dtype x shape x epilogue x operand structure x C alignment
x tile -1..21) and the way a verdict is read are those of tests/golden/make_gemm_admission.py, which recorded it."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_gemm_admission",
                                                  os.path.join(HERE, "golden", "make_gemm_admission.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gemm_admission_matches_the_recorded_matrix(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the pointers are fake, an admitted call must never reach a real device")
    from probpose_pytorch_amd import _lib
    gen = _generator()
    with open(gen.OUT) as f:
        doc = json.load(f)
    assert doc["tiles"] == list(gen.TILES)
    recorded = doc["verdicts"]
    keys = [k for k, _ in gen.cases()]
    assert sorted(keys) == sorted(recorded) and len(keys) * len(gen.TILES) >= 49680
    for t in gen.LIVE_TILES:             # the matrix shows every live form both ways
        col = {v[gen.TILES.index(t)] for v in recorded.values()}
        assert col == {"A", "R"}, f"tile {t}"
    wrong = []
    for key, case in gen.cases():
        a = gen.make_args(_lib, *case)
        # verdict() itself requires every refusal to start with "pp_gemm:" and every admitted call to fail in the runtime
        got = "".join(gen.verdict(built_lib, a, t) for t in gen.TILES)
        if got != recorded[key]:
            wrong += [f"{key} tile {t}: recorded {r}, got {g}" for t, r, g in zip(gen.TILES, recorded[key], got) if r != g]
    assert not wrong, f"{len(wrong)} verdicts changed, e.g. " + "; ".join(wrong[:10])
