"""CPU tests of the FusedAdamW boundary: the optimizer entry points refuse bad arguments on the host, before any
launch, and the Python class refuses what it does not implement; none of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch


def _build(lib, n=3, counts=(5, 8192, 8193), p=0x1000, table_off=0, n_groups=2, group=(0, 1, 0), step=0x2000):
    counts = np.asarray(counts, dtype=np.int64)
    ptrs = np.full(max(n, 1), p, dtype=np.uint64)
    steps = np.full(max(n, 1), step, dtype=np.uint64)
    grp = np.asarray(group, dtype=np.int32)
    hyper = np.array([[1e-3, 0.9, 0.999, 1e-8, 0.1]] * max(n_groups, 1))
    host = np.zeros(4096, dtype=np.uint64)
    nc, prefix = C.c_int(-1), C.c_longlong(-1)
    rc = lib.pp_optim_table_build(n, ptrs.ctypes.data, ptrs.ctypes.data, ptrs.ctypes.data, ptrs.ctypes.data,
                                  steps.ctypes.data, counts.ctypes.data, grp.ctypes.data, n_groups, hyper.ctypes.data,
                                  0x3000, host.ctypes.data + table_off, 1, C.byref(nc), C.byref(prefix))
    return rc, nc.value, prefix.value, host


def test_table_build_packs_and_validates(built_lib):
    rc, nc, prefix, host = _build(built_lib)
    assert rc == 0 and nc == 1 + 1 + 2 and prefix == 32 + 2 * 40 + 3 * 56
    counts = np.array([5, 8192, 8193], dtype=np.int64)
    assert built_lib.pp_optim_table_bytes(3, counts.ctypes.data, 2) == prefix + 8 * nc
    chunk_map = host.view(np.int32)[prefix // 4: prefix // 4 + 2 * nc].reshape(nc, 2)
    assert chunk_map.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1]]
    for kwargs, word in ((dict(n=0), b"zero tensors"), (dict(counts=(5, -1, 7)), b"count"),
                         (dict(counts=(5, 0, 7)), b"count"), (dict(p=0), b"null pointer"),
                         (dict(step=0), b"null pointer"), (dict(p=0x1002), b"aligned"),
                         (dict(table_off=4), b"8-byte aligned"), (dict(group=(0, 2, 0)), b"group"),
                         (dict(n_groups=0), b"n_groups")):
        rc = _build(built_lib, **kwargs)[0]
        assert rc != 0 and word in built_lib.pp_last_error(), (kwargs, built_lib.pp_last_error())
    assert built_lib.pp_optim_table_bytes(0, counts.ctypes.data, 2) == -1
    assert built_lib.pp_optim_table_bytes(3, None, 2) == -1
    bad = np.array([5, 0, 7], dtype=np.int64)
    assert built_lib.pp_optim_table_bytes(3, bad.ctypes.data, 2) == -1 and b"count" in built_lib.pp_last_error()


def test_launch_entry_points_refuse_bad_arguments_without_gpu(built_lib):
    from probpose_pytorch_amd import _lib
    L = built_lib
    assert L.pp_grad_sqnorm_partials(None, 4, 0x1000, None) != 0 and b"null table" in L.pp_last_error()
    assert L.pp_grad_sqnorm_partials(0x1004, 4, 0x1000, None) != 0 and b"aligned" in L.pp_last_error()
    assert L.pp_grad_sqnorm_partials(0x1000, 0, 0x1000, None) != 0 and b"n_chunks" in L.pp_last_error()
    assert L.pp_grad_sqnorm_partials(0x1000, -3, 0x1000, None) != 0 and b"n_chunks" in L.pp_last_error()
    assert L.pp_grad_sqnorm_partials(0x1000, 4, None, None) != 0 and b"null partials" in L.pp_last_error()
    assert L.pp_grad_norm_finish(None, 4, 1, 1.0, 0, 0x2000, None) != 0 and b"null" in L.pp_last_error()
    assert L.pp_grad_norm_finish(0x1000, 4, 1, 1.0, 0, None, None) != 0 and b"null" in L.pp_last_error()
    for max_norm in (0.0, -1.0, float("nan")):
        assert L.pp_grad_norm_finish(0x1000, 4, 1, max_norm, 0, 0x2000, None) != 0
        assert b"max_norm" in L.pp_last_error()
    assert L.pp_grad_norm_finish(0x1000, 0, 1, 1.0, 0, 0x2000, None) != 0 and b"n_chunks" in L.pp_last_error()
    assert L.pp_adamw_step(None, 4, None, 0, None) != 0 and b"null table" in L.pp_last_error()
    assert L.pp_adamw_step(0x1000, 0, None, 0, None) != 0 and b"n_chunks" in L.pp_last_error()
    assert L.pp_adamw_step(0x1000, 4, None, 1, None) != 0 and b"skip_nonfinite" in L.pp_last_error()
    assert L.pp_adamw_step(0x1002, 4, None, 0, None) != 0 and b"aligned" in L.pp_last_error()
    with pytest.raises(_lib.HipExtensionError):
        _lib.check(1, "pp_adamw_step")


def test_fused_adamw_refuses_what_it_does_not_implement():
    from probpose_pytorch_amd import FusedAdamW, _lib
    p = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError):
        FusedAdamW([p], amsgrad=True)
    with pytest.raises(NotImplementedError):
        FusedAdamW([p], maximize=True)
    with pytest.raises(NotImplementedError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(NotImplementedError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(ValueError):
        FusedAdamW([p], max_grad_norm=0.0)
    if not p.is_cuda:
        with pytest.raises(_lib.HipExtensionError):      # the hot path has no CPU fallback
            FusedAdamW([p])


def test_state_dict_of_torch_adamw_passes_validation():
    from probpose_pytorch_amd.optim import validate_state_dict

    def make():
        torch.manual_seed(0)
        a, b = torch.nn.Parameter(torch.randn(6, 5)), torch.nn.Parameter(torch.randn(7))
        c = torch.nn.Parameter(torch.randn(3))               # never gets a gradient: no state
        return [a, b, c], torch.optim.AdamW([dict(params=[a], weight_decay=0.1), dict(params=[b, c])], lr=1e-3)

    ps, opt = make()
    for _ in range(3):
        ps[0].grad, ps[1].grad = torch.randn(6, 5), torch.randn(7)
        opt.step()
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    groups = make()[1].param_groups
    validate_state_dict(sd, groups)
    bad = {"state": {**sd["state"], 0: {**sd["state"][0], "exp_avg": torch.zeros(5, 6)}},
           "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError, match="shape"):
        validate_state_dict(bad, groups)
    bad = {"state": {**sd["state"], 1: {"step": sd["state"][1]["step"], "exp_avg": sd["state"][1]["exp_avg"]}},
           "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError, match="keys"):
        validate_state_dict(bad, groups)
    with pytest.raises(ValueError, match="groups"):
        validate_state_dict({"state": sd["state"], "param_groups": sd["param_groups"][:1]}, groups)
    ams = {"state": sd["state"], "param_groups": [dict(g, amsgrad=True) for g in sd["param_groups"]]}
    with pytest.raises(NotImplementedError):
        validate_state_dict(ams, groups)
