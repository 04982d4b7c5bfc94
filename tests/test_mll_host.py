"""The host side of the device fit (no GPU; a device is never touched): the argument checks of
dkg_mll_workspace / dkg_mll_value_grad, which come before any HIP call, the ABI version, and fit_map's host route,
which the device route must leave bit for bit as it was."""

import ctypes
import json
import os

import pytest

from dkg_amd import _lib
from dkg_amd.bo_smoke import reference_model_config
from dkg_amd.fit import fit_map
from test_fit import _data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_map_parent.json")


def fake_outputs(ns, kernel=2):
    outs = (_lib.DkgOutput * len(ns))()
    for o, n in zip(outs, ns):
        o.n, o.kernel = n, kernel
        o.outputscale, o.noise, o.y_std = 1.0, 1e-3, 1.0
        o.inv_lengthscale = 64  # never dereferenced: the checks come first
        o.train_x = 64
    return outs


def workspace(lib, ns):
    return lib.dkg_mll_workspace((ctypes.c_int * len(ns))(*ns), len(ns))


def call(lib, ns=(64,), **kw):
    m = kw.pop("m", len(ns))
    a = dict(outs=fake_outputs(ns), d=2, train_y=(ctypes.c_void_p * max(len(ns), 1))(*[64] * len(ns)), max_tries=3,
             work=64, work_bytes=1 << 30, value=(ctypes.c_double * 8)(), grad=(ctypes.c_double * 8 * 19)(),
             jitter=(ctypes.c_double * 8)())
    a.update(kw)
    grad = None if a["grad"] is None else ctypes.cast(a["grad"], ctypes.POINTER(ctypes.c_double))
    return lib.dkg_mll_value_grad(a["outs"], m, a["d"], a["train_y"], a["max_tries"], a["work"], a["work_bytes"],
                                  a["value"], grad, a["jitter"], None)


def test_abi_version_is_still_9():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.dkg_abi_version() == 9
    assert lib.dkg_mll_workspace.restype is ctypes.c_size_t and lib.dkg_mll_value_grad.restype is ctypes.c_int


def test_workspace_sizes():
    lib = _lib.load()
    assert workspace(lib, [1]) > 0
    assert lib.dkg_mll_workspace(None, 1) == 0
    ns = (ctypes.c_int * 9)(*[16] * 9)
    assert lib.dkg_mll_workspace(ns, 0) == 0 and lib.dkg_mll_workspace(ns, 9) == 0
    assert lib.dkg_mll_workspace(ns, 8) > 0
    assert workspace(lib, [0]) == 0 and workspace(lib, [1025]) == 0 and workspace(lib, [64, 0]) == 0
    assert workspace(lib, [1024]) >= 2 * 1024 * 1024 * 8  # L and its inverse


def test_workspace_is_monotone_in_n():
    lib = _lib.load()
    sizes = [workspace(lib, [n]) for n in range(1, 1025)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert workspace(lib, [64, 100]) > workspace(lib, [64, 99]) >= workspace(lib, [64])


def test_null_pointers_are_argument_errors():
    lib = _lib.load()
    for name in ("outs", "train_y", "work", "value", "grad"):
        assert call(lib, **{name: None}) == _lib.DKG_ERR_ARG, name
        assert b"NULL" in lib.dkg_last_error()
    assert call(lib, jitter=None, work_bytes=8) == _lib.DKG_ERR_WORKSPACE  # jitter_used is nullable
    assert call(lib, train_y=(ctypes.c_void_p * 1)(None)) == _lib.DKG_ERR_ARG
    for field in ("inv_lengthscale", "train_x"):
        outs = fake_outputs([64])
        setattr(outs[0], field, None)
        assert call(lib, outs=outs) == _lib.DKG_ERR_ARG, field


def test_bad_sizes():
    lib = _lib.load()
    assert call(lib, m=0) == _lib.DKG_ERR_ARG
    assert call(lib, ns=[16] * 9) == _lib.DKG_ERR_UNSUPPORTED
    assert call(lib, d=0) == _lib.DKG_ERR_ARG
    assert call(lib, d=17) == _lib.DKG_ERR_UNSUPPORTED
    assert call(lib, ns=[0]) == _lib.DKG_ERR_ARG
    assert call(lib, ns=[64, 0]) == _lib.DKG_ERR_ARG
    assert call(lib, ns=[1025]) == _lib.DKG_ERR_UNSUPPORTED
    assert b"> 1024 training points" in lib.dkg_last_error()
    assert call(lib, max_tries=-1) == _lib.DKG_ERR_ARG
    assert call(lib, outs=fake_outputs([64], kernel=4)) == _lib.DKG_ERR_ARG


def test_short_workspace():
    lib = _lib.load()
    need = workspace(lib, [64, 100])
    assert call(lib, ns=[64, 100], work_bytes=need - 1) == _lib.DKG_ERR_WORKSPACE
    assert b"workspace" in lib.dkg_last_error()


def test_not_pd_status_maps_to_linalg_error():
    import torch

    lib = _lib.load()
    call(lib, m=0)  # leaves a message behind
    with pytest.raises(torch.linalg.LinAlgError):
        _lib.check_fit(_lib.DKG_ERR_NOT_PD, "dkg_mll_value_grad")
    with pytest.raises(_lib.BotorchTensorDimensionError):
        _lib.check_fit(_lib.DKG_ERR_ARG, "dkg_mll_value_grad")
    _lib.check_fit(_lib.DKG_OK, "dkg_mll_value_grad")


def test_fit_on_device_needs_a_device():
    from dkg_amd.bo_smoke import _fit_device

    class Problem:
        device = None

    assert _fit_device(Problem(), False) is None
    with pytest.raises(ValueError, match="fit_on_device"):
        _fit_device(Problem(), True)


def test_host_route_is_bit_identical_to_the_parent_commit():
    """fit_map(device=None) on _data(n=60, seed=1): the numbers the commit before the device route gave
    (tests/golden/fit_map_parent.json, floats as hex), every bit of them.  The host BLAS takes another code path per
    CPU family and the 41 L-BFGS-B iterations carry its last-bit differences into the result (1e-11 relative
    between an Intel Xeon and an AMD EPYC 9575F), so the fixture holds the parent's numbers once per family, each
    recorded by running the parent's fit.py there; the result must equal one record in every field."""
    with open(GOLDEN) as f:
        variants = json.load(f)["variants"]
    cfg = reference_model_config(2, [[0, 0], [1, 1]], "always")
    X, y = _data(n=60, seed=1)
    res = fit_map([X, X], [y, 2 * y], cfg, device=None)
    hx = lambda v: [hx(t) for t in v] if isinstance(v, list) else float(v).hex()  # noqa: E731
    keys = ("length_scales", "output_scales", "means", "noises", "mll")
    got = {**{k: hx(res[k]) for k in keys}, "success": res["success"], "iterations": res["iterations"]}
    match = [v["cpu"] for v in variants if all(v[k] == got[k] for k in got)]
    assert match, (got, variants)
