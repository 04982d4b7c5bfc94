"""The host side of the incremental GP state: which models extend a cached one
(gp_state.match_extension, pure host code) and the argument checks of dkg_append_observation, which come
before any HIP call and so need no GPU."""

import ctypes

import pytest
import torch

from dkg_amd import _lib
from dkg_amd.gp_state import match_extension
from dkg_amd.model import ModelListGPState, SingleTaskGPState


def output(n, seed=0, ls=(0.3, 0.7), s=2.0, noise=1e-3, c=0.1, kernel="matern", nu=2.5, n_rows=None, y_std=1.0):
    """The first n rows of a fixed data set (n_rows: how many the generator draws)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n_rows or 12, 2, generator=g, dtype=torch.double)
    y = torch.randn(n_rows or 12, generator=g, dtype=torch.double)
    return SingleTaskGPState(X[:n].clone(), y[:n].clone(), list(ls), s, noise, c, kernel, nu, 0.0, y_std)


def model(n0, n1, **kw):
    return ModelListGPState(output(n0, seed=0, **kw), output(n1, seed=1))


def test_equal_models_add_no_rows():
    assert match_extension(model(8, 9), model(8, 9)) == [0, 0]


def test_one_output_grown_by_one():
    assert match_extension(model(8, 9), model(9, 9)) == [1, 0]
    assert match_extension(model(8, 9), model(8, 10)) == [0, 1]


def test_all_outputs_grown_by_two():
    assert match_extension(model(8, 9), model(10, 11)) == [2, 2]


def test_new_targets_on_a_grown_output_still_match():
    new = model(9, 9)
    new.models[0].train_y = new.models[0].train_y + 1.0  # y' may be wholly new
    assert match_extension(model(8, 9), new) == [1, 0]


def test_changed_targets_without_growth_do_not_match():
    new = model(8, 9)
    new.models[0].train_y = new.models[0].train_y + 1.0
    assert match_extension(model(8, 9), new) is None


@pytest.mark.parametrize("change", [dict(ls=(0.3, 0.70001)), dict(noise=2e-3), dict(kernel="rbf"), dict(nu=1.5),
                                    dict(s=2.5), dict(c=0.2), dict(y_std=2.0)])
def test_changed_hyperparameters_do_not_match(change):
    assert match_extension(model(8, 9), model(9, 9, **change)) is None
    assert match_extension(model(8, 9), model(8, 9, **change)) is None


def test_changed_earlier_row_does_not_match():
    new = model(9, 9)
    new.models[0].train_x[3, 1] += 1e-12
    assert match_extension(model(8, 9), new) is None


def test_shorter_model_does_not_match():
    assert match_extension(model(8, 9), model(7, 9)) is None
    assert match_extension(model(8, 9), model(9, 8)) is None


def test_other_output_count_does_not_match():
    assert match_extension(model(8, 9), ModelListGPState(output(8))) is None


def test_different_discretisation_is_not_extended():
    """shared_state's incremental path looks only at cached entries over an equal discretisation."""
    from dkg_amd import discretekg

    class Entry:  # stands for a cached DeviceGPState: only .model is read before a match
        model = model(8, 9)

        def with_observation(self, *a, **k):
            raise AssertionError("a state over another discretisation must not be extended")

    D = torch.rand(9, 2, dtype=torch.double, generator=torch.Generator().manual_seed(3))
    dev = torch.device("cuda", 0)
    saved = list(discretekg._STATE_CACHE)
    try:
        discretekg._STATE_CACHE[:] = [(None, D.clone(), dev, Entry(), None)]
        assert discretekg._extended_state(model(9, 9), D + 1e-9, dev) is None
        assert discretekg._extended_state(model(9, 9), D[:8], dev) is None
        assert discretekg._extended_state(model(9, 9), D, torch.device("cuda", 1)) is None
        with pytest.raises(AssertionError, match="must not be extended"):
            discretekg._extended_state(model(9, 9), D, dev)  # the equal discretisation is the one that matches
    finally:
        discretekg._STATE_CACHE[:] = saved


def test_switch_and_counters():
    import dkg_amd

    assert dkg_amd.gp_state.incremental_state() is False  # off by default
    assert dkg_amd.set_incremental_state(True) is False
    assert dkg_amd.set_incremental_state(False) is True
    dkg_amd.reset_state_stats()
    assert dkg_amd.state_stats() == {"full_builds": 0, "appends": 0, "append_fallbacks": 0}


# --------------------------------------------------------------------------------------------------
# the C ABI: version, workspace and argument checks (no device call is reached)

def fake_output(n):
    o = _lib.DkgOutput()
    o.n = n
    o.kernel = 2
    o.outputscale, o.noise, o.y_std = 1.0, 1e-3, 1.0
    o.inv_lengthscale = 64  # never dereferenced: the checks come first
    o.disc_frag = 64
    return o


def call(lib, o, **kw):
    a = dict(d=2, L=64, Linv=64, disc=64, N=16, train_x=64, train_y=64, jitter=0.0, L_new=64, Linv_new=64,
             alpha_new=64, root_frag_new=64, disc_frag_new=64, disc_mean_new=64, work=64, work_bytes=1 << 20)
    a.update(kw)
    return lib.dkg_append_observation(o, a["d"], a["L"], a["Linv"], a["disc"], a["N"], a["train_x"], a["train_y"],
                                      a["jitter"], a["L_new"], a["Linv_new"], a["alpha_new"], a["root_frag_new"],
                                      a["disc_frag_new"], a["disc_mean_new"], a["work"], a["work_bytes"], None)


def test_abi_version_is_9():
    assert _lib.ABI_VERSION == 9 and _lib.load().dkg_abi_version() == 9


def test_append_workspace():
    lib = _lib.load()
    assert lib.dkg_append_workspace(64, 256) > 0
    assert lib.dkg_append_workspace(0, 256) == 0 and lib.dkg_append_workspace(64, -1) == 0


def test_null_pointers_are_argument_errors():
    lib = _lib.load()
    assert call(lib, None) == _lib.DKG_ERR_ARG
    for name in ("L", "Linv", "train_x", "train_y", "L_new", "Linv_new", "alpha_new", "root_frag_new", "work",
                 "disc", "disc_frag_new", "disc_mean_new"):
        assert call(lib, fake_output(64), **{name: None}) == _lib.DKG_ERR_ARG, name
        assert b"NULL" in lib.dkg_last_error()
    o = fake_output(64)
    o.inv_lengthscale = None
    assert call(lib, o) == _lib.DKG_ERR_ARG


def test_bad_sizes():
    lib = _lib.load()
    assert call(lib, fake_output(0)) == _lib.DKG_ERR_ARG
    assert call(lib, fake_output(64), N=-1) == _lib.DKG_ERR_ARG
    assert call(lib, fake_output(64), jitter=-1.0) == _lib.DKG_ERR_ARG
    assert call(lib, fake_output(64), d=0) == _lib.DKG_ERR_UNSUPPORTED
    assert call(lib, fake_output(64), work_bytes=8) == _lib.DKG_ERR_WORKSPACE


def test_append_beyond_1024_is_unsupported():
    lib = _lib.load()
    assert call(lib, fake_output(1024)) == _lib.DKG_ERR_UNSUPPORTED
    assert b"> 1024 training points" in lib.dkg_last_error()
