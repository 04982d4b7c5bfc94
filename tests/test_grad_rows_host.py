"""Global rows for the gradient plan (DKG_PLAN_GRAD_GLOBAL_ROWS / DKG_PLAN_FORCE_GLOBAL_ROWS), the parts that need
no device: dkg_plan_grad_rows against dkg_plan_init's own refusal rule, the flag checks, and the Python switch.

CPU-only: dkg_plan_init is only driven into returns that come before any device work (its refusals, or
DKG_ERR_WORKSPACE from a zero-byte workspace, which is checked after every refusal), with fake non-NULL pointers
that are never followed, as in tests/test_native_abi.py.
"""

import ctypes

import pytest

import dkg_amd
from dkg_amd import _lib

GRAD, F32 = _lib.DKG_PLAN_GRAD, _lib.DKG_PLAN_F32

# (m, d, n, N, S)
SHAPES = [
    (2, 2, 256, 1024, 16),
    (2, 2, 1024, 121, 16),
    (2, 6, 640, 64, 8),
    (2, 6, 800, 64, 8),
    (3, 2, 1024, 4096, 32),
    (3, 2, 1024, 50, 32),
    (8, 16, 128, 50, 8),
    (8, 16, 256, 50, 8),
    (1, 1, 16, 10, 1),
]
# rows whose staged gradient plan is refused for the gradient's LDS: M (d + 1) stage_len(n_pad) + 8 n_pad doubles
# beside the lists exceed 160 KiB (confirmed on a build without the global-rows flags)
REFUSED = {3, 4, 5, 6, 7}


def _outs(m, n):
    outs = (_lib.DkgOutput * m)()
    for o in outs:
        o.n, o.kernel = n, 2
        for f in ("inv_lengthscale", "train_x", "alpha", "root_frag", "disc_frag", "disc_mean"):
            setattr(o, f, 16)
    return outs


def _init(outs, m, d, N, S, flags, workspace_bytes=0):
    """dkg_plan_init up to its workspace check (a zero-byte workspace: no device work follows)."""
    lib = _lib.load()
    host = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    st = lib.dkg_plan_init(outs, m, d, 16, N, 16, S, -1, 4, flags, 16, workspace_bytes, host, 16, None)
    return st, lib.dkg_last_error()


@pytest.mark.parametrize("row", range(len(SHAPES)), ids=[f"m{m}-d{d}-n{n}-N{N}-S{S}" for m, d, n, N, S in SHAPES])
def test_plan_grad_rows_is_the_plan_rule(row):
    lib = _lib.load()
    m, d, n, N, S = SHAPES[row]
    outs = _outs(m, n)
    # the staged plan of this build: refused for the gradient's LDS, or through to the workspace check
    st, msg = _init(outs, m, d, N, S, GRAD)
    refused = st == _lib.DKG_ERR_UNSUPPORTED
    assert (refused and b"gradient" in msg) or st == _lib.DKG_ERR_WORKSPACE, (st, msg)
    assert refused == (row in REFUSED)
    got = lib.dkg_plan_grad_rows(outs, m, d, N, S, GRAD)
    if refused:
        assert got == -_lib.DKG_ERR_UNSUPPORTED
        assert b"gradient" in lib.dkg_last_error()
    else:
        assert got == 0
    # DKG_PLAN_GRAD_GLOBAL_ROWS: global rows exactly where the staged plan is refused, and the plan then builds
    assert lib.dkg_plan_grad_rows(outs, m, d, N, S, GRAD | _lib.DKG_PLAN_GRAD_GLOBAL_ROWS) == (1 if refused else 0)
    assert _init(outs, m, d, N, S, GRAD | _lib.DKG_PLAN_GRAD_GLOBAL_ROWS)[0] == _lib.DKG_ERR_WORKSPACE
    # DKG_PLAN_FORCE_GLOBAL_ROWS: always
    assert lib.dkg_plan_grad_rows(outs, m, d, N, S, GRAD | _lib.DKG_PLAN_FORCE_GLOBAL_ROWS) == 1
    assert _init(outs, m, d, N, S, GRAD | _lib.DKG_PLAN_FORCE_GLOBAL_ROWS)[0] == _lib.DKG_ERR_WORKSPACE


def test_workspace_does_not_depend_on_the_rows_flags():
    """The variant reads buffers the gradient plan already has: the same workspace with and without the flags."""
    lib = _lib.load()
    for m, d, n, N, S in SHAPES:
        outs = _outs(m, n)
        base = lib.dkg_plan_workspace(outs, m, d, N, 4, S, GRAD)
        assert base > 0
        for f in (_lib.DKG_PLAN_GRAD_GLOBAL_ROWS, _lib.DKG_PLAN_FORCE_GLOBAL_ROWS):
            assert lib.dkg_plan_workspace(outs, m, d, N, 4, S, GRAD | f) == base
            assert lib.dkg_plan_workspace_targets(outs, m, d, N, 4, S, m + 1, GRAD | f) == \
                lib.dkg_plan_workspace_targets(outs, m, d, N, 4, S, m + 1, GRAD)


def test_plan_flag_checks():
    lib = _lib.load()
    assert _lib.DKG_PLAN_GRAD_GLOBAL_ROWS == 32 and _lib.DKG_PLAN_FORCE_GLOBAL_ROWS == 128
    outs = _outs(2, 256)
    for f in (32, 128):
        # meaningless without the gradient
        st, msg = _init(outs, 2, 2, 1024, 16, f)
        assert st == _lib.DKG_ERR_ARG and b"DKG_PLAN_GRAD" in msg
        assert lib.dkg_plan_grad_rows(outs, 2, 2, 1024, 16, f) == -_lib.DKG_ERR_ARG
        # the fp32 plan is forward only, with or without them
        st, msg = _init(outs, 2, 2, 1024, 16, GRAD | F32 | f)
        assert st == _lib.DKG_ERR_UNSUPPORTED and b"forward only" in msg
        assert lib.dkg_plan_grad_rows(outs, 2, 2, 1024, 16, GRAD | F32 | f) == -_lib.DKG_ERR_UNSUPPORTED
    st, msg = _init(outs, 2, 2, 1024, 16, 64)
    assert st == _lib.DKG_ERR_ARG and b"unknown plan flags" in msg
    st, msg = _init(outs, 2, 2, 1024, 16, GRAD | 64)
    assert st == _lib.DKG_ERR_ARG and b"unknown plan flags" in msg
    assert lib.dkg_plan_grad_rows(outs, 2, 2, 1024, 16, GRAD | 64) == -_lib.DKG_ERR_ARG
    assert lib.dkg_plan_grad_rows(None, 2, 2, 1024, 16, GRAD) == -_lib.DKG_ERR_ARG
    assert lib.dkg_abi_version() == 9 == _lib.ABI_VERSION
    # a plan never initialised stages (has no gradient at all)
    blank = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    assert lib.dkg_plan_grad_rows_of(blank) == 0 and lib.dkg_plan_grad_rows_of(None) == 0


def test_python_switch():
    assert dkg_amd.gradient_rows() == "staged"
    try:
        assert dkg_amd.set_gradient_rows("auto") == "staged"
        assert dkg_amd.gradient_rows() == "auto"
        assert dkg_amd.set_gradient_rows("global") == "auto"
        with pytest.raises(ValueError):
            dkg_amd.set_gradient_rows("lds")
        assert dkg_amd.gradient_rows() == "global"  # a rejected value changes nothing
        assert dkg_amd.set_gradient_rows("staged") == "global"
    finally:
        dkg_amd.set_gradient_rows("staged")
    assert dkg_amd.gradient_rows() == "staged"


def test_unsupported_message_names_the_switch():
    """The refusal for the gradient's LDS keeps its text in front and names the opt-in after it."""
    from dkg_amd.errors import UnsupportedError

    st, _ = _init(_outs(8, 256), 8, 16, 50, 8, GRAD)
    with pytest.raises(UnsupportedError, match=r'gradient: m=8 outputs.*LDS.*set_gradient_rows\("auto"\)'):
        _lib.check(st, "dkg_plan_init")
    # other refusals are not touched
    st, _ = _init(_outs(2, 256), 2, 2, 1024, 16, GRAD | F32)
    with pytest.raises(UnsupportedError) as e:
        _lib.check(st, "dkg_plan_init")
    assert "set_gradient_rows" not in str(e.value)
