"""Host side of the wide Pareto-rank path (no GPU): the workspace entry, dkg_pareto_rank's argument checks with a
workspace, dkg_pareto_nsga2's grown carve, the debug switch, and the closed forms the GPU tests lean on
(tests/pareto_wide_ref.py) against the numpy restatement."""

import numpy as np
import pytest

import pareto_ref
import pareto_wide_ref
from dkg_amd import _lib

MAXQ = 16384


def test_rank_workspace_limits_and_growth():
    w = _lib.load().dkg_pareto_rank_workspace
    assert w(0, 2) == 0 and w(MAXQ + 1, 2) == 0 and w(8, 0) == 0 and w(8, 9) == 0
    sizes = [w(Q, 2) for Q in (1, 2, 63, 64, 65, 2048, 2049, 4097, MAXQ)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert w(MAXQ, 8) >= 2 * MAXQ * 4  # cnt [Q] and rk [Q] ints
    assert all(w(100, m) > 0 for m in range(1, 9))


def test_rank_argument_checks_with_a_workspace():
    lib = _lib.load()
    need = lib.dkg_pareto_rank_workspace(2049, 2)

    def rank(F=16, Q=2049, m=2, keep=1, work=16, nbytes=1 << 30):
        return lib.dkg_pareto_rank(F, Q, m, keep, 16, 16, 16, work, nbytes, None)

    assert rank(nbytes=need - 1) == _lib.DKG_ERR_WORKSPACE and b"workspace" in lib.dkg_last_error()
    assert rank(Q=64, nbytes=lib.dkg_pareto_rank_workspace(64, 2) - 1) == _lib.DKG_ERR_WORKSPACE
    assert rank(Q=MAXQ + 1) == _lib.DKG_ERR_UNSUPPORTED and b"16384" in lib.dkg_last_error()
    assert rank(keep=0) == _lib.DKG_ERR_ARG
    assert rank(keep=2050) == _lib.DKG_ERR_ARG
    assert rank(F=None) == _lib.DKG_ERR_ARG
    assert rank(m=9) == _lib.DKG_ERR_UNSUPPORTED
    # without a workspace the limit is the one-workgroup kernel's, whatever work_bytes says
    assert rank(work=None) == _lib.DKG_ERR_UNSUPPORTED and b"2048" in lib.dkg_last_error()


def parent_nsga2_carve(P, d, m):
    """The carve of dkg_pareto_nsga2 without the rank scratch (gen_ws in csrc/dkg_pareto.hip, one population): the
    evaluator normalises the points itself, so there is no section for normalised points."""
    up = lambda x: (x + 255) & ~255  # noqa: E731
    off = up(2 * P * d * 8)
    off = up(off + 2 * P * m * 8)
    off = up(off + 2 * P * 8)
    off = up(off + 2 * P * 4)
    return up(off + 2 * P * 4)


@pytest.mark.parametrize("P,d,m", [(8, 1, 1), (12, 2, 2), (100, 2, 2), (1000, 2, 2), (1024, 16, 8)])
def test_nsga2_workspace_holds_the_rank_scratch(P, d, m):
    lib = _lib.load()
    assert lib.dkg_pareto_workspace(P, d, m) >= parent_nsga2_carve(P, d, m) + lib.dkg_pareto_rank_workspace(2 * P, m)
    assert lib.dkg_pareto_rank_workspace(2 * P, m) > 0


def test_debug_switch_returns_the_previous_mode_and_restores():
    lib = _lib.load()
    first = lib.dkg_debug_pareto_wide(1)
    try:
        assert first == -1  # the rule is the default
        assert lib.dkg_debug_pareto_wide(0) == 1
        assert lib.dkg_debug_pareto_wide(-1) == 0
        assert lib.dkg_debug_pareto_wide(2) == -2 and b"mode=2" in lib.dkg_last_error()
        assert lib.dkg_debug_pareto_wide(-5) == -2
        assert lib.dkg_debug_pareto_wide(-1) == -1  # a refused mode changed nothing
    finally:
        lib.dkg_debug_pareto_wide(first)
    assert lib.dkg_debug_pareto_wide(first) == first


def test_abi_version_is_unchanged():
    assert _lib.load().dkg_abi_version() == 9 == _lib.ABI_VERSION


@pytest.mark.parametrize("keep", [256, 128, 65, 64, 1])
def test_tiled_closed_form_against_the_restatement(keep):
    base = pareto_wide_ref.tiled_base()
    assert base.shape == (64, 2) and (base >= 0).all() and (base < 1).all()
    assert (base * 1024 == np.round(base * 1024)).all()
    F = pareto_wide_ref.tiled_input(base, 4)
    assert F.shape == (256, 2) and (F[64:128] == base + 4.0).all()
    r, c, o = pareto_ref.rank_crowd_order(F, keep)
    er, ec, eo = pareto_wide_ref.tiled_expected(base, 4, keep)
    assert er.tolist() == r.tolist() and ec.tobytes() == c.tobytes() and eo.tolist() == o.tolist()


@pytest.mark.parametrize("kind", ["gauss", "grid", "chain", "equal"])
def test_cut_to_keep_against_the_restatement(kind):
    g = np.random.default_rng(3)
    Q = 97
    F = {"gauss": g.standard_normal((Q, 3)), "grid": g.integers(0, 4, size=(Q, 2)).astype(np.float64),
         "chain": np.repeat(np.arange(Q, dtype=np.float64)[:, None], 2, 1), "equal": np.full((Q, 2), 0.5)}[kind]
    full = pareto_ref.rank_crowd_order(F, Q)
    for keep in (Q, Q // 2, 7, 1):
        r, c, o = pareto_ref.rank_crowd_order(F, keep)
        er, ec, eo = pareto_wide_ref.cut_to_keep(*full, keep)
        assert er.tolist() == r.tolist() and ec.tobytes() == c.tobytes() and eo.tolist() == o.tolist(), keep
