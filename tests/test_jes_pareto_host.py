"""The JES Pareto sampler without a device (dkg_amd.jes_pareto, csrc/dkg_rff.hip, tests/rff_ref.py): the feature
map against the kernel it approximates, the restatement's pruning on hand cases, the argument checks of every new
C entry (they come before any HIP call), the rounding-floor condition of the GPU suite's weight cases, and the
host surface that needs no GPU."""

import ctypes

import numpy as np
import pytest
import torch

import rff_cases
import rff_ref
from dkg_amd import _lib
from dkg_amd.errors import UnsupportedError
from dkg_amd.jes_pareto import draw_rff_randomness, sample_discrete_pareto_optimal_points
from dkg_amd.optim import JesOptimisationSpec

FAKE = 0x1000  # a non-NULL address that must never be followed


# ---------------------------------------------------------------- the feature map

@pytest.mark.parametrize("kid,nu", [(0, 0.5), (1, 1.5), (2, 2.5), (3, None)])
def test_feature_map_approximates_its_kernel(kid, nu):
    """max |phi(x)^T phi(x') - s kappa(x, x')| <= 6 s sqrt(2 / R) at R = 4096 over 40 points: every term of the
    estimator is bounded by 2 s / R, so its standard deviation is at most s sqrt(2 / R).  A wrong Gamma scaling of
    the Matern frequencies fails it."""
    R, d, s = 4096, 3, 1.7
    wn, g, ub, _ = draw_rff_randomness(torch.Generator().manual_seed(11 + kid), [nu], 1, R, d)
    inv_ls = 1.0 / np.array([0.35, 0.6, 0.9])
    om, b = rff_ref.omega_bias(wn[0, 0].numpy(), g[0, 0].numpy(), ub[0, 0].numpy(), inv_ls, kid)
    x = torch.rand(40, d, dtype=torch.double, generator=torch.Generator().manual_seed(5)).numpy()
    phi = rff_ref.features(x, om, b, s)
    err = np.abs(phi @ phi.T - s * rff_ref.kernel(x, x, inv_ls, kid)).max()
    bound = 6.0 * s * np.sqrt(2.0 / R)
    print(f"kernel {kid}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_draws_come_from_the_generator_alone():
    before = torch.random.get_rng_state()
    a = draw_rff_randomness(torch.Generator().manual_seed(3), [2.5, None], 2, 8, 3)
    b = draw_rff_randomness(torch.Generator().manual_seed(3), [2.5, None], 2, 8, 3)
    assert torch.equal(before, torch.random.get_rng_state())
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].shape == (2, 2, 8, 3) and all(t.shape == (2, 2, 8) for t in a[1:])
    assert bool((a[1] > 0).all()) and bool(((a[2] >= 0) & (a[2] < 1)).all())


# ---------------------------------------------------------------- pruning: the restatement on hand cases

def test_prune_hand_cases():
    # a staircase of 5 points, one dominated point (rank 1) and one duplicate of point 1
    F = np.array([[0.0, 4.0], [1.0, 3.0], [2.0, 2.0], [3.5, 1.0], [4.0, 0.0], [0.5, 0.5], [1.0, 3.0]])
    rank = np.array([0, 0, 0, 0, 0, 1, 0])
    assert rff_ref.prune(F, rank, 7) == [0, 1, 2, 3, 4]  # the dominated point and the duplicate (index 6) go
    # crowding of the five: ends inf; 1: (2-0)/4 + (4-2)/4 = 1, 2: 2.5/4 + 2/4 = 1.125, 3: 2/4 + 2/4 = 1
    # -> 1 and 3 tie, the lowest index goes
    assert rff_ref.prune(F, rank, 4) == [0, 2, 3, 4]
    # then 2: (3.5-0)/4 + (4-1)/4 = 1.625 and 3: (4-2)/4 + (2-0)/4 = 1 -> 3 goes
    assert rff_ref.prune(F, rank, 3) == [0, 2, 4]
    assert rff_ref.prune(F, rank, 2) == [0, 4]
    assert rff_ref.prune(F, rank, 1) == [4]  # two ends, both inf: the lowest index goes
    assert rff_ref.prune(F[:1], rank[:1], 3) == [0]
    assert rff_ref.prune(F, np.full(7, -1), 3) == []
    # one objective: the members of rank 0 are the maxima; bit-equal ones collapse to the lowest index
    F1 = np.array([[1.0], [3.0], [3.0], [2.0]])
    assert rff_ref.prune(F1, np.array([1, 0, 0, 1]), 5) == [1]


def test_prune_crowding_is_the_ranks():
    """rff_ref.crowding on a front equals pareto_ref's crowding of that front, bit for bit."""
    import pareto_ref

    g = np.random.default_rng(0)
    t = np.sort(g.random(12))
    F = np.stack([t, 1.0 - t ** 2, g.random(12)], -1)
    rank, crowd, _ = pareto_ref.rank_crowd_order(F)
    front = np.flatnonzero(rank == 0)
    assert rff_ref.crowding(F[front]).tobytes() == crowd[front].tobytes()


# ---------------------------------------------------------------- argument checks, before any HIP call

def paths_struct(S=2, m=2, d=2, R=64, ptr=FAKE):
    return _lib.DkgRffPaths(S, m, d, R, ptr, ptr, ptr, ptr)


def status(call):
    return call, _lib.load().dkg_last_error().decode()


def test_new_symbols_are_declared_and_bound():
    header = open(_lib.__file__.replace("decoupled-kg_amd/dkg_amd/_lib.py", "include/dkg.h")).read()
    lib = _lib.load()
    for name in ("dkg_rff_workspace", "dkg_rff_weights", "dkg_rff_eval", "dkg_pareto_paths_workspace",
                 "dkg_pareto_nsga2_paths", "dkg_pareto_prune", "dkg_debug_rff_gram"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.DkgRffPaths) == 16 + 4 * 8
    assert "#define DKG_RFF_EVAL_LDS_BYTES" in header and 1024 * (16 + 2) * 8 <= 160 * 1024


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.dkg_rff_workspace(0, 10) == 0 and lib.dkg_rff_workspace(1025, 10) == 0
    assert lib.dkg_rff_workspace(64, 0) == 0 and lib.dkg_rff_workspace(64, 1025) == 0
    assert lib.dkg_rff_workspace(512, 256) >= 8 * (2 * 512 * 512 + 256 * 512) * 8
    assert lib.dkg_pareto_paths_workspace(0, 8, 2, 2) == 0 and lib.dkg_pareto_paths_workspace(65, 8, 2, 2) == 0
    assert lib.dkg_pareto_paths_workspace(2, 10, 2, 2) == 0 and lib.dkg_pareto_paths_workspace(2, 1028, 2, 2) == 0
    assert lib.dkg_pareto_paths_workspace(2, 8, 17, 2) == 0 and lib.dkg_pareto_paths_workspace(2, 8, 2, 9) == 0
    assert lib.dkg_pareto_paths_workspace(3, 100, 2, 2) >= 3 * 200 * (2 + 2 + 1) * 8 + 2 * 3 * 200 * 4


def test_rff_eval_refusals():
    lib = _lib.load()
    ev = lambda p, x=FAKE, P=4, F=FAKE: lib.dkg_rff_eval(p, x, P, 0, F, None)  # noqa: E731
    assert ev(None) == _lib.DKG_ERR_ARG
    assert ev(paths_struct(S=0)) == _lib.DKG_ERR_ARG
    assert ev(paths_struct(S=65)) == _lib.DKG_ERR_UNSUPPORTED
    assert ev(paths_struct(m=9)) == _lib.DKG_ERR_UNSUPPORTED
    assert ev(paths_struct(d=17)) == _lib.DKG_ERR_UNSUPPORTED
    assert ev(paths_struct(R=1025)) == _lib.DKG_ERR_UNSUPPORTED
    assert "R=1025" in lib.dkg_last_error().decode()
    assert ev(paths_struct(ptr=0)) == _lib.DKG_ERR_ARG
    assert ev(paths_struct(), P=-1) == _lib.DKG_ERR_ARG
    assert ev(paths_struct(), x=None) == _lib.DKG_ERR_ARG and ev(paths_struct(), F=None) == _lib.DKG_ERR_ARG
    assert ev(paths_struct(), P=0) == _lib.DKG_OK  # a no-op: nothing is read


def one_output(n=5, kernel=2, noise=1e-2, s=1.0):
    o = _lib.DkgOutput()
    o.n, o.kernel, o.outputscale, o.noise, o.y_std = n, kernel, s, noise, 1.0
    o.inv_lengthscale = o.train_x = FAKE
    return o


def test_rff_weights_refusals():
    lib = _lib.load()

    def call(outs=None, m=1, d=2, ys=(FAKE,), wn=FAKE, g=FAKE, p=None, work=FAKE, wbytes=1 << 40, tries=3):
        outs = (_lib.DkgOutput * 1)(one_output()) if outs is None else outs
        p = paths_struct(m=1) if p is None else p
        y = (ctypes.c_void_p * len(ys))(*ys)
        return lib.dkg_rff_weights(outs, m, d, y, wn, g, FAKE, FAKE, tries, p, work, wbytes, None, None)

    assert call(p=paths_struct(m=1, R=1025)) == _lib.DKG_ERR_UNSUPPORTED
    assert call(p=paths_struct(m=1, S=65)) == _lib.DKG_ERR_UNSUPPORTED
    assert call(d=3) == _lib.DKG_ERR_ARG  # d against the paths'
    assert call(wn=None) == _lib.DKG_ERR_ARG and call(work=None) == _lib.DKG_ERR_ARG
    assert call(tries=-1) == _lib.DKG_ERR_ARG
    assert call(ys=(None,)) == _lib.DKG_ERR_ARG
    assert call(outs=(_lib.DkgOutput * 1)(one_output(n=0))) == _lib.DKG_ERR_ARG
    assert call(outs=(_lib.DkgOutput * 1)(one_output(n=1025))) == _lib.DKG_ERR_UNSUPPORTED
    assert call(outs=(_lib.DkgOutput * 1)(one_output(kernel=4))) == _lib.DKG_ERR_ARG
    assert call(outs=(_lib.DkgOutput * 1)(one_output(noise=0.0))) == _lib.DKG_ERR_ARG
    assert call(g=None) == _lib.DKG_ERR_ARG  # a Matern output needs its Gamma draws
    assert call(wbytes=1024) == _lib.DKG_ERR_WORKSPACE
    assert "workspace" in lib.dkg_last_error().decode()


def test_nsga2_paths_refusals():
    lib = _lib.load()
    prm = _lib.DkgNsga2Params(0.9, 15.0, 0.5, 20.0)

    def call(p=None, lb=FAKE, P=8, gens=1, prm=prm, work=FAKE, wbytes=1 << 40):
        p = paths_struct() if p is None else p
        return lib.dkg_pareto_nsga2_paths(p, lb, FAKE, P, gens, prm, FAKE, FAKE, FAKE, FAKE, FAKE, work, wbytes, None)

    assert call(p=paths_struct(S=65)) == _lib.DKG_ERR_UNSUPPORTED
    assert call(P=10) == _lib.DKG_ERR_ARG and call(P=4) == _lib.DKG_ERR_ARG
    assert call(P=1028) == _lib.DKG_ERR_UNSUPPORTED
    assert call(gens=-1) == _lib.DKG_ERR_ARG
    assert call(prm=None) == _lib.DKG_ERR_ARG
    assert call(prm=_lib.DkgNsga2Params(1.5, 15.0, 0.5, 20.0)) == _lib.DKG_ERR_ARG
    assert call(lb=None) == _lib.DKG_ERR_ARG and call(work=None) == _lib.DKG_ERR_ARG
    assert call(wbytes=16) == _lib.DKG_ERR_WORKSPACE


def test_prune_refusals():
    lib = _lib.load()
    pr = lambda F=FAKE, S=1, Q=8, m=2, k=3, cnt=FAKE: lib.dkg_pareto_prune(F, FAKE, S, Q, m, k, cnt, FAKE, None)  # noqa
    assert pr(S=0) == _lib.DKG_ERR_ARG and pr(Q=0) == _lib.DKG_ERR_ARG and pr(k=0) == _lib.DKG_ERR_ARG
    assert pr(S=65) == _lib.DKG_ERR_UNSUPPORTED and pr(Q=2049) == _lib.DKG_ERR_UNSUPPORTED
    assert pr(m=9) == _lib.DKG_ERR_UNSUPPORTED and pr(k=2049) == _lib.DKG_ERR_UNSUPPORTED
    assert pr(F=None) == _lib.DKG_ERR_ARG and pr(cnt=None) == _lib.DKG_ERR_ARG


def test_debug_rff_gram_switch():
    lib = _lib.load()
    assert lib.dkg_debug_rff_gram(-1) == 0  # the MFMA tiles are the default
    assert lib.dkg_debug_rff_gram(1) == 0 and lib.dkg_debug_rff_gram(0) == 1 and lib.dkg_debug_rff_gram(-1) == 0
    assert lib.dkg_debug_rff_gram(2) == -2


# ---------------------------------------------------------------- the GPU suite's cases meet the floor condition

@pytest.mark.parametrize("name", list(rff_cases.WEIGHT_CASES))
def test_weight_cases_meet_the_rounding_floor_condition(name):
    """Every case the GPU suite asserts has spread <= 1e-6 y_std sqrt(s): the restatement itself pins the path that
    well (rows as given against rows reversed).  At noise 1e-8 it does not (9.5e-5 against 7.1e-6 at s = 50,
    l = 0.2): the linear system is that ill-conditioned on the reference side too, and no such case is asserted."""
    state, _, _, _, spread = rff_cases.weight_case(name)
    cap = rff_cases.spread_cap(state)
    print(f"{name}: spread {spread.max(0)}, cap {cap}")
    assert (spread <= cap[None, :]).all()


# ---------------------------------------------------------------- host surface

def test_maximize_false_is_refused():
    with pytest.raises(UnsupportedError):
        sample_discrete_pareto_optimal_points(None, torch.tensor([[0.0], [1.0]]), 1, 1, maximize=False)


def test_spec_constructor_is_unchanged_and_has_the_device_sampler():
    with pytest.raises(TypeError):
        JesOptimisationSpec("LB", 2, 3, 1, 4, 1, 5, pareto_sampler=None)
    spec = JesOptimisationSpec.with_device_sampler("LB2", 3, 5, 2, 8, 1, 10, seed=4, nsga2_generations=7)
    assert isinstance(spec, JesOptimisationSpec) and callable(spec.pareto_sampler)
    assert (spec.estimation_type, spec.num_pareto_samples, spec.num_pareto_points, spec.seed) == ("LB2", 3, 5, 4)
