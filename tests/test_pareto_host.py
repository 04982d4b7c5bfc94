"""Host side of the device NSGA-II and the BO metrics (no GPU): the numpy restatement the GPU tests compare
against (tests/pareto_ref.py) on hand cases, the exact hypervolume and the two estimators of dkg_amd.metrics, the
argument validation of the new C entries, and the committed quality yardstick."""

import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import pareto_ref
from dkg_amd import _lib, metrics

INF = np.inf
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- rank, crowding, order

def slow_rank_crowd_order(F, keep):
    """The specification in plain loops (independent of pareto_ref's vectorised form)."""
    Q, m = F.shape

    def dom(a, b):
        return all(a[j] >= b[j] for j in range(m)) and any(a[j] > b[j] for j in range(m))

    rank = [-1] * Q
    left, r, done = set(range(Q)), 0, 0
    while done < keep and left:
        front = [i for i in sorted(left) if not any(dom(F[k], F[i]) for k in left)]
        for i in front:
            rank[i] = r
        left -= set(front)
        done += len(front)
        r += 1
    crowd = [0.0] * Q
    for fr in range(r):
        mem = [i for i in range(Q) if rank[i] == fr]
        for j in range(m):
            s = sorted(mem, key=lambda i: (F[i, j], i))
            rng = F[s[-1], j] - F[s[0], j]
            for pos, i in enumerate(s):
                if pos == 0 or pos == len(s) - 1:
                    crowd[i] = crowd[i] + INF
                else:
                    crowd[i] = crowd[i] + ((F[s[pos + 1], j] - F[s[pos - 1], j]) / rng if rng > 0 else 0.0)
    ranked = sorted((i for i in range(Q) if rank[i] >= 0), key=lambda i: (rank[i], -crowd[i], i))
    return np.array(rank), np.array(crowd), np.array(ranked + [-1] * (Q - len(ranked)))


def check_same(F, keep=None):
    F = np.asarray(F, dtype=np.float64)
    keep = F.shape[0] if keep is None else keep
    rank, crowd, order = pareto_ref.rank_crowd_order(F, keep)
    r2, c2, o2 = slow_rank_crowd_order(F, keep)
    assert rank.tolist() == r2.tolist()
    assert crowd.tobytes() == c2.astype(np.float64).tobytes()
    assert order.tolist() == o2.tolist()
    return rank, crowd, order


def test_textbook_two_objective_fronts():
    F = [(1, 5), (2, 4), (3, 3), (4, 2), (5, 1), (1, 4), (2, 3), (3, 2), (1, 1)]
    rank, crowd, order = check_same(F)
    assert rank.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 2]
    assert crowd[[0, 4, 5, 7, 8]].tolist() == [INF] * 5
    assert crowd[[1, 2, 3]].tolist() == [1.0, 1.0, 1.0]  # (3 - 1) / 4 + (5 - 3) / 4
    assert crowd[6] == 2.0  # (3 - 1) / 2 + (4 - 2) / 2
    assert order.tolist() == [0, 4, 1, 2, 3, 5, 7, 6, 8]
    # keep: the front that reaches `keep` is ranked whole, the rest -1 with crowding 0
    rank, crowd, order = check_same(F, keep=6)
    assert rank.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, -1] and crowd[8] == 0.0 and order[-1] == -1
    rank, crowd, order = check_same(F, keep=1)
    assert rank.tolist() == [0] * 5 + [-1] * 4 and order[:5].tolist() == [0, 4, 1, 2, 3]


def test_all_equal_points_share_front_zero():
    F = np.full((7, 3), 2.5)
    rank, crowd, order = check_same(F)
    assert rank.tolist() == [0] * 7
    assert crowd.tolist() == [INF, 0, 0, 0, 0, 0, INF]  # ends by index; a zero range adds 0
    assert order.tolist() == [0, 6, 1, 2, 3, 4, 5]


def test_dominance_chain_gives_one_front_per_point():
    Q = 33
    F = np.stack([np.arange(Q), np.arange(Q)], -1).astype(float)
    rank, crowd, order = check_same(F)
    assert rank.tolist() == list(range(Q - 1, -1, -1)) and np.isinf(crowd).all()
    assert order.tolist() == list(range(Q - 1, -1, -1))
    rank, _, order = check_same(F, keep=1)
    assert rank.tolist() == [-1] * (Q - 1) + [0] and order.tolist() == [Q - 1] + [-1] * (Q - 1)
    one = pareto_ref.rank_crowd_order(np.arange(5.0)[::-1].reshape(5, 1))  # m = 1: a total order
    assert one[0].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("m", [2, 3])
def test_integer_grid_with_single_objective_ties(m):
    g = np.random.default_rng(m)
    F = g.integers(0, 4, size=(60, m)).astype(float)  # many ties in one objective, duplicated rows
    for keep in (60, 30, 1):
        check_same(F, keep)


def test_crowding_with_a_zero_range():
    F = np.array([(1, 1, 4), (1, 2, 3), (1, 3, 2), (1, 4, 1)], dtype=float)  # f_0 constant over the front
    rank, crowd, _ = check_same(F)
    assert rank.tolist() == [0] * 4
    assert crowd.tolist() == [INF, 0.0 + 2 / 3 + 2 / 3, 0.0 + 2 / 3 + 2 / 3, INF]


# ---------------------------------------------------------------- variation and the run

def _population(P, d, seed):
    g = np.random.default_rng(seed)
    lb, ub = -1.0 - g.random(d), 1.0 + g.random(d)
    X = lb + g.random((P, d)) * (ub - lb)
    rank, crowd, _ = pareto_ref.rank_crowd_order(g.standard_normal((P, 2)))
    return X, rank, crowd, lb, ub, g.random(pareto_ref.draws(P, d))


def test_variation_copies_winners_without_crossover_and_mutation():
    X, rank, crowd, lb, ub, u = _population(12, 3, 0)
    C = pareto_ref.variation(X, rank, crowd, lb, ub, u, cr=0.0, eta_c=10.0, m=0.0, eta_m=50.0)
    assert C.tobytes() == X[pareto_ref.tournament_winners(rank, crowd, u, 12)].tobytes()


def test_variation_stays_in_bounds_and_moves_points():
    X, rank, crowd, lb, ub, u = _population(64, 4, 1)
    C = pareto_ref.variation(X, rank, crowd, lb, ub, u, cr=1.0, eta_c=10.0, m=1.0, eta_m=50.0)
    assert (C >= lb).all() and (C <= ub).all() and np.isfinite(C).all()
    W = X[pareto_ref.tournament_winners(rank, crowd, u, 64)]
    assert (C != W).mean() > 0.9
    # crossover alone: a crossed coordinate's children straddle or stay near the parents' interval, about half of
    # the coordinates are crossed, the others are copies
    C = pareto_ref.variation(X, rank, crowd, lb, ub, u, cr=1.0, eta_c=10.0, m=0.0, eta_m=50.0)
    assert 0.25 < (C == W).mean() < 0.75


def test_tournament_prefers_rank_then_crowding_then_the_first_drawn():
    rank = np.array([0, 1, 1, 1], dtype=np.int32)
    crowd = np.array([0.0, 5.0, 7.0, 7.0])
    P = 4
    u = np.array([0.3, 0.1, 0.3, 0.6, 0.6, 0.8, 0.8, 0.6]) + 0.01  # pairs (1,0) (1,2) (2,3) (3,2)
    assert pareto_ref.tournament_winners(rank, crowd, u, P).tolist() == [0, 2, 2, 3]


def test_run_is_elitist_and_deterministic():
    lb, ub = np.zeros(2), np.ones(2)

    def fit(X):  # a concave two-objective trade-off
        return np.stack([-(X ** 2).sum(-1), -((X - 1.0) ** 2).sum(-1)], -1)

    u = pareto_ref.uniforms(3, 24, 2, 10)
    hist = []
    X, F, rank, crowd = pareto_ref.run(fit, lb, ub, 24, 10, u, history=hist, **pareto_ref.DEFAULTS)
    X2, F2, *_ = pareto_ref.run(fit, lb, ub, 24, 10, u, **pareto_ref.DEFAULTS)
    assert X.tobytes() == X2.tobytes() and F.tobytes() == F2.tobytes()
    ref = np.array([-2.5, -2.5])
    hv = [pareto_ref.hypervolume_2d(f[r == 0], ref) for _, f, r in hist]
    assert hv[-1] > hv[0]
    # (mu + lambda) with infinite crowding at a front's ends never loses the best value of an objective
    best = np.array([f.max(0) for _, f, _ in hist])
    assert (np.diff(best, axis=0) >= 0).all()
    assert (rank >= 0).all() and (np.diff(rank) >= 0).all()  # survivors come out in order order


# ---------------------------------------------------------------- exact hypervolume

def test_hypervolume_two_objective_staircases():
    assert metrics.hypervolume([(3, 1), (2, 2), (1, 3)], [0, 0]) == 6.0
    assert metrics.hypervolume([(3, 1), (2, 2), (1, 3), (1, 1), (2, 2)], [0, 0]) == 6.0  # dominated, duplicate
    assert metrics.hypervolume([(4.0, 2.0)], [1.0, 1.0]) == 3.0
    assert pareto_ref.hypervolume_2d([(3, 1), (2, 2), (1, 3)], [0, 0]) == 6.0
    assert metrics.hypervolume([(2.0,), (5.0,)], [1.0]) == 4.0


def test_hypervolume_ignores_points_outside_the_reference_point():
    assert metrics.hypervolume([(3, -1), (-1, 3), (0, 5)], [0, 0]) == 0.0
    assert metrics.hypervolume([(3, 1), (5, 0), (-2, 9)], [0, 0]) == 3.0
    lo, hi = metrics.estimate_hypervolume(torch.tensor([(3.0, -1.0)]), torch.tensor([0.0, 0.0]))
    assert lo == 0.0 and hi == 0


def inclusion_exclusion(P, ref):
    hv = 0.0
    for k in range(1, len(P) + 1):
        for S in itertools.combinations(range(len(P)), k):
            side = np.clip(P[list(S)].min(0) - ref, 0.0, None)
            hv += (-1) ** (k + 1) * side.prod()
    return hv


@pytest.mark.parametrize("m", [3, 4])
def test_hypervolume_against_inclusion_exclusion(m):
    g = np.random.default_rng(10 + m)
    for n in (1, 4, 10):
        P = g.random((n, m)) * 2.0 - 0.3  # some points outside the reference point
        ref = np.zeros(m)
        want = inclusion_exclusion(P[(P > ref).all(-1)], ref)
        assert metrics.hypervolume(P, ref) == pytest.approx(want, rel=1e-12, abs=1e-14)


@pytest.mark.parametrize("m", [2, 3])
def test_hypervolume_bounds_on_an_integer_lattice(m):
    g = np.random.default_rng(m)
    P = g.integers(1, 6, size=(9, m))
    P = P[~pareto_ref.dominance_matrix(P).any(0)]  # a front: the upper bound is one only for non-dominated samples
    assert len(P) >= 2
    ideal = P.max(0)
    cells = list(itertools.product(*[range(k) for k in ideal]))  # unit cells of the box (0, ideal], lower corners
    lower = sum(any((p >= np.array(c) + 1).all() for p in P) for c in cells)
    beyond = sum(any((np.array(c) >= p).all() for p in P) for c in cells)  # cells no sampled front could reach
    lo, hi = metrics.estimate_hypervolume(torch.tensor(P, dtype=torch.double), torch.zeros(m, dtype=torch.double))
    assert lo == float(lower) and hi == float(len(cells) - beyond) and lo <= hi
    assert metrics.estimate_hypervolume(torch.tensor(P, dtype=torch.double), torch.zeros(m), return_upper=False) == lo


def test_reference_point():
    F = torch.tensor([[1.0, 10.0], [3.0, 0.0]])
    assert metrics.calculate_reference_point(F).tolist() == [1.0 - 0.02, 0.0 - 0.1]
    from dkg_amd.errors import BotorchTensorDimensionError
    with pytest.raises(BotorchTensorDimensionError):
        metrics.calculate_reference_point(torch.zeros(3))


# ---------------------------------------------------------------- the two estimators

class QuadraticProblem:
    num_objectives = 2

    def __call__(self, X):
        X = torch.as_tensor(X)
        return torch.stack([-(X ** 2).sum(-1), -((X - 1.0) ** 2).sum(-1)], -1)


def test_estimators_against_the_formulas():
    from dkg_amd.utils import sample_simplex

    g = torch.Generator().manual_seed(5)
    pset = torch.rand(20, 2, generator=g, dtype=torch.double)
    front = torch.rand(20, 2, generator=g, dtype=torch.double)
    front[7] = front[3]  # tied maxima: the first index is the recommendation
    front[3, 0] = front[7, 0] = 2.0
    problem = QuadraticProblem()
    W = sample_simplex(2, 1024, qmc=True, seed=11, dtype=torch.double)
    scal = (front.unsqueeze(0) * W.unsqueeze(1)).sum(-1)  # [1024, 20]
    rec = [int(np.flatnonzero(row == row.max())[0]) for row in scal.numpy()]
    assert 3 in rec and 7 not in rec
    predicted = float(np.mean([scal[i, r].item() for i, r in enumerate(rec)]))
    actual = float((problem(pset[rec]) * W).sum(-1).mean())
    got = metrics.estimate_expected_performance_after_scalarisation(pset.numpy(), front.numpy(), problem,
                                                                    scalarisations_seed=11)
    assert set(got) == {"predicted_scalarperf", "actual_scalarperf"}
    assert got["predicted_scalarperf"] == pytest.approx(predicted, rel=1e-13)
    assert got["actual_scalarperf"] == pytest.approx(actual, rel=1e-13)
    best = metrics.estimate_best_possible_expected_performance_after_scalarisation(front.numpy(),
                                                                                   scalarisations_seed=11)
    assert best == pytest.approx(predicted, rel=1e-13)
    state = torch.random.get_rng_state()
    metrics.estimate_best_possible_expected_performance_after_scalarisation(front.numpy(), scalarisations_seed=1)
    assert torch.equal(state, torch.random.get_rng_state())  # a seeded estimate leaves the global RNG alone


def test_hypervolume_from_posterior_mean_keys():
    problem = QuadraticProblem()
    pset = np.linspace(0, 1, 9).reshape(-1, 1).repeat(2, 1)
    front = problem(pset).numpy()
    out = metrics.estimate_hypervolume_from_posterior_mean(pset, front, problem, [-2.5, -2.5])
    assert list(out) == ["pfront_hv_lo", "pfront_hv_hi", "pset_hv_lo", "pset_hv_hi"]
    assert out["pfront_hv_lo"] == out["pset_hv_lo"] and out["pfront_hv_lo"] <= out["pfront_hv_hi"]


# ---------------------------------------------------------------- C entries, without a device

def _outs(m=2, n=8):
    outs = (_lib.DkgOutput * 8)()
    for o in outs:
        o.n, o.kernel = n, 2
        for f in ("inv_lengthscale", "train_x", "alpha"):
            setattr(o, f, 16)
    return outs


def test_pareto_validation_without_device():
    lib = _lib.load()
    outs, prm = _outs(), _lib.DkgNsga2Params()
    assert (prm.cr, prm.eta_c, prm.m, prm.eta_m, prm.raw_inputs) == (0.95, 10.0, 0.01, 50.0, 0)
    assert ctypes.sizeof(prm) == 40

    def nsga2(m=2, d=2, P=8, gens=1, ptr=16, work=1 << 30, outs=outs, prm=prm):
        return lib.dkg_pareto_nsga2(outs, m, d, ptr, ptr, P, gens, prm, ptr, ptr, ptr, ptr, ptr, ptr, work, None)

    assert nsga2(P=6) == _lib.DKG_ERR_ARG and b"P=6" in lib.dkg_last_error()
    assert nsga2(P=10) == _lib.DKG_ERR_ARG
    assert nsga2(P=1028) == _lib.DKG_ERR_UNSUPPORTED
    assert nsga2(m=9) == _lib.DKG_ERR_UNSUPPORTED
    assert nsga2(d=17) == _lib.DKG_ERR_UNSUPPORTED
    assert nsga2(ptr=None) == _lib.DKG_ERR_ARG
    assert nsga2(outs=None) == _lib.DKG_ERR_ARG
    assert nsga2(prm=None) == _lib.DKG_ERR_ARG
    assert nsga2(gens=-1) == _lib.DKG_ERR_ARG
    assert nsga2(work=lib.dkg_pareto_workspace(8, 2, 2) - 1) == _lib.DKG_ERR_WORKSPACE
    assert nsga2(outs=_outs(n=1025)) == _lib.DKG_ERR_UNSUPPORTED
    assert nsga2(prm=_lib.DkgNsga2Params(cr=1.5)) == _lib.DKG_ERR_ARG
    # the stage entries
    assert lib.dkg_posterior_mean(outs, 9, 2, 16, 4, 16, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_posterior_mean(outs, 2, 17, 16, 4, 16, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_posterior_mean(outs, 2, 2, None, 4, 16, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_posterior_mean(outs, 2, 2, 16, -1, 16, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_posterior_mean(outs, 2, 2, None, 0, None, None) == _lib.DKG_OK  # no points: a no-op
    assert lib.dkg_pareto_rank(16, 2049, 2, 1, 16, 16, 16, None, 0, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_pareto_rank(16, 8, 9, 8, 16, 16, 16, None, 0, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_pareto_rank(16, 8, 2, 9, 16, 16, 16, None, 0, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_pareto_rank(16, 8, 2, 0, 16, 16, 16, None, 0, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_pareto_rank(None, 8, 2, 8, 16, 16, 16, None, 0, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_pareto_variation(16, 16, 16, 6, 2, 16, 16, prm, 16, 16, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_pareto_variation(16, 16, 16, 1028, 2, 16, 16, prm, 16, 16, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_pareto_variation(16, 16, 16, 8, 17, 16, 16, prm, 16, 16, None) == _lib.DKG_ERR_UNSUPPORTED
    assert lib.dkg_pareto_variation(16, 16, 16, 8, 2, 16, 16, prm, None, 16, None) == _lib.DKG_ERR_ARG
    from dkg_amd.errors import UnsupportedError
    with pytest.raises(UnsupportedError):
        _lib.check(nsga2(P=1028), "dkg_pareto_nsga2")


def test_pareto_workspace_and_draws_grow():
    lib = _lib.load()
    assert lib.dkg_pareto_draws(8, 1) == 2 * 8 + 4 + 3 * 4 * 1 + 2 * 8 * 1 == pareto_ref.draws(8, 1)
    assert lib.dkg_pareto_draws(100, 2) == pareto_ref.draws(100, 2)
    assert lib.dkg_pareto_draws(8, 1) < lib.dkg_pareto_draws(12, 1) < lib.dkg_pareto_draws(12, 2)
    assert lib.dkg_pareto_draws(7, 2) == 0 and lib.dkg_pareto_draws(8, 0) == 0
    w = lib.dkg_pareto_workspace
    assert 0 < w(8, 1, 1) < w(1024, 1, 1) < w(1024, 16, 1) < w(1024, 16, 8)
    assert w(1024, 16, 8) >= 2 * 1024 * (16 + 8) * 8
    assert w(6, 2, 2) == 0 and w(1028, 2, 2) == 0 and w(8, 17, 2) == 0 and w(8, 2, 9) == 0


def test_evolution_entries_share_their_argument_checks():
    """dkg_pareto_variation, dkg_pareto_nsga2 and dkg_pareto_nsga2_paths refuse the same bad argument with the same
    status, before any device call; the workspace queries against the values of the commit before the one driver
    (recorded from its library): the paths' unchanged, the single population's less its normalised-points section."""
    lib = _lib.load()
    ptr, good = 16, _lib.DkgNsga2Params()
    paths = _lib.DkgRffPaths(2, 2, 2, 64, ptr, ptr, ptr, ptr)
    outs = _outs()

    def variation(P=8, prm=good):
        return lib.dkg_pareto_variation(ptr, ptr, ptr, P, 2, ptr, ptr, prm, ptr, ptr, None)

    def nsga2(P=8, prm=good, gens=1, short=0):
        work = (lib.dkg_pareto_workspace(P, 2, 2) or 1 << 30) - short
        return lib.dkg_pareto_nsga2(outs, 2, 2, ptr, ptr, P, gens, prm, ptr, ptr, ptr, ptr, ptr, ptr, work, None)

    def nsga2_paths(P=8, prm=good, gens=1, short=0):
        work = (lib.dkg_pareto_paths_workspace(2, P, 2, 2) or 1 << 30) - short
        return lib.dkg_pareto_nsga2_paths(paths, ptr, ptr, P, gens, prm, ptr, ptr, ptr, ptr, ptr, ptr, work, None)

    every, evolutions = (variation, nsga2, nsga2_paths), (nsga2, nsga2_paths)
    table = [(every, dict(P=6), _lib.DKG_ERR_ARG), (every, dict(P=10), _lib.DKG_ERR_ARG),
             (every, dict(P=1028), _lib.DKG_ERR_UNSUPPORTED),
             (every, dict(prm=_lib.DkgNsga2Params(cr=1.5)), _lib.DKG_ERR_ARG),
             (every, dict(prm=_lib.DkgNsga2Params(m=-0.1)), _lib.DKG_ERR_ARG),
             (every, dict(prm=_lib.DkgNsga2Params(eta_c=-1.0)), _lib.DKG_ERR_ARG),
             (every, dict(prm=None), _lib.DKG_ERR_ARG),
             (evolutions, dict(gens=-1), _lib.DKG_ERR_ARG),
             (evolutions, dict(short=1), _lib.DKG_ERR_WORKSPACE)]
    for entries, bad, want in table:
        assert [entry(**bad) for entry in entries] == [want] * len(entries), bad
    sizes = [lib.dkg_pareto_paths_workspace(*a) for a in ((1, 8, 1, 1), (3, 100, 2, 2), (10, 1024, 16, 8))]
    assert sizes == [1280, 29440, 4259840]
    before = {(8, 1, 1): 2304, (100, 2, 2): 14592, (1024, 16, 8): 573696}
    for (P, d, m), old in before.items():
        assert lib.dkg_pareto_workspace(P, d, m) == old - (P * d * 8 + 255) // 256 * 256


def test_front_sampler_refuses_minimisation_before_any_device_work():
    from dkg_amd import UnsupportedError, sample_points_on_pareto_front

    with pytest.raises(UnsupportedError):
        sample_points_on_pareto_front(None, maximize=False)


# ---------------------------------------------------------------- the committed quality yardstick

def test_quality_yardstick_is_consistent():
    q = json.load(open(os.path.join(HERE, "golden", "pareto_quality.json")))
    assert q["P"] == 100 and q["gen"] == 100 and q["seeds"] == [0, 1, 2, 3, 4] and len(q["r"]) == 5
    assert q["t"] == pytest.approx(min(q["r"]) - 2.0 * (max(q["r"]) - min(q["r"])), rel=1e-15)
    assert all(r0 < q["t"] for r0 in q["r0"])  # the threshold tells evolution from the initial sample
    assert all(0.0 < r <= 1.01 for r in q["r"])
    shared = torch.load(os.path.join(HERE, "golden", "shared", "gp-problem", "lengthscales", "0.pt"),
                        weights_only=True)
    assert q["ref_point"] == list(shared["ref_point"])
