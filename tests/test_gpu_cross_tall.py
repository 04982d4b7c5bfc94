"""The one-launch cross stage with K(x, X) kept in LDS (cross_tall_kernel; include/dkg.h dkg_debug_cross_tall).

Every comparison is bit for bit between mode 1 (the kernel wherever the shape is eligible) and mode 0 (never: the
per-row-tile cross kernels) on the same plan inputs: KG, KG per (candidate, scalarisation) and the exported lines,
whose slopes carry Q_X through the covariance stage and whose first intercept carries the means.  Training-set
sizes cover odd and even tile counts (the middle column tile that has no partner, and the one-tile case); batch
sizes cover partial 16-row tiles, a lone candidate tile in a two-tile workgroup and launches of several batches
that straddle tiles.  One case holds mode 1 against the oracle, and one checks the default dispatch.
"""

import pytest
import torch

from dkg_amd import DiscreteKnowledgeGradient, _lib
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from dkg_amd.synthetic import WORKLOADS, make_problem
from helpers import check_parity_case, parity_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FAMILIES = {"matern52": ("matern", 2.5), "matern32": ("matern", 1.5), "matern12": ("matern", 0.5),
            "rbf": ("rbf", None)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")


@pytest.fixture(autouse=True)
def _restore_mode():
    lib = _lib.load()
    prev = lib.dkg_debug_cross_tall(-1)
    yield
    torch.cuda.synchronize()
    lib.dkg_debug_cross_tall(prev)


def _problem(n, d, m, family, N=40, S=5, seed=0):
    """m outputs on n shared training points (output i keeps n - 3 i of them when that leaves any, so the outputs
    of one launch have different tile counts), N discretisation points, S scalarisations."""
    kernel, nu = FAMILIES[family]
    g = torch.Generator().manual_seed(100 + seed)
    X = torch.rand(n, d, generator=g, dtype=torch.double)
    outs = []
    for i in range(m):
        ni = n - 3 * i if n - 3 * i >= 1 else n
        y = torch.sin(3 * X[:ni, 0]) + 0.3 * i + 0.05 * torch.randn(ni, generator=g, dtype=torch.double)
        ls = [0.3 + 0.1 * i + 0.05 * k for k in range(d)]
        outs.append(SingleTaskGPState(X[:ni].clone(), y, ls, 1.0 + 0.5 * i, 1e-2, 0.1 * (i + 1), kernel=kernel,
                                      nu=nu))
    D = torch.rand(N, d, generator=g, dtype=torch.double)
    W = torch.rand(S, m, generator=g, dtype=torch.double)
    return ModelListGPState(*outs), D, W / W.sum(-1, keepdim=True)


def _run(plan, X, B, mode):
    """KG of the launch (batches of B), and of all of X as one batch: KG, pairs, lines."""
    lib = _lib.load()
    lib.dkg_debug_cross_tall(mode)
    before = lib.dkg_debug_cross_tall_launches()
    kgb = torch.full((X.shape[0],), float("nan"), dtype=torch.double, device=DEV)
    plan.forward_batches_into(X, kgb, B)
    kg, pairs, _ = plan.forward_stats(X)
    a, b = plan.lines(X)
    torch.cuda.synchronize()
    took = lib.dkg_debug_cross_tall_launches() - before
    assert took == (3 if mode == 1 else 0), f"mode {mode}: {took} of 3 cross launches took the one-launch kernel"
    return [t.cpu() for t in (kgb, kg, pairs, a, b)]


def _assert_same(got, ref):
    for name, x, y in zip(("kg (batches)", "kg", "kg_pairs", "intercepts", "slopes"), got, ref):
        assert not torch.isnan(y).any(), name
        assert torch.equal(x, y), f"{name}: {(x != y).sum().item()} of {y.numel()} values differ"


# (n, B, batches, d, m, family, target): every n of {15, 16, 17, 33, 100, 256}, B of {1, 15, 17, 65, 130} and
# 3 x 37, d of {1, 2, 6}, m of {1, 2, 3}, the four families, targets None / 0 / last
CASES = [
    (15, 1, 1, 1, 1, "matern52", None),
    (16, 15, 1, 2, 2, "rbf", 0),
    (17, 17, 1, 6, 3, "matern32", 2),
    (33, 65, 1, 2, 2, "matern12", 1),
    (100, 130, 1, 2, 2, "matern52", None),
    (256, 130, 1, 2, 2, "matern52", 0),
    (256, 17, 1, 6, 3, "rbf", None),
    (100, 37, 3, 2, 3, "matern32", 2),
    (256, 37, 3, 1, 1, "matern12", 0),
    (33, 1, 1, 6, 2, "matern52", 1),
    (17, 130, 1, 1, 2, "rbf", None),
    (16, 65, 1, 6, 1, "matern32", None),
    (15, 37, 3, 2, 3, "matern12", 0),
    (100, 15, 1, 1, 2, "rbf", 1),
]


@pytest.mark.parametrize("n,B,K,d,m,family,target", CASES)
def test_same_bits_as_the_row_tile_kernels(n, B, K, d, m, family, target):
    model, D, W = _problem(n, d, m, family)
    acq = DiscreteKnowledgeGradient(model, D, W, target_output_ix=target, device=DEV)
    X = torch.quasirandom.SobolEngine(d, scramble=True, seed=5).draw(K * B, dtype=torch.double).to(DEV)
    plan = acq._state.plan(acq._W, acq._target, K * B)
    ref = _run(plan, X, B, 0)
    got = _run(plan, X, B, 1)
    _assert_same(got, ref)
    assert (ref[1] > 0).any()


def test_candidates_on_discretisation_points_and_repeated_launches():
    """Coincidence marks set by one launch and cleared by the next, on one plan: a launch with candidates on
    discretisation points, then one without them, then the first again."""
    model, D, W = _problem(100, 2, 2, "matern52", N=60)
    acq = DiscreteKnowledgeGradient(model, D, W, device=DEV)
    B, K = 37, 3
    X1 = torch.quasirandom.SobolEngine(2, scramble=True, seed=8).draw(K * B, dtype=torch.double)
    X2 = X1.clone()
    X1[[0, 16, 40, 110]] = D[[3, 3, 17, 59]]
    X1, X2 = X1.to(DEV), X2.to(DEV)
    plan = acq._state.plan(acq._W, acq._target, K * B)
    ref = [_run(plan, X, B, 0) for X in (X1, X2, X1)]
    got = [_run(plan, X, B, 1) for X in (X1, X2, X1)]
    for g, r in zip(got, ref):
        _assert_same(g, r)
    assert not torch.equal(ref[0][1], ref[1][1])  # the coincident candidates changed the result
    _assert_same(ref[2], ref[0])


def test_replayed_from_a_captured_graph_twice():
    """A launch captured under mode 1 keeps the kernel it was captured with; its replays leave no state behind."""
    lib = _lib.load()
    model, D, W = _problem(100, 2, 2, "matern32", N=60)
    acq = DiscreteKnowledgeGradient(model, D, W, target_output_ix=1, device=DEV)
    B, K = 37, 3
    X = torch.quasirandom.SobolEngine(2, scramble=True, seed=9).draw(K * B, dtype=torch.double)
    X[5] = D[11]
    X = X.to(DEV)
    plan = acq._state.plan(acq._W, acq._target, K * B)
    lib.dkg_debug_cross_tall(0)
    ref = torch.full((K * B,), float("nan"), dtype=torch.double, device=DEV)
    plan.forward_batches_into(X, ref, B)
    torch.cuda.synchronize()
    lib.dkg_debug_cross_tall(1)
    kg = torch.full_like(ref, float("nan"))
    plan.forward_batches_into(X, kg, B)  # warm: the capture must not be the kernel's first launch
    torch.cuda.synchronize()
    before = lib.dkg_debug_cross_tall_launches()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(DEV), capture_error_mode="thread_local"):
        plan.forward_batches_into(X, kg, B)
    assert lib.dkg_debug_cross_tall_launches() == before + 1
    lib.dkg_debug_cross_tall(0)  # the graph keeps its kernel
    for _ in range(2):
        kg.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(kg.cpu(), ref.cpu())
    assert (ref > 0).any()


def test_against_the_oracle():
    """Mode 1 against the oracle at the suite's parity tolerances (helpers.check_parity_case), so the kernel
    cannot pass only by matching a wrong default."""
    lib = _lib.load()
    model, D, W = _problem(100, 2, 2, "matern52", N=60, S=6)
    X = torch.quasirandom.SobolEngine(2, scramble=True, seed=4).draw(130, dtype=torch.double)
    lib.dkg_debug_cross_tall(1)
    before = lib.dkg_debug_cross_tall_launches()
    res = parity_case(model, D, W, X, None, dev=DEV)
    assert lib.dkg_debug_cross_tall_launches() > before
    check_parity_case(res)


def test_default_dispatch_takes_it_at_512_candidates():
    """4 batches of 128 at n = 256, m = 2 with the mode left at its default: the launch's rows are those of four
    single forwards (the contract of dkg_plan_forward_batches), and its cross stage is the one-launch kernel."""
    lib = _lib.load()
    assert lib.dkg_debug_cross_tall(-1) == -1
    model, D, _, W = make_problem(WORKLOADS["headline"])
    acq = DiscreteKnowledgeGradient(model, D, W, device=DEV)
    B, K = 128, 4
    X = torch.quasirandom.SobolEngine(D.shape[1], scramble=True, seed=3).draw(K * B, dtype=torch.double)
    X[130:133] = D[[5, 500, 1000]]
    X = X.to(DEV)
    big = acq._state.plan(acq._W, acq._target, K * B)
    one = acq._state.plan(acq._W, acq._target, B)
    ref = torch.full((K * B,), float("nan"), dtype=torch.double, device=DEV)
    before = lib.dkg_debug_cross_tall_launches()
    for j in range(K):
        one.forward_into(X[j * B:(j + 1) * B], ref[j * B:(j + 1) * B])
    assert lib.dkg_debug_cross_tall_launches() == before  # 128 candidates: the per-tile kernel
    kg = torch.full_like(ref, float("nan"))
    big.forward_batches_into(X, kg, B)
    assert lib.dkg_debug_cross_tall_launches() == before + 1
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any()
    assert torch.equal(kg.cpu(), ref.cpu())
    assert (ref > 0).any()
