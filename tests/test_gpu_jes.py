"""The device joint entropy search (dkg_jes_*, dkg_amd.jes) against CPU yardsticks only: the oracle posterior of
every conditioned model and the fp64 restatement of the entropy bound (tests/jes_oracle.py, itself pinned to the
reference's function by tests/golden/jes_entropy.npz).  Cases and their conditions: tests/jes_cases.py.

Bounds.  Moments: the project's LINE_RTOL = 1e-8 on the prior scale (v is the cancellation s - |q|^2):
|d mu| <= 1e-8 y_std (|c| + sqrt(s)), |d v| <= 1e-8 y_std^2 s.  Values: 1e-6 |acq| plus 4 x SPREAD_VALUE, the
largest difference over the committed cases between the restatement on the oracle posterior as is and with every
output's training rows reversed (the same function, another summation order: the reference side's own rounding
floor; the factor 4 covers the device's different association of the same sums).  Gradients: 1e-6 max_j |g_j|
plus 4 x SPREAD_GRAD, measured the same way on the autograd gradient.  Both spreads are measured on the CPU
(test_jes_host.py checks the constants against a fresh measurement) and are set by the noise = 1e-8 case.

The same three tests and bounds run over jes_cases.SHAPE_CASES: the shapes at which the kernels' loops repeat
(more than 8 column tiles of Q per workgroup, up to the 64 of n = 1024; more states than waves, up to 65; the
d buckets 4 and 16; m = 4, 5, 7; 64, 65, 129 and 4096 boxes; sum_j W_j on both sides of 1).  The spreads stay
those of CASES.  Bit tests cover a plan that grows, a full candidate tile, and the candidate limit.

Measured on MI355X (worst over the cases): DEVICE_WORST and DEVICE_WORST_SHAPES below and DESIGN.md 8d.
"""

import functools

import pytest
import torch

import jes_cases
import jes_oracle
from helpers import LINE_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# reference-side spreads over jes_cases.CASES (tests/jes_cases.spreads; both from "m2-d2-P3-J6-noise1e-8")
SPREAD_VALUE = 1.1e-8
SPREAD_GRAD = 1.8e-6
RTOL = 1e-6
# the device's worst errors over the cases as measured on MI355X (informational; the asserts use the bounds above):
# moments |d mu| / bound, |d v| / bound; entropy stage alone |d acq|; end to end |d acq|; gradient |d g|
DEVICE_WORST = {"mu_ratio": 5.3e-6, "v_ratio": 4.3e-7, "stage": 2.7e-9, "end_to_end": 3.1e-9, "grad": 3.9e-11}

# the same over jes_cases.SHAPE_CASES, asserted with the bounds above (their own reference-side spreads, at most
# 1.3e-13 and 1.3e-12, set none: test_jes_host.py).  mu and the gradient from n1019-k5, v from n127-P4-d3, the values from m7-d8-J65
DEVICE_WORST_SHAPES = {"mu_ratio": 1.65e-5, "v_ratio": 3.0e-7, "stage": 1.42e-14, "end_to_end": 1.55e-13,
                       "grad": 1.15e-12}

ALL_CASES = {**jes_cases.CASES, **jes_cases.SHAPE_CASES}
CASE_IDS = list(ALL_CASES)
COMBOS = [(cid, est, t) for cid in CASE_IDS for est in jes_cases.ESTIMATORS
          for t in jes_cases.targets_of(ALL_CASES[cid]["m"])]
M12_CASES = {cid for cid, c in ALL_CASES.items() if "M12" in c["fam"]}


def _id(v):
    return "all" if v is None else str(v)


@functools.lru_cache(maxsize=None)
def acquisition(cid, est, target):
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch

    state, sets, fronts, bounds, _ = jes_cases.problem(cid)
    return qLowerBoundMultiObjectiveJointEntropySearch(state, sets, fronts, bounds, estimation_type=est,
                                                       target_output_ix=target, device=DEV)


@functools.lru_cache(maxsize=None)
def device_result(cid, est, target):
    """(acq [B], dacq [B, d], (mu, v, tau) [S, m, B]) of the device, on the host."""
    X = jes_cases.problem(cid)[4]
    acq = acquisition(cid, est, target)
    val, g = acq.value_and_grad_host(X)
    _, mu, v, tau = acq.moments(X)
    return val, g, (mu.cpu(), v.cpu(), tau.cpu())


@pytest.mark.parametrize("cid", CASE_IDS)
def test_moments_match_the_oracle_posterior_of_every_conditioned_model(cid):
    state = jes_cases.problem(cid)[0]
    mu_r, v_r, tau_r = jes_cases.reference(cid)["moments"]
    _, _, (mu, v, tau) = device_result(cid, "LB", None)
    worst_mu = worst_v = 0.0
    for i, o in enumerate(state.models):
        tol_mu = LINE_RTOL * o.y_std * (abs(o.mean_constant) + o.outputscale ** 0.5)
        tol_v = LINE_RTOL * o.y_std ** 2 * o.outputscale
        e_mu = float((mu[:, i] - mu_r[:, i]).abs().max())
        e_v = max(float((v[:, i] - v_r[:, i]).abs().max()), float((tau[:, i] - tau_r[:, i]).abs().max()))
        worst_mu, worst_v = max(worst_mu, e_mu / tol_mu), max(worst_v, e_v / tol_v)
    print(f"{cid}: moments worst |d mu| / bound {worst_mu:.3g}, |d v| / bound {worst_v:.3g}")
    assert worst_mu <= 1.0 and worst_v <= 1.0, (worst_mu, worst_v)


@pytest.mark.parametrize("cid,est,target", COMBOS, ids=[f"{c}-{e}-t{_id(t)}" for c, e, t in COMBOS])
def test_entropy_stage_alone_on_the_devices_own_moments(cid, est, target):
    bounds = jes_cases.problem(cid)[3]
    val, _, (mu, v, tau) = device_result(cid, est, target)
    ref = jes_oracle.acq_from_moments(bounds, mu, v, tau, target, est == "LB2")
    err = (val - ref).abs()
    print(f"{cid} {est} t={target}: entropy stage worst |d acq| {float(err.max()):.3g}")
    assert bool((err <= RTOL * ref.abs() + 4 * SPREAD_VALUE).all()), float(err.max())


@pytest.mark.parametrize("cid,est,target", COMBOS, ids=[f"{c}-{e}-t{_id(t)}" for c, e, t in COMBOS])
def test_end_to_end_value_and_gradient(cid, est, target):
    ref, g_ref = jes_cases.reference(cid)[(est, target)]
    val, g, _ = device_result(cid, est, target)
    err = (val - ref).abs()
    print(f"{cid} {est} t={target}: end to end worst |d acq| {float(err.max()):.3g}")
    assert bool((err <= RTOL * ref.abs() + 4 * SPREAD_VALUE).all()), float(err.max())
    # every candidate; on a Matern-1/2 output the gradient at a coincident point (candidates 0 and 1: on a
    # Pareto-set point and on a training point) is a convention and is left out
    rows = torch.arange(2 if cid in M12_CASES else 0, g.shape[0])
    gerr = (g - g_ref).abs()[rows].amax(-1)
    tol = RTOL * g_ref.abs()[rows].amax(-1) + 4 * SPREAD_GRAD
    print(f"{cid} {est} t={target}: gradient worst |d g| {float(gerr.max()):.3g}")
    assert bool((gerr <= tol).all()), (float(gerr.max()), float((gerr / tol).max()))


def test_gradient_is_the_central_difference_of_the_device_value():
    """h = 1e-5: the truncation h^2 f''' / 6 with f''' ~ 1e2 |g| (a few lengthscales of ~0.3) is ~2e-9 |g| and
    the rounding eps |acq| / h ~ 1e-11: both far inside 1e-5 max |g| + 1e-9."""
    cid = "m1-d1-P1-J1"
    X = jes_cases.problem(cid)[4]
    for est in jes_cases.ESTIMATORS:
        acq = acquisition(cid, est, None)
        _, g = acq.value_and_grad_host(X)
        h = 1e-5
        fd = torch.zeros_like(g)
        for j in range(X.shape[1]):
            e = torch.zeros_like(X)
            e[:, j] = h
            fd[:, j] = (acq.value_and_grad_host(X + e)[0] - acq.value_and_grad_host(X - e)[0]) / (2 * h)
        err = (g - fd).abs().amax(-1)
        assert bool((err <= 1e-5 * g.abs().amax(-1) + 1e-9).all()), float(err.max())


def test_bits():
    cid = "m2-d2-P3-J6-noise1e-8"
    X = jes_cases.problem(cid)[4]
    assert X.shape[0] == 40
    acq = acquisition(cid, "LB", None)
    v1, g1 = acq.value_and_grad_host(X)
    v2, g2 = acq.value_and_grad_host(X)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)                     # two calls
    for b in (0, 17, 39):                                                   # B = 1 against row b of B = 40
        vb, gb = acq.value_and_grad_host(X[b:b + 1])
        assert torch.equal(vb, v1[b:b + 1]) and torch.equal(gb, g1[b:b + 1]), b
    v17, g17 = acq.value_and_grad_host(X[5:22])                             # B = 17: another tile split
    assert torch.equal(v17, v1[5:22]) and torch.equal(g17, g1[5:22])
    # the host route, the device route and value_and_grad_host
    Xh = X.clone().unsqueeze(1).requires_grad_(True)
    vh = acq(Xh)
    (gh,) = torch.autograd.grad(vh.sum(), Xh)
    Xd = X.to(DEV).unsqueeze(1).requires_grad_(True)
    vd = acq(Xd)
    (gd,) = torch.autograd.grad(vd.sum(), Xd)
    assert torch.equal(vh.detach(), v1) and torch.equal(vd.detach().cpu(), v1)
    assert torch.equal(gh.squeeze(1), g1) and torch.equal(gd.squeeze(1).cpu(), g1)
    with torch.no_grad():
        assert torch.equal(acq(X.unsqueeze(1)), v1) and torch.equal(acq(X.to(DEV).unsqueeze(1)).cpu(), v1)
    # LB and LB2 with a target are the same value in exact arithmetic
    for t in (0, 1):
        a = device_result(cid, "LB", t)[0]
        b = device_result(cid, "LB2", t)[0]
        assert bool(((a - b).abs() <= RTOL * a.abs() + 4 * SPREAD_VALUE).all()), t


def _fresh(cid, est="LB", target=None):
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    state, sets, fronts, bounds, X = jes_cases.problem(cid)
    return JES(state, sets, fronts, bounds, estimation_type=est, target_output_ix=target, device=DEV), X


def test_bits_do_not_change_when_the_plan_grows():
    """A new acquisition: 3 candidates (a plan for 16), then 17 (a new plan for 32, another workspace carve and
    row pitch), then the 3 again on the grown plan."""
    acq, X = _fresh("n253-P7-d4")
    assert X.shape[0] == 17
    v3, g3 = acq.value_and_grad_host(X[:3])
    assert acq._plan.max_B == 16
    v17, g17 = acq.value_and_grad_host(X)
    assert acq._plan.max_B == 32
    w3, h3 = acq.value_and_grad_host(X[:3])
    assert acq._plan.max_B == 32
    assert torch.equal(v3, w3) and torch.equal(g3, h3)
    assert torch.equal(v3, v17[:3]) and torch.equal(g3, g17[:3])
    # and the cached acquisition of the oracle tests, whose plan began at 32
    v, g, _ = device_result("n253-P7-d4", "LB", None)
    assert torch.equal(v, v17) and torch.equal(g, g17)


def test_bits_of_a_full_tile_are_those_of_its_candidates_alone():
    """B = 16: no row of the moments stage's tile is a clamped repeat; against 16 calls with B = 1, where 15 are."""
    cid = "n127-P4-d3"
    X = jes_cases.problem(cid)[4]
    assert X.shape[0] == 16
    for est, t in (("LB", None), ("LB2", 0)):
        acq = acquisition(cid, est, t)
        v16, g16 = acq.value_and_grad_host(X)
        for b in range(16):
            vb, gb = acq.value_and_grad_host(X[b:b + 1])
            assert torch.equal(vb, v16[b:b + 1]) and torch.equal(gb, g16[b:b + 1]), (est, t, b)


def test_grid_edge_of_the_candidates():
    """DKG_JES_MAX_CANDIDATES = 65536 candidates in one call (4096 tiles x 8 state-outputs; 65536 workgroups of
    the entropy stage): the 40 candidates of the case over and over, every copy with the bits of the B = 40 call.
    One more candidate is refused by dkg_jes_init, before any launch."""
    from dkg_amd import UnsupportedError, _lib

    cid = "m2-d2-P3-J6-noise1e-8"
    acq, X = _fresh(cid)
    B = _lib.DKG_JES_MAX_CANDIDATES
    with torch.no_grad():
        v40 = acq(X.unsqueeze(1))
        assert torch.equal(v40, device_result(cid, "LB", None)[0])
        reps = -(-B // 40)
        big = acq(X.repeat(reps, 1)[:B].unsqueeze(1))
        assert acq._plan.max_B == B and big.shape == (B,)
        assert torch.equal(big, v40.repeat(reps)[:B])
        plan = acq._plan
        with pytest.raises(UnsupportedError, match="dkg_jes_init.*candidates"):
            acq(X.repeat(reps, 1)[:B + 1].unsqueeze(1))
        assert acq._plan is plan


def test_more_than_1024_training_rows_are_refused():
    """A model of 1024 points is served (n1019-k5 reaches 1024 rows by conditioning); one Pareto point more makes
    the conditioned state 1025 rows, which the preparation of that state refuses at construction, ahead of
    dkg_jes_init's own check of n (test_jes_host.py)."""
    from dkg_amd import UnsupportedError, compute_sample_box_decomposition
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES
    from helpers import grad_case

    state, _, _, X = grad_case(1, 1, (1024,), ("M52",), 4, 2, 2, 31, noise=1e-2)
    front = torch.tensor([[1.0]], dtype=torch.double)
    with pytest.raises(UnsupportedError, match="1025"):
        acq = JES(state, [X[:1]], [front], compute_sample_box_decomposition([front]), device=DEV)
        acq.value_and_grad_host(X)


def test_errors_on_the_device():
    from dkg_amd import UnsupportedError

    cid = "m1-d1-P1-J1"
    state, sets, fronts, bounds, X = jes_cases.problem(cid)
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    acq = JES(state, sets, fronts, bounds, target_output_ix=-1, device=DEV)     # -1: the last output
    assert torch.equal(acq.value_and_grad_host(X)[0], acquisition(cid, "LB", 0).value_and_grad_host(X)[0])
    with pytest.raises(IndexError):
        JES(state, sets, fronts, bounds, target_output_ix=1, device=DEV)(X.unsqueeze(1))
    with pytest.raises(AssertionError):
        acq(torch.rand(3, 2, 1))                                                # q = 2
    with pytest.raises(UnsupportedError):
        acq.set_X_pending(torch.rand(1, 1))


OPT_CASE = jes_cases.OPT_CASE


@pytest.mark.parametrize("est,target", [("LB", None), ("LB2", 1)])
def test_optimize_acqf_matches_the_restatement(est, target):
    """SMOKE settings (2 restarts, 4 raw samples, fixed Pareto samples); the tolerances and the argument are
    test_gpu_optim.py's: values and gradients agree far below L-BFGS-B's own tolerances, so both
    runs follow the same path."""
    from dkg_amd.optim import optimize_acqf

    state, sets, fronts, bounds, _ = jes_cases.problem(OPT_CASE)
    dev = acquisition(OPT_CASE, est, target)
    ora = jes_oracle.OracleJES(state, sets, fronts, bounds, est, target)
    box = torch.tensor([[0.0, 0.0], [1.0, 1.0]])
    opts = {"batch_limit": 1, "maxiter": 40, "seed": 5}
    torch.manual_seed(7)
    Xd, Vd = optimize_acqf(dev, box, 1, 2, raw_samples=4, options=opts, return_best_only=False)
    torch.manual_seed(7)
    Xo, Vo = optimize_acqf(ora, box, 1, 2, raw_samples=4, options=opts, return_best_only=False)
    assert bool(((Vd - Vo).abs() <= 1e-6 * Vo.abs() + 1e-8).all()), (Vd, Vo)
    assert bool(((Xd - Xo).abs() <= 1e-4).all()), (Xd, Xo)


def test_spec_returns_the_objective_of_the_restatement_driven_spec():
    from dkg_amd.optim import JesOptimisationSpec

    state, sets, fronts, _, _ = jes_cases.problem(OPT_CASE)
    calls = []

    def sampler(model, bounds, num_samples, target_num_points):
        calls.append((num_samples, target_num_points, tuple(bounds.shape)))
        return sets, fronts

    def oracle_factory(model, ps, pf, hb, est, target):
        return jes_oracle.OracleJES(model, ps, pf, hb, est, target)

    out = []
    for factory in (None, oracle_factory):
        spec = JesOptimisationSpec("LB2", 3, 5, 2, 4, 1, 30, pareto_sampler=sampler, device=DEV, seed=3,
                                   acq_factory=factory)
        torch.manual_seed(11)
        out.append(spec.optimize_for_single_objective(state, [1.0, 2.0], 2))
    (xd, i_d, vd), (xo, i_o, vo) = out
    assert calls[0] == (3, 5, (2, 2))
    assert i_d == i_o
    assert bool(((xd - xo).abs() <= 1e-4).all()) and abs(float(vd - vo)) <= 1e-6 * abs(float(vo)) + 1e-8
    torch.manual_seed(11)
    x, v = JesOptimisationSpec("LB", 3, 5, 2, 4, 1, 30, pareto_sampler=sampler, device=DEV,
                               seed=3).optimize_for_full_evaluation(state, 2)
    assert x.shape == (1, 2) and bool(torch.isfinite(v))
