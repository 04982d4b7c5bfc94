"""Joint entropy search with conditioning="append": the conditioned states built from state 0's caches by one
batched block update (dkg_append_rows) instead of a full preparation each.  The cases, references and bounds are
those of test_gpu_jes.py (tests/jes_cases.py, tests/jes_oracle.py), unchanged: the exported moments of every
conditioned state against the oracle posterior (DESIGN.md 8d's moment bounds), and value and gradient end to end.

Conditions on the inputs, asserted on the CPU before anything runs on the device: every base output factorises
without jitter, every augmented matrix has torch.linalg.cholesky_ex(...).info == 0 (so no job may fall back: the
tests assert append_fallbacks == 0), and the cases' own W >= 1e-3 (jes_cases.reference asserts it).
"""

import functools

import pytest
import torch

import jes_cases
import jes_oracle
from append_rows_ref import covar
from helpers import LINE_RTOL
from test_gpu_jes import RTOL, SPREAD_GRAD, SPREAD_VALUE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every family, noise 1e-8 and 1e-2, Standardize on and off, m = 1..8; unequal front lengths (ks differ between
# the samples) in all but the P = 1 cases; n = 1024 reached by the update; 64 samples; 36 jobs of d = 16
CASE_IDS = list(jes_cases.CASES) + ["n127-P4-d3", "n253-P7-d4", "n1019-k5", "m4-d16-P9-J129", "m1-P64"]
ALL_CASES = {**jes_cases.CASES, **jes_cases.SHAPE_CASES}
COMBOS = [(cid, est, t) for cid in CASE_IDS for est in jes_cases.ESTIMATORS
          for t in jes_cases.targets_of(ALL_CASES[cid]["m"])]
M12_CASES = {cid for cid in CASE_IDS if "M12" in ALL_CASES[cid]["fam"]}


def _id(v):
    return "all" if v is None else str(v)


@functools.lru_cache(maxsize=None)
def conditions(cid):
    """The conditions on the inputs, on the CPU alone."""
    from dkg_amd.jes import conditioned_states

    state, sets, fronts, _, _ = jes_cases.problem(cid)
    for s in [state] + conditioned_states(state, sets, fronts):
        for i, o in enumerate(s.models):
            K = covar(o, o.train_x, o.train_x) + o.noise * torch.eye(o.num_train, dtype=torch.double)
            assert int(torch.linalg.cholesky_ex(K).info) == 0, (cid, i, o.num_train)
    jes_cases.reference(cid)  # asserts W >= 1e-3
    return True


@functools.lru_cache(maxsize=None)
def acquisition(cid, est, target):
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch

    assert conditions(cid)
    state, sets, fronts, bounds, _ = jes_cases.problem(cid)
    acq = qLowerBoundMultiObjectiveJointEntropySearch(state, sets, fronts, bounds, estimation_type=est,
                                                      target_output_ix=target, device=DEV, conditioning="append")
    assert acq.conditioning == "append" and acq.append_fallbacks == 0
    assert all(c.jitter == 0.0 for cs in acq._caches for c in cs)
    return acq


@functools.lru_cache(maxsize=None)
def device_result(cid, est, target):
    X = jes_cases.problem(cid)[4]
    acq = acquisition(cid, est, target)
    val, g = acq.value_and_grad_host(X)
    _, mu, v, tau = acq.moments(X)
    return val, g, (mu.cpu(), v.cpu(), tau.cpu())


def test_unequal_front_lengths_are_among_the_cases():
    assert len(set(ALL_CASES["m2-d2-P3-J6-noise1e-8"]["ks"])) > 1 and len(set(ALL_CASES["n253-P7-d4"]["ks"])) > 1


@pytest.mark.parametrize("cid", CASE_IDS)
def test_moments_of_every_appended_state_match_the_oracle_posterior(cid):
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
    print(f"{cid}: append: moments worst |d mu| / bound {worst_mu:.3g}, |d v| / bound {worst_v:.3g}")
    assert worst_mu <= 1.0 and worst_v <= 1.0, (worst_mu, worst_v)


@pytest.mark.parametrize("cid,est,target", COMBOS, ids=[f"{c}-{e}-t{_id(t)}" for c, e, t in COMBOS])
def test_end_to_end_value_and_gradient(cid, est, target):
    ref, g_ref = jes_cases.reference(cid)[(est, target)]
    val, g, _ = device_result(cid, est, target)
    err = (val - ref).abs()
    print(f"{cid} {est} t={target}: append: end to end worst |d acq| {float(err.max()):.3g}")
    assert bool((err <= RTOL * ref.abs() + 4 * SPREAD_VALUE).all()), float(err.max())
    rows = torch.arange(2 if cid in M12_CASES else 0, g.shape[0])  # as test_gpu_jes.py: Matern-1/2 at a coincidence
    gerr = (g - g_ref).abs()[rows].amax(-1)
    tol = RTOL * g_ref.abs()[rows].amax(-1) + 4 * SPREAD_GRAD
    print(f"{cid} {est} t={target}: append: gradient worst |d g| {float(gerr.max()):.3g}")
    assert bool((gerr <= tol).all()), (float(gerr.max()), float((gerr / tol).max()))


def test_default_is_the_full_preparation():
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    state, sets, fronts, bounds, X = jes_cases.problem("m1-d1-P1-J1")
    acq = JES(state, sets, fronts, bounds, device=DEV)
    assert acq.conditioning == "refactorise" and acq.append_fallbacks == 0
    with pytest.raises(ValueError, match="conditioning"):
        JES(state, sets, fronts, bounds, device=DEV, conditioning="chain")


def test_a_base_output_prepared_with_jitter_takes_the_full_preparation():
    """test_gpu_append.py's duplicated-input output (noise -5e-9: psd_safe_cholesky needs jitter 1e-8): its job is
    not appended, the state is the full preparation's, bit for bit, and one fallback is counted."""
    from dkg_amd import compute_sample_box_decomposition
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    X = torch.rand(12, 2, generator=torch.Generator().manual_seed(3), dtype=torch.double)
    X = torch.cat([X, X[:4]])
    y = torch.randn(16, generator=torch.Generator().manual_seed(4), dtype=torch.double)
    state = ModelListGPState(SingleTaskGPState(X, y, 0.5, 1.0, -5e-9, 0.0))
    sets = [torch.tensor([[0.37, 0.81]], dtype=torch.double)]
    fronts = [torch.tensor([[1.5]], dtype=torch.double)]
    bounds = compute_sample_box_decomposition(fronts)
    Xc = torch.rand(5, 2, generator=torch.Generator().manual_seed(6), dtype=torch.double)
    a = JES(state, sets, fronts, bounds, device=DEV, conditioning="append")
    b = JES(state, sets, fronts, bounds, device=DEV)
    assert a._caches[0][0].jitter == pytest.approx(1e-8) and a.append_fallbacks == 1 and b.append_fallbacks == 0
    va, ga = a.value_and_grad_host(Xc)
    vb, gb = b.value_and_grad_host(Xc)
    assert torch.equal(va, vb) and torch.equal(ga, gb)


def test_spec_with_device_sampler_and_append(monkeypatch):
    """SMOKE sizes (test_gpu_jes_pareto.py's spec test).  Every evaluation the optimiser made is recorded and
    replayed on the restatement, within the bounds of the end-to-end test."""
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES
    from dkg_amd.optim import JesOptimisationSpec

    state = jes_cases.problem(jes_cases.OPT_CASE)[0]
    d = state.input_dim
    record = []
    orig = JES.value_and_grad_host

    def recording(self, X):
        val, g = orig(self, X)
        record.append((self, X.detach().clone(), val.clone(), g.clone()))
        return val, g

    monkeypatch.setattr(JES, "value_and_grad_host", recording)
    spec = JesOptimisationSpec.with_device_sampler("LB", 3, 5, 2, 8, 1, 5, device=DEV, seed=0, num_rffs=64,
                                                   nsga2_pop_size=24, nsga2_generations=10, conditioning="append")
    assert spec.conditioning == "append"
    x, i, v = spec.optimize_for_single_objective(state, [1.0] * state.num_outputs, d)
    assert x.shape == (1, d) and bool(((x >= 0) & (x <= 1)).all()) and 0 <= int(i) < state.num_outputs
    assert bool(torch.isfinite(v).all())
    assert record and {id(r[0]) for r in record} and all(r[0].conditioning == "append" for r in record)
    models = {}
    for acq, X, val, g in record:
        assert acq.append_fallbacks == 0
        if id(acq) not in models:
            models[id(acq)] = jes_oracle.augmented_models(state, [p.detach().cpu() for p in acq.pareto_sets],
                                                          [p.detach().cpu() for p in acq.pareto_fronts])
        Xf = X.reshape(-1, d).cpu().double()
        ref, g_ref = jes_oracle.value_and_grad(models[id(acq)], acq.hypercell_bounds.detach().cpu().double(), Xf,
                                               acq.target_output_ix, acq.estimation_type == "LB2")
        err = (val.reshape(-1) - ref).abs()
        assert bool((err <= RTOL * ref.abs() + 4 * SPREAD_VALUE).all()), float(err.max())
        gerr = (g.reshape(-1, d) - g_ref).abs().amax(-1)
        assert bool((gerr <= RTOL * g_ref.abs().amax(-1) + 4 * SPREAD_GRAD).all()), float(gerr.max())
    assert len(models) == state.num_outputs  # one acquisition per objective, all on appended states
