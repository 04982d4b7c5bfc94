"""The staged forward envelope's set-up: the line coefficients of a workgroup's pairs are evaluated once, by one
wave (lane p: pair j0 + p) ahead of the staging barrier, and handed to the pairs' waves through LDS
(dkg_device.h envelope_body, COEF1).  Needs a real MI355X.

What can go wrong in the hand-over, and the shapes that reach it:

  * fewer pairs than waves (S = 3), a second workgroup per candidate holding a partial group (S = 11), whole
    groups (S = 8) and more than two workgroups (S = 24); lanes of the coefficient wave without a pair must not
    read past the weight rows nor write a slot;
  * one candidate and a batch that is no multiple of anything (B = 1, 17);
  * every output bucket, the padded ones included: m = 1, 2, 3, 4 and m = 5 in the M = 8 bucket, whose
    components i >= m carry zero weights; the full path and the decoupled one with the first and the last output
    as the target;
  * per-output constants that all differ (y_std = 1 + 0.25 i, y_mean = 0.3 i) and one output with noise 0;
  * a candidate on a discretisation point (Plan::dup): line 0 is rebuilt from the record after the barrier while
    the coefficients come from the candidate's own variance;
  * 2, 8 and 17 register slots (N = 90, 300, 560 by case).

Each case asserts the batched oracle at helpers' stated tolerance, and that five routes to the same numbers agree
bit for bit: the production forward, the walked (kg_pairs) forward, the walked pairs summed as the kernel sums them
(groups of 8 in pair order, each group's sum / S, the groups folded in order), three batches in one launch, and
DKG_PLAN_FORCE_WALK.  Further down: a plan of two targets against the single-target plans, and an acquisition
object whose weights and model are edited between calls."""

import dataclasses
import functools

import pytest
import torch

from dkg_amd import DiscreteKnowledgeGradient
from dkg_amd.gp_state import DeviceGPState
from dkg_amd.model import ModelListGPState
from helpers import ALL_FAMILIES, assert_within, grad_case, stated_tol, to_oracle
from oracle.discretekg import discrete_kg_batched, lines_batched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = {1: (37,), 2: (40, 33), 3: (37, 50, 23), 4: (33, 48, 17, 64), 5: (20, 31, 16, 45, 27)}
SLOT_N = {2: 90, 8: 300, 17: 560}
S_VALUES = (3, 8, 11, 24)
B_VALUES = (1, 17)
K = 3  # batches per batched launch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")


def _slots(m, S, B):
    return (2, 8, 17)[(m + S_VALUES.index(S) + B_VALUES.index(B)) % 3]


@functools.lru_cache(maxsize=None)
def _problem(m, S, B):
    """K * B candidates, the second one on a discretisation point; output 0 (Matern-1/2: K stays well conditioned
    without a nugget) has noise 0."""
    N = SLOT_N[_slots(m, S, B)]
    fam = ("M12",) + ALL_FAMILIES[:3]
    state, D, W, X = grad_case(m, 2 + (m + S) % 3, NS[m], fam, N, S, K * B, seed=900 + 40 * m + S + B)
    models = list(state.models)
    models[0] = dataclasses.replace(models[0], noise=0.0)
    X = X.clone()
    X[1] = D[N // 3]
    return ModelListGPState(*models), D, W, X


@functools.lru_cache(maxsize=None)
def _device_state(m, S, B):
    state, D, _, _ = _problem(m, S, B)
    return DeviceGPState(state, D, device=DEV)


def kernel_order_mean(pairs):
    """KG from the pair values [..., S] as the envelope stage sums them: G_g over each group of 8 consecutive
    pairs in pair order, G_g / S, the groups' terms folded in order (two groups: onto a zeroed accumulator)."""
    pairs = pairs.cpu()  # (on the host, by a tensor divisor: a true division, as the kernel's, not a reciprocal)
    S = pairs.shape[-1]
    total = None
    for g0 in range(0, S, 8):
        gsum = torch.zeros_like(pairs[..., 0])
        for q in range(g0, min(S, g0 + 8)):
            gsum = gsum + pairs[..., q]
        term = gsum / torch.full_like(gsum, float(S))
        total = term if total is None else total + term
    return total


def _targets(m):
    return [None] + sorted({0, m - 1})


@pytest.mark.parametrize("B", B_VALUES)
@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("m", sorted(NS))
def test_coefficient_handover(m, S, B):
    state, D, W, X = _problem(m, S, B)
    dstate = _device_state(m, S, B)
    om = to_oracle(state)
    Xd = X.to(DEV)
    n = X.shape[0]
    for target in _targets(m):
        plan = dstate.plan(W, target, n)
        geo = plan.envelope_geometry()
        assert (geo["slots"], geo["stream"], geo["sw"], geo["split"]) == (_slots(m, S, B), 0, min(8, S), -(-S // 8)), geo
        kg = plan.forward(Xd)
        kg_ref, _ = discrete_kg_batched(om, X, D, W, target)
        amax = lines_batched(om, X, D, W, target)[0].abs().amax((-1, -2))
        ratio = assert_within(kg, kg_ref, stated_tol(kg_ref, amax), f"m={m} S={S} B={B} target={target}: KG")
        kg_walked, pairs, _ = plan.forward_stats(Xd)
        assert torch.equal(kg, kg_walked), "production KG differs in bits from the walked (kg_pairs) forward"
        assert torch.equal(kg.cpu(), kernel_order_mean(pairs)), "KG is not the walked pairs summed in the kernel's order"
        kg_b = torch.full((n,), float("nan"), dtype=torch.double, device=DEV)
        plan.forward_batches_into(Xd, kg_b, B)
        assert torch.equal(kg, kg_b), f"{K} batches of {B} in one launch differ from one forward of {n}"
        kg_w = dstate.plan(W, target, n, force_walk=True).forward(Xd)
        assert torch.equal(kg, kg_w), "DKG_PLAN_FORCE_WALK differs in bits"
        # the coincident candidate is marked, and its lines are the plan's own
        a_dev, b_dev = plan.lines(Xd[1:2])
        k = 1 + SLOT_N[_slots(m, S, B)] // 3
        assert torch.equal(a_dev[..., 0], a_dev[..., k]) and torch.equal(b_dev[..., 0], b_dev[..., k])
        print(f"m={m} S={S} B={B} target={target}: KG worst err/tol {ratio:.3g}, {int((pairs > 0).sum())} of "
              f"{pairs.numel()} pairs with KG > 0")


@pytest.mark.parametrize("m,S,B", [(2, 11, 17), (3, 3, 1), (5, 24, 17)])
def test_two_target_plan(m, S, B):
    """dkg_plan_init_targets: the items (tau, b) of a plan of two targets take their target from the kernel
    arguments; each row is the single-target plan's, bit for bit, and the oracle's at the stated tolerance."""
    state, D, W, X = _problem(m, S, B)
    dstate = _device_state(m, S, B)
    om = to_oracle(state)
    Xd = X.to(DEV)
    targets = (None, m - 1)
    tplan = dstate.plan(W, None, X.shape[0], targets=targets)
    kg = tplan.forward(Xd)
    kg_walked, pairs, _ = tplan.forward_stats(Xd)
    assert kg.shape == (2, X.shape[0])
    assert torch.equal(kg, kg_walked) and torch.equal(kg.cpu(), kernel_order_mean(pairs))
    for tau, target in enumerate(targets):
        assert torch.equal(kg[tau], dstate.plan(W, target, X.shape[0]).forward(Xd)), f"target {target}"
        kg_ref, _ = discrete_kg_batched(om, X, D, W, target)
        amax = lines_batched(om, X, D, W, target)[0].abs().amax((-1, -2))
        assert_within(kg[tau], kg_ref, stated_tol(kg_ref, amax), f"two-target plan, target={target}: KG")


@pytest.mark.parametrize("target", [None, 1])
def test_plan_follows_edited_weights_and_a_refit_model(target):
    """One acquisition object through an in-place edit of its weights and a model with other output constants:
    the coefficients follow both (the plan is rebuilt by the fingerprints of dkg_amd/discretekg.py), against the
    oracle on the edited inputs and against a fresh object."""
    state, D, W, X = grad_case(3, 2, NS[3], ALL_FAMILIES, 300, 11, 17, seed=977)
    W = W.clone()
    acq = DiscreteKnowledgeGradient(state, D, W, target_output_ix=target, device=DEV)
    Xq = X.to(DEV).unsqueeze(-2)

    def check(what):
        om = to_oracle(acq.model)
        kg = acq(Xq)
        kg_ref, _ = discrete_kg_batched(om, X, D, acq.scalarisation_weights, target)
        amax = lines_batched(om, X, D, acq.scalarisation_weights, target)[0].abs().amax((-1, -2))
        assert_within(kg, kg_ref, stated_tol(kg_ref, amax), f"{what}, target={target}: KG")
        fresh = DiscreteKnowledgeGradient(acq.model, D, acq.scalarisation_weights.clone(), target_output_ix=target,
                                          device=DEV)
        assert torch.equal(kg, fresh(Xq)), f"{what}: a reused object differs from a fresh one"
        return kg

    kg0 = check("as built")
    W.mul_(torch.linspace(0.5, 2.0, W.shape[0], dtype=torch.double).reshape(-1, 1))   # in place: same tensor
    W[:, 0] += 0.25
    kg1 = check("weights edited in place")
    assert not torch.equal(kg0, kg1)
    models = [dataclasses.replace(mo, y_std=mo.y_std * (1.5 + 0.5 * i), y_mean=mo.y_mean - 0.7 * i,
                                  noise=mo.noise * (2.0 + i))
              for i, mo in enumerate(state.models)]
    acq.model = ModelListGPState(*models)
    kg2 = check("model with other output constants")
    assert not torch.equal(kg1, kg2)
