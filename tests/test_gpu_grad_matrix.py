"""dKG/dx (dkg_plan_forward_grad) against the oracle's autograd across kernel families, lengthscales per
dimension, output buckets, dimension buckets and every envelope instantiation of the gradient path.

The rows are helpers.GRAD_MATRIX (seeded plain tensors, helpers.grad_case); tests/test_grad_matrix_oracle.py
checks the reference itself on the same rows (autograd against central differences, gradients far above the
tolerance's floor, envelopes longer than the flush queue where the row claims them).  Each row asserts, through
ForwardPlan.envelope_geometry, the envelope kernel it is there for: the staged 2 / 8 / 17 / 33-slot kernels, the
streaming one (by N, or by the gradient's LDS at a small N) and the number of workgroups per candidate.

The long-envelope rows (d = 1, 1000 grid points, envelopes of 66 to 447 lines) are the ones that found the
gradient flush evaluating the kernel-derivative term of only the first 64 queued lines (dkg_device.h flush():
one line per lane, a queue of up to 128): every pair with more than 64 envelope lines had a wrong gradient.

Tolerances are the project's stated ones, unchanged: KG 1e-6 |KG| + 64 eps max|a| (helpers.stated_tol), the
gradient 1e-6 |g| + 64 eps G per coordinate (helpers.grad_tol, G from helpers.grad_scale).
"""

import functools

import pytest
import torch

from dkg_amd import DiscreteKnowledgeGradient
from dkg_amd.errors import UnsupportedError
from dkg_amd.gp_state import DeviceGPState
from helpers import (ALL_FAMILIES, GRAD_CASES, GRAD_ROWS, assert_within, grad_case, grad_row_problem, grad_scale,
                     grad_tol, oracle_value_and_grad, stated_tol, to_oracle)
from oracle.discretekg import discrete_kg_batched, discrete_kg_forward, lines_batched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one row per output bucket M = 1, 2, 3, 4, 8 for the bit-for-bit checks
BUCKET_ROWS = ["M1", "family-M32", "M3-mixed", "M4", "M8-padded-m5"]


@functools.lru_cache(maxsize=None)
def _problem(row_id, B=None):
    state, D, W, X = grad_row_problem(GRAD_ROWS[row_id], B)
    return state, to_oracle(state), D, W, X


@functools.lru_cache(maxsize=None)
def _device_state(row_id):
    state, _, D, _, _ = _problem(row_id)
    return DeviceGPState(state, D, device=DEV)


def _reference(om, X, D, W, target, value_and_grad=oracle_value_and_grad):
    """KG, dKG/dx and their tolerances from the oracle (computed once per case)."""
    kg_ref, g_ref = value_and_grad(om, X, D, W, target)
    amax = lines_batched(om, X, D, W, target)[0].abs().amax((-1, -2))
    return kg_ref, g_ref, stated_tol(kg_ref, amax), grad_tol(g_ref, grad_scale(om, X, D, W, target))


@functools.lru_cache(maxsize=None)
def _row_reference(row_id, target):
    _, om, D, W, X = _problem(row_id)
    return _reference(om, X, D, W, target)


def _check(what, kg, g, ref):
    kg_ref, g_ref, tol_kg, tol_g = ref
    assert g.shape == g_ref.shape
    kr = assert_within(kg, kg_ref, tol_kg, f"{what}: KG of the gradient plan (stated tolerance)")
    gr = assert_within(g, g_ref, tol_g, f"{what}: dKG/dx")
    print(f"{what}: KG worst err/tol {kr:.3g}, gradient worst err/tol {gr:.3g}")


def _assert_geometry(plan, row):
    geo = plan.envelope_geometry()
    assert geo["stream"] == row["stream"] and geo["slots"] == row["slots"] and geo["split"] == row["split"], (
        f"{row['id']}: envelope {geo}, expected slots {row['slots']} stream {row['stream']} split {row['split']}")
    assert geo["sw"] == min(8, row["S"])


@pytest.mark.parametrize("row_id,target", GRAD_CASES, ids=[f"{r}-t{t}" for r, t in GRAD_CASES])
def test_grad_matrix_vs_oracle(row_id, target):
    row = GRAD_ROWS[row_id]
    _, _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    plan = dstate.plan(W, target, X.shape[0], grad=True)
    _assert_geometry(plan, row)
    if row_id.startswith("stream-by-LDS"):  # the LDS of the gradient alone makes it stream: the forward plan is staged
        fwd = dstate.plan(W, target, X.shape[0]).envelope_geometry()
        assert fwd["stream"] == 0 and fwd["slots"] == 8
    kg, g = plan.forward_grad(X.to(DEV))
    _check(f"{row_id} target={target}", kg, g, _row_reference(row_id, target))


@pytest.mark.parametrize("row_id", BUCKET_ROWS)
def test_module_route_and_single_rows_give_the_same_bits(row_id):
    """Per output bucket: DiscreteKnowledgeGradient + autograd gives forward_grad's bits, and rows 0..4
    evaluated alone equal the batch's rows bit for bit (test_grad_headline_batch_consistent at m = 2)."""
    row = GRAD_ROWS[row_id]
    target = row["targets"][-1]
    state, _, D, W, X = _problem(row_id)
    plan = _device_state(row_id).plan(W, target, X.shape[0], grad=True)
    kg, g = plan.forward_grad(X.to(DEV))
    acq = DiscreteKnowledgeGradient(state, D, W, target_output_ix=target, device=DEV)
    Xr = X.clone().to(DEV).requires_grad_(True)
    kg_m = acq(Xr.unsqueeze(-2))
    (g_m,) = torch.autograd.grad(kg_m.sum(), Xr)
    assert torch.equal(kg_m.detach(), kg) and torch.equal(g_m, g)
    kg_s, g_s = plan.forward_grad(X[:5].to(DEV))
    assert torch.equal(kg_s, kg[:5]) and torch.equal(g_s, g[:5])


@pytest.mark.parametrize("family", ALL_FAMILIES)
@pytest.mark.parametrize("target", [None, 1])
def test_candidates_on_training_points(family, target):
    """Candidates exactly on training points of one output (r = 0 against a training row): the Matern-1/2
    term's gradient there is 0 by the device's convention (kernel_dprofile_t: r^2 <= 1e-30), the one the
    oracle's clamped cdist gives; the other families are smooth there."""
    row_id = f"family-{family}"
    state, om, D, W, X = _problem(row_id)
    X = X.clone()
    X[:3] = state.models[0].train_x[torch.tensor([0, 17, 39])]
    X[3] = state.models[1].train_x[5]
    plan = _device_state(row_id).plan(W, target, X.shape[0], grad=True)
    kg, g = plan.forward_grad(X.to(DEV))
    _check(f"on training points {family} target={target}", kg, g, _reference(om, X, D, W, target))


def _faithful(om, X, D, W, target):
    """The structure-faithful forward (the reference's joint posterior over [x; D] per candidate) with
    autograd: at x = z_k its lines 0 and k + 1 are exact copies (test_gpu_grad.py)."""
    Xr = X.clone().unsqueeze(-2).requires_grad_(True)
    kg = discrete_kg_forward(om, Xr, D, W, target)
    (g,) = torch.autograd.grad(kg.sum(), Xr)
    return kg.detach(), g.squeeze(-2)


@pytest.mark.parametrize("target", [None, 1])
def test_candidates_on_discretisation_points_streaming(target):
    """Three candidates on rows of D under the streaming gradient envelope (N = 2200)."""
    row_id = "stream-by-N"
    _, om, D, W, X = _problem(row_id)
    X = torch.cat([D[torch.tensor([0, 1100, 2199])], X[:2]])
    plan = _device_state(row_id).plan(W, target, X.shape[0], grad=True)
    assert plan.envelope_geometry()["stream"] == 1
    kg, g = plan.forward_grad(X.to(DEV))
    _check(f"on discretisation points, streaming, target={target}", kg, g,
           _reference(om, X, D, W, target, _faithful))


@pytest.mark.parametrize("row_id", ["M3-mixed", "M8-padded-m5", "M8-full"])
def test_force_walk_value_and_grad(row_id):
    """DKG_PLAN_FORCE_WALK (the envelope's list-overflow path for every pair) in the M = 3 and M = 8 buckets:
    the forward plan's KG and the gradient plan's KG and dKG/dx."""
    row = GRAD_ROWS[row_id]
    _, _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    for target in row["targets"]:
        ref = _row_reference(row_id, target)
        kg_f = dstate.plan(W, target, X.shape[0], force_walk=True).forward(X.to(DEV))
        assert_within(kg_f, ref[0], ref[2], f"{row_id} target={target}: force-walk KG")
        kg, g = dstate.plan(W, target, X.shape[0], grad=True, force_walk=True).forward_grad(X.to(DEV))
        _check(f"force-walk {row_id} target={target}", kg, g, ref)


@pytest.mark.parametrize("row_id,B", [("d16", 4), ("d1", 64), ("d16", 5)], ids=["d16-B4", "d1-B64", "d16-B5"])
def test_host_route_at_the_argument_limit(row_id, B):
    """forward_grad_host at B d = DKG_XARG_MAX = 64 (candidates in the first kernel's arguments) and one
    candidate past it (pinned copies): the bits of forward_grad."""
    _, _, _, W, X = _problem(row_id, B)
    plan = _device_state(row_id).plan(W, None, B, grad=True)
    kg, g = plan.forward_grad(X.to(DEV))
    kg_h, g_h = plan.forward_grad_host(X)
    assert kg_h.device.type == "cpu" and g_h.shape == (B, X.shape[1])
    assert torch.equal(kg_h, kg.cpu()) and torch.equal(g_h, g.cpu())


def test_gradient_plan_refuses_what_its_lds_cannot_hold():
    """m = 8, d = 16, n = 256: the gradient envelope's LDS exceeds 160 KiB even when streaming, so the
    gradient plan raises UnsupportedError naming the gradient; the forward plan of the same model builds
    and gives the oracle's KG."""
    state, D, W, X = grad_case(8, 16, (256,), ALL_FAMILIES, 50, 8, 4, seed=91)
    dstate = DeviceGPState(state, D, device=DEV)
    with pytest.raises(UnsupportedError, match="gradient"):
        dstate.plan(W, None, 4, grad=True)
    om = to_oracle(state)
    kg_ref, _ = discrete_kg_batched(om, X, D, W, None)
    amax = lines_batched(om, X, D, W, None)[0].abs().amax((-1, -2))
    kg = dstate.plan(W, None, 4).forward(X.to(DEV))
    r = assert_within(kg, kg_ref, stated_tol(kg_ref, amax), "forward KG at m = 8, d = 16, n = 256")
    print(f"m=8 d=16 n=256 forward: KG worst err/tol {r:.3g}")
