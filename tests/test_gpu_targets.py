"""Plans of several targets (dkg_plan_init_targets): one call evaluates KG, and dKG/dx, of the same candidates
under T targets with the cross and covariance stages run once.

The requirement is bit equality: row (tau, b) of a T-target call has exactly the bits a single-target plan of
targets[tau], built on the same DeviceGPState, writes for candidate b -- KG, kg_pairs, hull sizes and the
gradient, on every envelope instantiation (staged 2 / 8 / 17 / 33 slots, streaming with and without the sample
chain, the gradient envelope), for one, two and three workgroups per item, for candidates on discretisation
points, and on a second and third call of the same plan with another B (the per-item accumulators and tickets
are cleared by the cross stage of every call).  The rows are helpers.GRAD_ROWS; one case adds S = 12 (two
workgroups per item meeting in one atomic add onto the zeroed accumulator), which no row has.  One oracle
parity check (M3-mixed, stated tolerances) shows the rows are right, not only equal to the single plans.
"""

import functools

import pytest
import torch

from dkg_amd import DiscreteKnowledgeGradient, _lib, make_torch_std_grid
from dkg_amd.errors import UnsupportedError
from dkg_amd.gp_state import DeviceGPState
from dkg_amd.synthetic import WORKLOADS, make_problem
from helpers import (GRAD_ROWS, assert_within, grad_case, grad_row_problem, grad_scale, grad_tol,
                     oracle_value_and_grad, stated_tol, to_oracle)
from oracle.discretekg import lines_batched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def all_targets(m):
    return [None] + list(range(m))


@functools.lru_cache(maxsize=None)
def _problem(row_id, B=None):
    if row_id == "S12":  # 8 < S <= 16: two workgroups per item, one atomic add each onto the cleared accumulator
        return grad_case(2, 3, (40, 40), ("M52", "M32"), 200, 12, 19 if B is None else B, seed=71)
    return grad_row_problem(GRAD_ROWS[row_id], B)


@functools.lru_cache(maxsize=None)
def _device_state(row_id):
    state, D, _, _ = _problem(row_id)
    return DeviceGPState(state, D, device=DEV)


def _singles_forward(dstate, W, X, targets, **flags):
    return torch.stack([dstate.plan(W, t, X.shape[0], **flags).forward(X) for t in targets])


def _singles_grad(dstate, W, X, targets):
    outs = [dstate.plan(W, t, X.shape[0], grad=True).forward_grad(X) for t in targets]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def _assert_same_geometry(tplan, single, row_id, grad):
    """The T-target plan launches the single-target plan's envelope kernel with its waves and workgroups per
    item, and that is the instantiation the row is there for."""
    geo = tplan.envelope_geometry()
    assert geo == single.envelope_geometry()
    row = GRAD_ROWS.get(row_id)
    if row is not None and (grad or not row_id.startswith("stream-by-LDS")):
        assert (geo["slots"], geo["stream"], geo["split"]) == (row["slots"], row["stream"], row["split"]), geo


FORWARD_CASES = [
    ("M1", (None,)), ("M1", (None, 0)),
    ("family-M52", (None, 0, 1)), ("family-M52", (1, None)),
    ("M3-mixed", tuple(all_targets(3))),
    ("M8-padded-m5", tuple(all_targets(5))),
    ("S24", (None, 0, 1)),
    ("S12", (None, 0, 1)),
    ("slots2-B1", (None, 0, 1)),
    ("slots33", (None, 0, 1)),
    ("stream-by-N", (None, 0, 1)),
]
GRAD_CASES = [c for c in FORWARD_CASES if c[0] != "slots33"] + [
    ("stream-by-LDS-m3", tuple(all_targets(3))),
    ("long-M12-m2", (None, 0, 1)),
]


def _ids(cases):
    return [f"{r}-{'_'.join('all' if t is None else str(t) for t in ts)}" for r, ts in cases]


@pytest.mark.parametrize("row_id,targets", FORWARD_CASES, ids=_ids(FORWARD_CASES))
def test_forward_rows_are_the_single_target_bits(row_id, targets):
    _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    Xd = X.to(DEV)
    tplan = dstate.plan(W, None, X.shape[0], targets=targets)
    _assert_same_geometry(tplan, dstate.plan(W, targets[0], X.shape[0]), row_id, grad=False)
    kg = tplan.forward(Xd)
    ref = _singles_forward(dstate, W, Xd, targets)
    assert kg.shape == (len(targets), X.shape[0])
    assert torch.equal(kg, ref)
    # the host route of the same plan (pinned copies each way)
    kg_h = tplan.forward_host(X)
    assert kg_h.device.type == "cpu" and torch.equal(kg_h, ref.cpu())


@pytest.mark.parametrize("row_id,targets", GRAD_CASES, ids=_ids(GRAD_CASES))
def test_grad_rows_are_the_single_target_bits(row_id, targets):
    _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    Xd = X.to(DEV)
    tplan = dstate.plan(W, None, X.shape[0], grad=True, targets=targets)
    _assert_same_geometry(tplan, dstate.plan(W, targets[0], X.shape[0], grad=True), row_id, grad=True)
    kg, g = tplan.forward_grad(Xd)
    kg_ref, g_ref = _singles_grad(dstate, W, Xd, targets)
    assert kg.shape == (len(targets), X.shape[0]) and g.shape == (len(targets),) + tuple(X.shape)
    assert torch.equal(kg, kg_ref)
    assert torch.equal(g, g_ref)


def test_streaming_overflow_path():
    """DKG_PLAN_NO_CHAIN: the streaming envelope without its sample chain (extremes from the streamed lines,
    quickhull refinement, walks) for every pair of every item."""
    _, _, W, X = _problem("stream-by-N")
    dstate = _device_state("stream-by-N")
    Xd = X.to(DEV)
    targets = (None, 0, 1)
    tplan = dstate.plan(W, None, X.shape[0], no_chain=True, targets=targets)
    assert tplan.envelope_geometry()["stream"] == 1
    assert torch.equal(tplan.forward(Xd), _singles_forward(dstate, W, Xd, targets, no_chain=True))


def test_candidates_on_discretisation_points():
    """Three candidates on rows of D: line 0 of each of their items is the copy of record k (Plan::dup)."""
    _, D, W, X = _problem("family-M52")
    X = X.clone()
    X[:3] = D[torch.tensor([0, 100, 199])]
    dstate = _device_state("family-M52")
    Xd = X.to(DEV)
    targets = (None, 0, 1)
    assert torch.equal(dstate.plan(W, None, 19, targets=targets).forward(Xd), _singles_forward(dstate, W, Xd, targets))
    kg, g = dstate.plan(W, None, 19, grad=True, targets=targets).forward_grad(Xd)
    kg_ref, g_ref = _singles_grad(dstate, W, Xd, targets)
    assert torch.equal(kg, kg_ref) and torch.equal(g, g_ref)


@pytest.mark.parametrize("row_id", ["family-M52", "S24", "stream-by-N"])
def test_pairs_and_hull_sizes_per_item(row_id):
    _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    Xd = X.to(DEV)
    targets = (1, None, 0)
    kg, pairs, hull = dstate.plan(W, None, 32, targets=targets).forward_stats(Xd)  # capacity above B: bpad = 32
    B, S = X.shape[0], W.shape[0]
    assert kg.shape == (3, B) and pairs.shape == (3, B, S) and hull.shape == (3, B, S) and hull.dtype == torch.int32
    for tau, t in enumerate(targets):
        kg_s, pairs_s, hull_s = dstate.plan(W, t, 32).forward_stats(Xd)
        assert torch.equal(kg[tau], kg_s) and torch.equal(pairs[tau], pairs_s) and torch.equal(hull[tau], hull_s)


@pytest.mark.parametrize("row_id", ["S12", "S24"])
def test_one_plan_called_with_changing_batch_sizes(row_id):
    """B = 19, then 5, then 19 on one plan: the items' accumulators (S12: atomic adds onto them) and tickets
    (S24: last-arriver counts) are cleared by every call's cross stage, whatever the last call's B was."""
    _, _, W, X = _problem(row_id)
    dstate = _device_state(row_id)
    Xd = X.to(DEV)
    targets = (None, 0, 1)
    fwd = dstate.plan(W, None, 19, targets=targets)
    grad = dstate.plan(W, None, 19, grad=True, targets=targets)
    ref = {B: (_singles_forward(dstate, W, Xd[:B], targets), _singles_grad(dstate, W, Xd[:B], targets))
           for B in (19, 5)}
    for B in (19, 5, 19):
        assert torch.equal(fwd.forward(Xd[:B]), ref[B][0]), B
        kg, g = grad.forward_grad(Xd[:B])
        assert torch.equal(kg, ref[B][1][0]) and torch.equal(g, ref[B][1][1]), B
    # forward_into on a caller's buffer that holds stale values
    kg = torch.full((3, 19), 7.0, dtype=torch.double, device=DEV)
    fwd.forward_into(Xd, kg)
    assert torch.equal(kg, ref[19][0])


@pytest.mark.parametrize("B", [4, 5])
def test_host_route_at_the_argument_limit(B):
    """forward_grad_host at B d = DKG_XARG_MAX = 64 (the shared candidates in the first kernel's arguments, the
    envelope writing [kg | dkg_dx] of all T B items into pinned memory) and one candidate past it."""
    _, _, W, X = _problem("d16", B)
    dstate = _device_state("d16")
    targets = (None, 0, 1)
    assert (B * X.shape[1] <= _lib.DKG_XARG_MAX) == (B == 4)
    kg_h, g_h = dstate.plan(W, None, B, grad=True, targets=targets).forward_grad_host(X)
    assert kg_h.device.type == "cpu" and kg_h.shape == (3, B) and g_h.shape == (3, B, 16)
    singles = [dstate.plan(W, t, B, grad=True).forward_grad_host(X) for t in targets]
    assert torch.equal(kg_h, torch.stack([s[0] for s in singles]))
    assert torch.equal(g_h, torch.stack([s[1] for s in singles]))
    kg_d, g_d = _singles_grad(dstate, W, X.to(DEV), targets)
    assert torch.equal(kg_h, kg_d.cpu()) and torch.equal(g_h, g_d.cpu())


def test_host_route_sums_in_order_with_three_workgroups_per_item():
    """S24 at B = 2: the pinned host copy of a folded (ordered) combine, per item."""
    _, _, W, X = _problem("S24", 2)
    dstate = _device_state("S24")
    targets = (None, 0, 1)
    kg_h, g_h = dstate.plan(W, None, 2, grad=True, targets=targets).forward_grad_host(X)
    kg_d, g_d = _singles_grad(dstate, W, X.to(DEV), targets)
    assert torch.equal(kg_h, kg_d.cpu()) and torch.equal(g_h, g_d.cpu())


def test_fp32_plan():
    model, D, X, W = make_problem(WORKLOADS["small"])
    dstate = DeviceGPState(model, D, device=DEV)
    Xd = X.to(DEV)
    targets = (None, 0, 1)
    kg = dstate.plan(W, None, X.shape[0], f32=True, targets=targets).forward(Xd)
    assert torch.equal(kg, _singles_forward(dstate, W, Xd, targets, f32=True))
    with pytest.raises(UnsupportedError):
        dstate.plan(W, None, X.shape[0], f32=True, grad=True, targets=targets)


def test_oracle_parity_of_every_row():
    """M3-mixed, all four targets, against the oracle's KG and autograd gradient at the stated tolerances."""
    state, D, W, X = _problem("M3-mixed")
    om = to_oracle(state)
    targets = all_targets(3)
    kg, g = _device_state("M3-mixed").plan(W, None, X.shape[0], grad=True, targets=targets).forward_grad(X.to(DEV))
    for tau, t in enumerate(targets):
        kg_ref, g_ref = oracle_value_and_grad(om, X, D, W, t)
        amax = lines_batched(om, X, D, W, t)[0].abs().amax((-1, -2))
        kr = assert_within(kg[tau], kg_ref, stated_tol(kg_ref, amax), f"target {t}: KG")
        gr = assert_within(g[tau], g_ref, grad_tol(g_ref, grad_scale(om, X, D, W, t)), f"target {t}: dKG/dx")
        print(f"target {t}: KG worst err/tol {kr:.3g}, gradient worst err/tol {gr:.3g}")


def test_unsupported_combinations_and_lines():
    _, _, W, X = _problem("family-M52")
    dstate = _device_state("family-M52")
    Xd = X.to(DEV)
    with pytest.raises(UnsupportedError, match="DKG_PLAN_FUSED"):
        dstate.plan(W, None, 19, fused=True, targets=(None, 0))
    tplan = dstate.plan(W, None, 38, targets=(1, None))
    with pytest.raises(UnsupportedError, match="dkg_plan_forward_batches"):
        tplan.forward_batches_into(torch.cat([Xd, Xd]), torch.empty(2, 38, dtype=torch.double, device=DEV), 19)
    with pytest.raises(ValueError):
        dstate.plan(W, None, 19, targets=(0, 0))
    with pytest.raises(ValueError):
        dstate.plan(W, None, 19, targets=(2,))
    a, b = tplan.lines(Xd)  # the lines of targets[0]
    a1, b1 = dstate.plan(W, 1, 38).lines(Xd)
    assert torch.equal(a, a1) and torch.equal(b, b1)
    # a fused single-target plan built through the targets entry is the plain fused plan
    assert dstate.plan(W, None, 19, fused=True, targets=(0,)).fused == dstate.plan(W, 0, 19, fused=True).fused


def test_module_forward_targets_and_host_value_and_grad():
    """forward_targets on host X and on device X: the bits of m + 1 single acquisitions, backward of row tau
    (a one-hot incoming gradient) that acquisition's autograd gradient; value_and_grad_host_targets the same."""
    state, D, W, X = _problem("family-M52")
    X = X[:6]
    acq = DiscreteKnowledgeGradient(state, D, W, device=DEV)
    targets = all_targets(2)
    singles = [DiscreteKnowledgeGradient(state, D, W, target_output_ix=t, device=DEV) for t in targets]
    for dev in ("cpu", DEV):
        Xr = X.clone().to(dev).unsqueeze(-2).requires_grad_(True)
        kg = acq.forward_targets(Xr)
        assert kg.shape == (3, 6) and kg.device == Xr.device
        for tau, s in enumerate(singles):
            Xs = X.clone().to(dev).unsqueeze(-2).requires_grad_(True)
            kg_s = s(Xs)
            (g_s,) = torch.autograd.grad(kg_s.sum(), Xs)
            onehot = torch.zeros_like(kg)
            onehot[tau] = 1.0
            (g,) = torch.autograd.grad(kg, Xr, grad_outputs=onehot, retain_graph=True)
            assert torch.equal(kg[tau].detach(), kg_s.detach()), (dev, tau)
            assert torch.equal(g, g_s), (dev, tau)
        with torch.no_grad():
            assert torch.equal(acq.forward_targets(X.to(dev).unsqueeze(-2)), kg.detach())
    kg_h, g_h = acq.value_and_grad_host_targets(X.unsqueeze(-2))
    assert kg_h.shape == (3, 6) and g_h.shape == (3, 6, 1, 3)
    for tau, s in enumerate(singles):
        kg_s, g_s = s.value_and_grad_host(X.unsqueeze(-2))
        assert torch.equal(kg_h[tau], kg_s) and torch.equal(g_h[tau], g_s)
    # a subset with a negative index, and the plans cached by target tuple
    sub = acq.forward_targets(X.to(DEV).unsqueeze(-2), targets=[-1, None])
    assert torch.equal(sub, torch.stack([kg[2], kg[0]]).detach().to(DEV))
    assert ((1, None), False) in acq._plans_targets and ((None, 0, 1), True) in acq._plans_targets
    with pytest.raises(IndexError):
        acq.forward_targets(X.unsqueeze(-2), targets=[0, 2])
    with pytest.raises(ValueError):
        acq.forward_targets(X.unsqueeze(-2), targets=[1, -1])


def test_joint_decoupled_search_matches_the_oracle_run():
    """optimize_for_single_objective(joint=True) on the small workload under the SMOKE settings (3 grid points
    per axis, 2 restarts, 4 raw samples, batch_limit 1, seeded): the device run evaluates all objectives on one
    acquisition through value_and_grad_host_targets; the same spec with the oracle's KG injected through
    acq_factory combines one acquisition per objective.  Same objective, x within 1e-4, value within
    1e-6 relative + 1e-8 (the thresholds of test_gpu_optim.py / test_gpu_bo_smoke.py)."""
    from dkg_amd.optim import DiscreteKgOptimisationSpec
    from smoke_oracle import oracle_acq_factory

    model, _, _, W = make_problem(WORKLOADS["small"])
    W = W[:4]
    costs = [1.0, 2.0]
    out = {}
    for name, kw in (("device", dict(device=DEV)), ("oracle", dict(acq_factory=oracle_acq_factory))):
        spec = DiscreteKgOptimisationSpec(n_discretisation_points_per_axis=3, num_restarts=2, raw_samples=4,
                                          batch_limit=1, max_iter=200, seed=3, **kw)
        torch.manual_seed(11)  # the Boltzmann draw of the starting points reads the global generator
        out[name] = spec.optimize_for_single_objective(model, costs, 2, scalarisation_weights=W, joint=True)
    (x, i, v), (x_o, i_o, v_o) = out["device"], out["oracle"]
    print(f"joint: device x={x.tolist()} i={i} v={float(v):.12g}; oracle x={x_o.tolist()} i={i_o} v={float(v_o):.12g}")
    assert i == i_o and x.shape == x_o.shape == (1, 2)
    assert float((x - x_o).abs().max()) <= 1e-4, (x, x_o)
    assert float(v) == pytest.approx(float(v_o), rel=1e-6, abs=1e-8)
    # the value returned is the winning objective's own KG per cost at x
    acq = DiscreteKnowledgeGradient(model, make_torch_std_grid(3, 2, {"dtype": torch.double}), W,
                                    target_output_ix=i, device=DEV)
    with torch.no_grad():
        assert float(acq(x.unsqueeze(0))) / costs[i] == pytest.approx(float(v), rel=1e-12)
