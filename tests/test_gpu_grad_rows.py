"""The gradient envelope with global rows (ForwardPlan grad_rows="auto" / "global"; DKG_PLAN_GRAD_GLOBAL_ROWS /
DKG_PLAN_FORCE_GLOBAL_ROWS): the candidates' Q_X and J rows read from the workspace instead of LDS.

1. Where the default gradient plan already streams its lines (N = 2200), "global" gives the bits of "staged", per
   output bucket, both flush branches (n_pad <= 256 and wider), unequal n per output (the zeroed tails), d = 1, 6
   and 16, targets None, 0 and m - 1, envelopes of more than 64 lines, and the list-overflow path.
2. Shapes the staged plan refuses build under "auto" and give the oracle's KG and dKG/dx.
3. Candidates on discretisation points and on training points.
4. A plan of several targets.
5. The host routes and the module switch.
6. The optimiser end to end on the stress model (m = 3, d = 2, n = 1024).

Tolerances are the project's stated ones, unchanged: KG 1e-6 |KG| + 64 eps max|a| (helpers.stated_tol), the
gradient 1e-6 |g| + 64 eps G per coordinate (helpers.grad_tol, G from helpers.grad_scale).
"""

import functools

import pytest
import torch

import dkg_amd
from dkg_amd import DiscreteKnowledgeGradient
from dkg_amd.errors import UnsupportedError
from dkg_amd.gp_state import DeviceGPState
from dkg_amd.optim import DiscreteKgOptimisationSpec, draw_sobol_samples
from helpers import (ALL_FAMILIES, assert_within, grad_case, grad_scale, grad_tol, oracle_value_and_grad,
                     stated_tol, to_oracle)
from oracle.discretekg import (calculate_epigraph_indices, discrete_kg_batched, discrete_kg_forward,
                               lines_batched)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# id -> grad_case arguments (m, d, ns, families, N, S, B, seed) and keywords.
# Streaming by N (2200 points: N + 1 > 2112 lines), S = 8, B = 5: the default gradient plan stages its rows and
# streams its lines, so "global" differs from it in the rows alone.  Short lengthscales and a noise of 0.05 to 0.1
# where the observations would otherwise pin the posterior down (KG = 0 and a flat envelope at every candidate).
STREAM = {
    "m1-d1-n40": ((1, 1, (40,), ("M52",), 2200, 8, 5, 101), dict(lengthscale=0.05, noise=0.05)),
    "m2-d2-n300": ((2, 2, (300, 300), ("M52", "M32"), 2200, 8, 5, 102), dict(lengthscale=0.05, noise=0.1)),
    "m3-mixed-d6-unequal": ((3, 6, (300, 40, 130), ALL_FAMILIES, 2200, 8, 5, 103), dict(lengthscale=0.35, noise=0.1)),
    "m4-d16-unequal-np128": ((4, 16, (40, 25, 120, 64), ALL_FAMILIES, 2200, 8, 5, 104), {}),
    "m5-d2-n45": ((5, 2, (40, 31, 16, 45, 27), ALL_FAMILIES, 2200, 8, 5, 105), dict(lengthscale=0.12, noise=0.1)),
    # d = 1, a grid of 2200 points, Matern-1/2: envelopes of more than 64 lines (the flush's second round)
    "long-d1": ((1, 1, (6,), ("M12",), 2200, 3, 5, 81), dict(lengthscale=1.0, noise=0.1, grid=True, mean_shift=1.2)),
    # Matern-1/2 beside Matern-5/2, for the candidates on discretisation and training points
    "m2-d3-M12": ((2, 3, (40, 40), ("M52", "M12"), 2200, 8, 5, 106), {}),
}
# (row, target): one row per output bucket; n = 40 (n_pad <= 256) and n = 300 (wider); unequal n; d in {1, 6, 16};
# targets None, 0 and m - 1
BIT_CASES = [("m1-d1-n40", None), ("m2-d2-n300", None), ("m2-d2-n300", 1), ("m3-mixed-d6-unequal", 0),
             ("m3-mixed-d6-unequal", 2), ("m4-d16-unequal-np128", 3), ("m5-d2-n45", None), ("m5-d2-n45", 4),
             ("long-d1", None)]

# Shapes whose staged gradient plan is refused for its LDS: (m, d, n, N, S, B, seed)
REFUSED = {
    "m8-d16-n128": (8, 16, 128, 50, 8, 4, 92),
    "m8-d16-n256": (8, 16, 256, 50, 8, 4, 91),
    "m3-d2-n1024": (3, 2, 1024, 50, 32, 4, 93),
    "m2-d6-n800": (2, 6, 800, 64, 8, 4, 94),
}


@functools.lru_cache(maxsize=None)
def _problem(case_id, B=None):
    if case_id in STREAM:
        args, kw = STREAM[case_id]
        args = args[:6] + (args[6] if B is None else B,) + args[7:]
        state, D, W, X = grad_case(*args, **kw)
    else:
        m, d, n, N, S, B0, seed = REFUSED[case_id]
        state, D, W, X = grad_case(m, d, (n,), ALL_FAMILIES, N, S, B0 if B is None else B, seed)
    return state, to_oracle(state), D, W, X


@functools.lru_cache(maxsize=None)
def _device_state(case_id):
    state, _, D, _, _ = _problem(case_id)
    return DeviceGPState(state, D, device=DEV)


def _reference(om, X, D, W, target, value_and_grad=oracle_value_and_grad):
    """KG, dKG/dx and their tolerances from the oracle."""
    kg_ref, g_ref = value_and_grad(om, X, D, W, target)
    amax = lines_batched(om, X, D, W, target)[0].abs().amax((-1, -2))
    return kg_ref, g_ref, stated_tol(kg_ref, amax), grad_tol(g_ref, grad_scale(om, X, D, W, target))


@functools.lru_cache(maxsize=None)
def _case_reference(case_id, target):
    _, om, D, W, X = _problem(case_id)
    return _reference(om, X, D, W, target)


def _check(what, kg, g, ref):
    kg_ref, g_ref, tol_kg, tol_g = ref
    assert g.shape == g_ref.shape
    kr = assert_within(kg, kg_ref, tol_kg, f"{what}: KG (stated tolerance)")
    gr = assert_within(g, g_ref, tol_g, f"{what}: dKG/dx")
    print(f"{what}: KG worst err/tol {kr:.3g}, gradient worst err/tol {gr:.3g}")


def _staged_and_global(case_id, target, X, **kw):
    """forward_grad of the default (staged rows) plan and of the global-rows plan, both streaming their lines."""
    _, _, _, W, _ = _problem(case_id)
    dstate = _device_state(case_id)
    staged = dstate.plan(W, target, X.shape[0], grad=True, **kw)
    glob = dstate.plan(W, target, X.shape[0], grad=True, grad_rows="global", **kw)
    assert staged.envelope_geometry()["stream"] == 1 and not staged.grad_rows_global
    assert glob.envelope_geometry() == staged.envelope_geometry() and glob.grad_rows_global
    return staged.forward_grad(X.to(DEV)), glob.forward_grad(X.to(DEV))


# ---- 1. the bits of the staged-rows streaming kernel

@pytest.mark.parametrize("case_id,target", BIT_CASES, ids=[f"{c}-t{t}" for c, t in BIT_CASES])
def test_global_rows_give_the_staged_bits(case_id, target):
    _, _, _, _, X = _problem(case_id)
    (kg_s, g_s), (kg_g, g_g) = _staged_and_global(case_id, target, X)
    assert torch.equal(kg_g, kg_s) and torch.equal(g_g, g_s)
    _check(f"{case_id} target={target}", kg_g, g_g, _case_reference(case_id, target))


def test_long_row_envelopes_pass_64_lines():
    """The d = 1 grid row has pairs whose upper envelope holds more than 64 lines, so their flush queue (one line
    per lane per round) takes its second round (the sizes are the reference walk's)."""
    _, om, D, W, X = _problem("long-d1")
    a, b = lines_batched(om, X, D, W, None)
    sizes = torch.tensor([[len(calculate_epigraph_indices(a[i, j], b[i, j])[0]) for j in range(a.shape[1])]
                          for i in range(a.shape[0])])
    print(f"long-d1 envelope sizes: {sorted(sizes.reshape(-1).tolist())}")
    assert int(sizes.max()) > 64


def test_force_walk_with_global_rows():
    case_id, target = "m3-mixed-d6-unequal", 2
    _, _, _, _, X = _problem(case_id)
    (kg_s, g_s), (kg_g, g_g) = _staged_and_global(case_id, target, X, force_walk=True)
    assert torch.equal(kg_g, kg_s) and torch.equal(g_g, g_s)
    _check(f"force-walk {case_id}", kg_g, g_g, _case_reference(case_id, target))


def test_rows_mode_is_checked():
    _, _, _, W, X = _problem("m1-d1-n40")
    with pytest.raises(ValueError, match="grad_rows"):
        _device_state("m1-d1-n40").plan(W, None, 4, grad=True, grad_rows="lds")
    # "auto" where the staged plan builds: that plan
    auto = _device_state("m1-d1-n40").plan(W, None, X.shape[0], grad=True, grad_rows="auto")
    assert not auto.grad_rows_global
    # a forward plan has no gradient rows
    assert not _device_state("m1-d1-n40").plan(W, None, 4, grad_rows="global").grad_rows_global


# ---- 2. shapes the staged plan refuses

@pytest.mark.parametrize("case_id", list(REFUSED))
def test_refused_shapes_under_auto(case_id):
    _, _, _, W, X = _problem(case_id)
    dstate = _device_state(case_id)
    with pytest.raises(UnsupportedError, match="gradient"):
        dstate.plan(W, None, X.shape[0], grad=True)
    plan = dstate.plan(W, None, X.shape[0], grad=True, grad_rows="auto")
    assert plan.grad_rows_global and plan.envelope_geometry()["stream"] == 1
    kg, g = plan.forward_grad(X.to(DEV))
    _check(f"{case_id} auto", kg, g, _case_reference(case_id, None))


# ---- 3. candidates on discretisation points and on training points

def _faithful(om, X, D, W, target):
    """The structure-faithful forward (the reference's joint posterior over [x; D] per candidate) with
    autograd: at x = z_k its lines 0 and k + 1 are exact copies (test_gpu_grad_matrix.py)."""
    Xr = X.clone().unsqueeze(-2).requires_grad_(True)
    kg = discrete_kg_forward(om, Xr, D, W, target)
    (g,) = torch.autograd.grad(kg.sum(), Xr)
    return kg.detach(), g.squeeze(-2)


@pytest.mark.parametrize("target", [None, 1])
def test_candidates_on_discretisation_and_training_points(target):
    """Three candidates on rows of D and four on training points of either output, the Matern-1/2 one included.
    The reference is the batched oracle (oracle_value_and_grad; its clamped distance gives the device's
    convention for the Matern-1/2 derivative at r = 0), except for the gradient on rows of D: there the oracle's
    lines 0 and k + 1 are copies only in the joint posterior over [x; D], whose torch.max shares the gradient of
    max a between them as the device does (test_gpu_grad_matrix.py), so the gradient's reference is that
    structure-faithful forward.  Its KG is not used: a 2201 x 2201 joint posterior with a Matern-1/2 output is
    itself 1.03 stated tolerances from the batched oracle at D[0] under target 1 (two CPU references, KG = 9.2e-7;
    the device is 5e-10 relative from the batched one)."""
    case_id = "m2-d3-M12"
    state, om, D, W, X = _problem(case_id)
    on_d = D[torch.tensor([0, 1100, 2199])]
    on_x = torch.cat([state.models[0].train_x[torch.tensor([0, 17])], state.models[1].train_x[torch.tensor([5, 39])]])
    Xc = torch.cat([on_d, on_x, X[:1]])
    (kg_s, g_s), (kg_g, g_g) = _staged_and_global(case_id, target, Xc)
    assert torch.equal(kg_g, kg_s) and torch.equal(g_g, g_s)
    ref_b, ref_f = _reference(om, on_d, D, W, target), _reference(om, on_d, D, W, target, _faithful)
    _check(f"on discretisation points target={target}", kg_g[:3], g_g[:3], (ref_b[0], ref_f[1], ref_b[2], ref_f[3]))
    _check(f"on training points target={target}", kg_g[3:], g_g[3:], _reference(om, Xc[3:], D, W, target))


# ---- 4. several targets

def test_targets_plan_rows_are_the_single_target_plans():
    case_id = "m3-d2-n1024"
    _, _, _, W, X = _problem(case_id)
    dstate = _device_state(case_id)
    targets = [None, 0, 1, 2]
    plan = dstate.plan(W, None, X.shape[0], grad=True, targets=targets, grad_rows="auto")
    assert plan.grad_rows_global
    kg, g = plan.forward_grad(X.to(DEV))
    assert kg.shape == (4, X.shape[0]) and g.shape == (4, X.shape[0], X.shape[1])
    for tau, t in enumerate(targets):
        single = dstate.plan(W, t, X.shape[0], grad=True, grad_rows="auto")
        assert single.grad_rows_global
        kg_1, g_1 = single.forward_grad(X.to(DEV))
        assert torch.equal(kg[tau], kg_1) and torch.equal(g[tau], g_1), f"target {t}"


# ---- 5. host routes and the module switch

@pytest.mark.parametrize("B", [4, 5], ids=["Bd64-kernel-arguments", "Bd80-pinned-copies"])
def test_host_route_gives_forward_grad_bits(B):
    case_id = "m8-d16-n128"
    _, _, _, W, X = _problem(case_id, B)
    plan = _device_state(case_id).plan(W, None, B, grad=True, grad_rows="auto")
    assert plan.grad_rows_global
    kg, g = plan.forward_grad(X.to(DEV))
    kg_h, g_h = plan.forward_grad_host(X)
    assert kg_h.device.type == "cpu" and g_h.shape == (B, 16)
    assert torch.equal(kg_h, kg.cpu()) and torch.equal(g_h, g.cpu())


def test_module_routes_follow_the_switch():
    case_id = "m8-d16-n128"
    state, _, D, W, X = _problem(case_id)
    kg, g = _device_state(case_id).plan(W, None, X.shape[0], grad=True, grad_rows="auto").forward_grad(X.to(DEV))
    acq = DiscreteKnowledgeGradient(state, D, W, device=DEV)
    assert dkg_amd.gradient_rows() == "staged"
    Xr = X.clone().to(DEV).requires_grad_(True)
    with pytest.raises(UnsupportedError, match=r'gradient.*set_gradient_rows\("auto"\)'):
        acq(Xr.unsqueeze(-2))
    with pytest.raises(UnsupportedError, match="gradient"):
        acq.value_and_grad_host(X.unsqueeze(-2))
    prev = dkg_amd.set_gradient_rows("auto")
    try:
        kg_m = acq(Xr.unsqueeze(-2))
        (g_m,) = torch.autograd.grad(kg_m.sum(), Xr)
        assert acq._plan_grad.grad_rows_global
        assert torch.equal(kg_m.detach(), kg) and torch.equal(g_m, g)
        Xh = X.clone().unsqueeze(-2).requires_grad_(True)  # the host route of forward
        kg_c = acq(Xh)
        (g_c,) = torch.autograd.grad(kg_c.sum(), Xh)
        assert torch.equal(kg_c.detach(), kg.cpu()) and torch.equal(g_c.squeeze(-2), g.cpu())
        kg_h, g_h = acq.value_and_grad_host(X.unsqueeze(-2))
        assert torch.equal(kg_h, kg.cpu()) and torch.equal(g_h.squeeze(-2), g.cpu())
        kg_t, g_t = acq.value_and_grad_host_targets(X.unsqueeze(-2), targets=[None, 7])
        assert torch.equal(kg_t[0], kg.cpu()) and torch.equal(g_t[0].squeeze(-2), g.cpu())
        Xt = X.clone().to(DEV).requires_grad_(True)
        kg_f = acq.forward_targets(Xt.unsqueeze(-2), targets=[None, 7])
        (g_f,) = torch.autograd.grad(kg_f[0].sum(), Xt)
        assert torch.equal(kg_f[0].detach(), kg) and torch.equal(g_f, g)
    finally:
        dkg_amd.set_gradient_rows(prev)
    # back under "staged" the acquisition refuses again (the plans are kept by mode)
    with pytest.raises(UnsupportedError, match="gradient"):
        acq.value_and_grad_host(X.unsqueeze(-2))
    # an acquisition of its own mode does not follow the module default
    own = DiscreteKnowledgeGradient(state, D, W, device=DEV, gradient_rows="auto")
    kg_o, g_o = own.value_and_grad_host(X.unsqueeze(-2))
    assert torch.equal(kg_o, kg.cpu()) and torch.equal(g_o.squeeze(-2), g.cpu())
    with pytest.raises(ValueError):
        DiscreteKnowledgeGradient(state, D, W, device=DEV, gradient_rows="lds")


# ---- 6. the optimiser end to end

def test_optimiser_on_the_stress_model_under_auto():
    """optimize_for_full_evaluation with the SMOKE settings on (m = 3, d = 2, n = 1024), which the default mode
    refuses: it returns, its value is the oracle's KG at the returned x, and no raw start has a larger KG (L-BFGS-B
    ascends from the best raw start, which initialize_q_batch always keeps; the comparison allows the stated
    tolerance of the two values compared, the device's and the oracle's)."""
    state, om, _, W, _ = _problem("m3-d2-n1024")
    spec = DiscreteKgOptimisationSpec(n_discretisation_points_per_axis=3, num_restarts=2, raw_samples=4,
                                      batch_limit=1, max_iter=200, device=DEV, seed=7)
    with pytest.raises(UnsupportedError, match="gradient"):
        spec.optimize_for_full_evaluation(state, 2, scalarisation_weights=W)
    prev = dkg_amd.set_gradient_rows("auto")
    try:
        x, value = spec.optimize_for_full_evaluation(state, 2, scalarisation_weights=W)
    finally:
        dkg_amd.set_gradient_rows(prev)
    assert x.shape == (1, 2) and bool(((x >= 0) & (x <= 1)).all())
    D = dkg_amd.make_torch_std_grid(3, 2, {"dtype": torch.double})
    bounds = torch.stack([torch.zeros(2, dtype=torch.double), torch.ones(2, dtype=torch.double)])
    raw = draw_sobol_samples(bounds, 4, 1, seed=7).squeeze(-2)
    pts = torch.cat([x.reshape(1, 2).double(), raw])
    kg_ref, _ = discrete_kg_batched(om, pts, D, W, None)  # five oracle forwards
    tol = stated_tol(kg_ref, lines_batched(om, pts, D, W, None)[0].abs().amax((-1, -2)))
    print(f"optimiser: x {x.tolist()} value {float(value):.6g}, oracle at x {float(kg_ref[0]):.6g}, "
          f"at the raw starts {kg_ref[1:].tolist()}")
    assert_within(value.reshape(1), kg_ref[:1], tol[:1], "KG at the optimiser's x")
    for i in range(1, 5):
        assert float(value) >= float(kg_ref[i] - tol[i]), f"raw start {i - 1}: {float(kg_ref[i])} > {float(value)}"
