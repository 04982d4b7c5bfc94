"""The hypervolume knowledge gradient on the device (csrc/dkg_hvkg.hip, dkg_amd/hvkg.py) against the fp64
restatement of tests/hvkg_oracle.py, on the cases of tests/hvkg_cases.py.

Bounds, per restart: the fantasised means within the moment bound of DESIGN.md 8d, ``1e-8 y_std (|c| + sqrt(s))`` per
entry; the value within ``1e-6 mean_f HV_f / cost + 4 spread_v`` (the scale is the uncancelled hypervolume: HV -
current_value may vanish); the gradient within ``1e-6 max_j |g_j| + 4 spread_g``; the spreads are the restatement as
given against every output's training rows reversed.  ``dkg_hypervolume`` alone is held to
``64 eps prod_i (ideal_i - ref_i)``, the rounding of at most Np^2 products of coordinate differences.
"""


import pytest
import torch

import hvkg_cases as hc
import hvkg_oracle as ho

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -52


def make_acq(cid, device=DEV, **over):
    from dkg_amd.hvkg import qHypervolumeKnowledgeGradient

    c = hc.CASES[cid]
    state, z, X, ref = hc.problem(cid)
    mask = torch.zeros(1, c["m"], dtype=torch.bool)
    mask[0, list(c["mask"])] = True
    kw = dict(num_fantasies=c["Nf"], num_pareto=c["Np"], X_evaluation_mask=mask, current_value=c["current"],
              cost_aware_utility=c["costs"], base_samples=z, device=device)
    kw.update(over)
    return qHypervolumeKnowledgeGradient(state, kw.pop("ref_point", ref), **kw), X


def worst(err, tol):
    return float((err / tol).max())


@pytest.mark.parametrize("cid", list(hc.CASES))
def test_fantasy_means_match_the_oracle(cid):
    acq, X = make_acq(cid)
    state = hc.problem(cid)[0]
    got = acq.fantasy_means(X).cpu()
    ref = hc.reference(cid)["Y"]
    tol = torch.tensor([1e-8 * o.y_std * (abs(o.mean_constant) + o.outputscale ** 0.5) for o in state.models])
    err = (got - ref).abs()
    print(f"{cid}: worst |dY| / bound = {worst(err, tol):.3g}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("cid", list(hc.CASES))
def test_value_and_gradient_match_the_oracle(cid):
    acq, X = make_acq(cid)
    r = hc.reference(cid)
    vtol, gtol = hc.bounds(cid)
    val, grad = acq.value_and_grad_host(X)
    B = X.shape[0]
    verr = (val - r["acq"]).abs()
    gerr = (grad - r["grad"]).reshape(B, -1).abs().max(dim=1).values
    print(f"{cid}: value err/bound {worst(verr, vtol):.3g}, gradient err/bound {worst(gerr, gtol):.3g}, "
          f"kink margin {r['kink']:.3g}")
    assert bool((verr <= vtol).all())
    assert bool((gerr <= gtol).all())


# ---- conventions at kinks ------------------------------------------------------------------------------------

def _classify(Y, ref):
    """Per point of Y [B, Nf, Np, m]: (strictly dominated within its fantasy, not strictly above ref)."""
    ge = (Y[..., None, :, :] >= Y[..., :, None, :]).all(-1) & (Y[..., None, :, :] > Y[..., :, None, :]).all(-1)
    dominated = ge.any(-1)  # some other point of the fantasy is larger in every objective
    below = ~(Y > ref).all(-1)
    return dominated, below


def test_points_that_add_nothing_get_exactly_zero():
    """A fantasy with a strictly dominated point and one with a point below ref in one objective: those rows of
    the gradient are exactly 0 (the oracle's own rows there are rounding, not 0: its kernels centre the inputs)."""
    cid = "n256-d2-m2-f9p8"
    acq, X = make_acq(cid)
    r = hc.reference(cid)
    ref = hc.problem(cid)[3]
    dominated, below = _classify(r["Y"], ref)
    one_below = ((r["Y"] > ref).sum(-1) == r["Y"].shape[-1] - 1)
    assert int(dominated.sum()) > 0 and int(one_below.sum()) > 0  # the inputs hold both kinds
    _, grad = acq.value_and_grad_host(X)
    rows = grad[:, 1:].reshape(dominated.shape + (grad.shape[-1],))
    assert float(rows[dominated | below].abs().max()) == 0.0
    assert float(rows[~(dominated | below)].abs().max()) > 0.0


def test_every_point_below_ref():
    cid = "n17-d2-m2-f2p2"
    c = hc.CASES[cid]
    r = hc.reference(cid)
    acq, X = make_acq(cid, ref_point=r["Y"].reshape(-1, c["m"]).max(0).values + 1.0)
    val, grad = acq.value_and_grad_host(X)
    assert bool((val == -c["current"] / hc.case_cost(c)).all())
    assert float(grad.abs().max()) == 0.0


def _special(cid, edit):
    """The case's first restart with ``edit(X)`` applied: device (value, gradient) and the oracle's with bounds."""
    c = hc.CASES[cid]
    state, z, X, ref = hc.problem(cid)
    X = X[:1].clone()
    edit(X, state)
    acq, _ = make_acq(cid)
    cur, cost = (0.0 if c["current"] is None else c["current"]), hc.case_cost(c)
    out = []
    for rev in (False, True):
        Xr = X.clone().requires_grad_(True)
        a, scale = ho.acquisition(ho.models_of(state, rev), Xr, z, hc.mask_bits(c["mask"]), c["Nf"], c["Np"], ref, cur,
                                  cost)
        (g,) = torch.autograd.grad(a.sum(), Xr)
        out.append((a.detach(), g, scale))
    (a, g, scale), (a2, g2, _) = out
    vtol = 1e-6 * scale + 4.0 * (a - a2).abs().max()
    gtol = 1e-6 * g.abs().max() + 4.0 * (g - g2).abs().max()
    val, grad = acq.value_and_grad_host(X)
    return val, grad, a, g, vtol, gtol


def test_exact_duplicate_rows():
    """Two equal points in one fantasy: the value is within its bound, and the gradient summed over the duplicates
    equals the oracle's (which of the two takes it is the convention: the lower index)."""
    def edit(X, state):
        X[0, 2] = X[0, 1]
    val, grad, a, g, vtol, gtol = _special("n17-d2-m2-f2p2", edit)
    assert bool(((val - a).abs() <= vtol).all())
    both, both_ref = grad.clone(), g.clone()
    both[0, 1] += both[0, 2]; both[0, 2] = 0.0
    both_ref[0, 1] += both_ref[0, 2]; both_ref[0, 2] = 0.0
    assert float((both - both_ref).abs().max()) <= float(gtol)
    assert float(grad[0, 2].abs().max()) == 0.0 or float(grad[0, 1].abs().max()) > 0.0


@pytest.mark.parametrize("kind", ["fantasy-on-candidate", "candidate-on-training-point"])
def test_coincident_points(kind):
    """Matern-3/2 and RBF outputs (the Matern-1/2 gradient at a coincident point is the exception of DESIGN.md 4.5)."""
    def edit(X, state):
        if kind == "fantasy-on-candidate":
            X[0, 3] = X[0, 0]
        else:
            X[0, 0] = state.models[1].train_x[4]
    val, grad, a, g, vtol, gtol = _special("n17-d2-m2-f2p2", edit)
    assert bool(((val - a).abs() <= vtol).all())
    assert float((grad - g).abs().max()) <= float(gtol)


# ---- the hypervolume stage alone -------------------------------------------------------------------------------

def _hv_sets(kind, Np, m, g):
    S = 6
    if kind == "random":
        return torch.rand(S, Np, m, generator=g, dtype=torch.double)
    if kind == "staircase":  # mutually non-dominated: objective 0 ascending, the others descending
        t = (torch.arange(Np, dtype=torch.double) + 1.0) / (Np + 1.0)
        base = torch.stack([t] + [1.0 - t ** (i + 1) for i in range(m - 1)], dim=-1)
        return base[None] * (0.5 + 0.5 * torch.rand(S, 1, 1, generator=g, dtype=torch.double))
    if kind == "all-dominated":  # point Np - 1 dominates every other
        Y = 0.8 * torch.rand(S, Np, m, generator=g, dtype=torch.double)
        Y[:, -1] = 0.9
        return Y
    # tied: coordinates on a grid of four levels, so equal coordinates, equal points and points on ref abound
    return torch.randint(0, 4, (S, Np, m), generator=g).double() / 4.0


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("Np", [1, 2, 9, 32])
@pytest.mark.parametrize("kind", ["random", "staircase", "all-dominated", "tied"])
def test_hypervolume_stage_alone(kind, Np, m):
    from dkg_amd.hvkg import hypervolume_device
    from dkg_amd.metrics import hypervolume

    g = torch.Generator().manual_seed(100 * Np + m)
    Y = _hv_sets(kind, Np, m, g)
    ref = torch.full((m,), 0.25 if kind == "tied" else 0.05, dtype=torch.double)
    hv, dhv = hypervolume_device(Y.to(DEV), ref, grad=True)
    hv, dhv = hv.cpu(), dhv.cpu()
    for s in range(Y.shape[0]):
        want = hypervolume(Y[s].numpy(), ref.numpy())
        span = (Y[s].max(0).values - ref).clamp_min(0.0)
        assert abs(float(hv[s]) - want) <= 64 * EPS * float(span.prod()), (kind, Np, m, s)
    if kind in ("random", "staircase"):  # the kink condition holds: the gradient against the oracle's
        Yr = Y.clone().requires_grad_(True)
        (gref,) = torch.autograd.grad(ho.hypervolume(Yr, ref).sum(), Yr)
        assert ho.kink_margin(Y[:, None], ref) >= hc.KINK_MIN
        span = (Y.max(1).values - ref).clamp_min(0.0)                        # [S, m]
        others = torch.stack([span[:, [j for j in range(m) if j != i]].prod(-1) for i in range(m)], dim=-1)
        assert bool(((dhv - gref).abs() <= 64 * EPS * others[:, None, :]).all())
    else:  # a point that adds nothing gets exactly 0
        dominated, below = _classify(Y[:, None], ref)
        assert float(dhv[(dominated | below)[:, 0]].abs().max() if bool((dominated | below).any()) else 0.0) == 0.0


# ---- bits ------------------------------------------------------------------------------------------------------

BITS_CASE = "n256-d2-m2-f9p8"


def test_two_calls_and_both_routes_give_the_same_bits():
    acq, X = make_acq(BITS_CASE)
    v1, g1 = acq.value_and_grad_host(X)
    v2, g2 = acq.value_and_grad_host(X)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    Xd = X.to(DEV).requires_grad_(True)
    vd = acq(Xd)
    (gd,) = torch.autograd.grad(vd.sum(), Xd)
    assert torch.equal(vd.detach().cpu(), v1) and torch.equal(gd.cpu(), g1)
    Xh = X.clone().requires_grad_(True)
    vh = acq(Xh)
    (gh,) = torch.autograd.grad(vh.sum(), Xh)
    assert torch.equal(vh.detach(), v1) and torch.equal(gh, g1)
    with torch.no_grad():
        assert torch.equal(acq(X), v1) and torch.equal(acq(X.to(DEV)).cpu(), v1)


def test_a_restart_has_the_same_bits_alone_and_a_grown_plan_keeps_them():
    acq, X = make_acq(BITS_CASE)  # B = 17: the plan holds 32 restarts
    v, g = acq.value_and_grad_host(X)
    fresh, _ = make_acq(BITS_CASE)
    for b in range(X.shape[0]):   # the fresh acquisition's plan holds 16
        vb, gb = fresh.value_and_grad_host(X[b:b + 1])
        assert torch.equal(vb, v[b:b + 1]) and torch.equal(gb, g[b:b + 1])
    assert fresh._plans[hc.mask_bits(hc.CASES[BITS_CASE]["mask"])].max_B == 16
    v16, g16 = fresh.value_and_grad_host(X[:16])
    v17, g17 = fresh.value_and_grad_host(X)  # grows the plan to 32
    assert fresh._plans[hc.mask_bits(hc.CASES[BITS_CASE]["mask"])].max_B == 32
    assert torch.equal(v16, v[:16]) and torch.equal(g16, g[:16])
    assert torch.equal(v17, v) and torch.equal(g17, g)
    assert torch.equal(fresh.value_and_grad_host(X[:16])[1], g[:16])


def test_the_value_function_is_the_one_shot_with_one_zero_fantasy():
    from dkg_amd.hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient

    cid = "n130-d6-m3-f3p4"
    state, _, X, ref = hc.problem(cid)
    q = 12
    pts = X[:, 1:1 + q]
    vf = PosteriorMeanHypervolume(state, ref, device=DEV)
    v, g = vf.value_and_grad_host(pts)
    one = qHypervolumeKnowledgeGradient(state, ref, num_fantasies=1, num_pareto=q,
                                        base_samples=torch.zeros(1, 3), device=DEV)
    v1, g1 = one.value_and_grad_host(torch.cat([X[:, :1], pts], dim=1))
    assert torch.equal(v, v1) and torch.equal(g, g1[:, 1:])
    assert float(g1[:, 0].abs().max()) == 0.0  # z = 0: the candidate does not matter
    # and against the oracle
    Xr = pts.clone().requires_grad_(True)
    a, scale = ho.value_function(ho.models_of(state), Xr, ref)
    (gr,) = torch.autograd.grad(a.sum(), Xr)
    assert bool(((v - a.detach()).abs() <= 1e-6 * scale + 1e-13).all())
    assert float((g - gr).abs().max()) <= 1e-6 * float(gr.abs().max()) + 1e-13


def test_changing_the_mask_and_back_restores_the_bits():
    cid = "n130-d6-m3-f3p4"
    acq, X = make_acq(cid)
    v, g = acq.value_and_grad_host(X)
    first = acq.X_evaluation_mask
    one = torch.zeros(1, 3, dtype=torch.bool)
    one[0, 1] = True
    acq.X_evaluation_mask = one
    v1, g1 = acq.value_and_grad_host(X)
    assert not torch.equal(v1, v)
    c = hc.CASES[cid]
    state, z, _, ref = hc.problem(cid)
    Xr = X.clone().requires_grad_(True)
    a, scale = ho.acquisition(ho.models_of(state), Xr, z, 2, c["Nf"], c["Np"], ref, c["current"], c["costs"][1])
    assert bool(((v1 - a.detach()).abs() <= 1e-6 * scale + 1e-13).all())
    acq.X_evaluation_mask = first
    v2, g2 = acq.value_and_grad_host(X)
    assert torch.equal(v2, v) and torch.equal(g2, g)


# ---- limits ----------------------------------------------------------------------------------------------------

def test_limits_are_refused():
    from dkg_amd import _lib
    from dkg_amd.errors import BotorchTensorDimensionError, UnsupportedError
    from dkg_amd.hvkg import HvkgPlan, PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient

    cid = "n17-d2-m2-f2p2"
    state, z, X, ref = hc.problem(cid)
    acq, _ = make_acq(cid)
    acq._refresh()
    structs = acq._state.structs
    lib = _lib.load()
    assert lib.dkg_hvkg_workspace(2, 2, 65, 2, 16) == 0 and lib.dkg_hvkg_workspace(2, 2, 2, 33, 16) == 0
    assert lib.dkg_hvkg_workspace(4, 2, 2, 2, 16) == 0 and lib.dkg_hvkg_workspace(2, 2, 2, 2, 4097) == 0
    for Nf, Np, maxB in ((65, 2, 16), (2, 33, 16), (2, 2, 4097)):
        with pytest.raises(UnsupportedError):
            HvkgPlan(structs, 2, 2, ref.tolist(), Nf, Np, torch.zeros(Nf, 2), 1, 0.0, 1.0, maxB, torch.device(DEV))
    four = (_lib.DkgOutput * 4)(*[structs[i % 2] for i in range(4)])
    with pytest.raises(UnsupportedError, match="m = 2 and m = 3"):
        HvkgPlan(four, 4, 2, [0.0] * 4, 2, 2, torch.zeros(2, 4), 1, 0.0, 1.0, 16, torch.device(DEV))
    plan = acq._plan_for(1, X.shape[1])
    with pytest.raises(BotorchTensorDimensionError, match="max_B"):
        plan.forward(torch.zeros(plan.max_B + 1, X.shape[1], 2, dtype=torch.double, device=DEV))
    # the class: at construction, and at evaluation for the batch
    with pytest.raises(UnsupportedError):
        qHypervolumeKnowledgeGradient(state, ref, num_fantasies=65, num_pareto=2, device=DEV)
    with pytest.raises(UnsupportedError):
        qHypervolumeKnowledgeGradient(state, ref, num_fantasies=2, num_pareto=33, device=DEV)
    from helpers import grad_case
    four_state = grad_case(4, 2, (9,), ("M52",), 4, 2, 1, 5)[0]
    with pytest.raises(UnsupportedError):
        qHypervolumeKnowledgeGradient(four_state, [0.0] * 4, device=DEV)
    with pytest.raises(UnsupportedError):
        PosteriorMeanHypervolume(four_state, [0.0] * 4, device=DEV)
    small, _ = make_acq("n5-d1-m2-f1p1")
    with pytest.raises(UnsupportedError, match="4096"):
        small.value_and_grad_host(torch.zeros(4097, 2, 1))
    with pytest.raises(UnsupportedError):
        PosteriorMeanHypervolume(state, ref, device=DEV)(torch.zeros(1, 33, 2))


# ---- optimisation ----------------------------------------------------------------------------------------------

def test_optimize_acqf_on_the_value_function():
    """q = 2, 2 restarts, 8 raw samples: every point L-BFGS-B evaluates on the device is replayed on the
    restatement under the two bounds; the returned set is the best recorded one."""
    from dkg_amd.hvkg import PosteriorMeanHypervolume
    from dkg_amd.optim import _get_standard_bounds, optimize_acqf

    state, ref, _, _ = hc.opt_problem()
    records = []
    acq = hc.Recorder(PosteriorMeanHypervolume(state, ref, device=DEV), records, "value_function")
    x, v = optimize_acqf(acq, _get_standard_bounds(2), q=2, num_restarts=2, raw_samples=8,
                         options={"seed": hc.OPT["seed"], "batch_limit": 2})
    total, skipped, wv, wg = hc.replay(records)
    print(f"value function: {total} evaluated restarts, {skipped} skipped, worst err/bound {wv:.3g} (value) {wg:.3g} (gradient)")
    assert skipped <= hc.SKIP_CAP * total and any(r["grad"] is not None for r in records)
    last = records[-1]  # the final evaluation of the candidates
    best = int(last["val"].argmax())
    assert x.shape == (2, 2) and torch.equal(x, last["X"][best]) and float(v) == float(last["val"][best])


def _device_spec(records, z):
    from dkg_amd.hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient
    from dkg_amd.optim import HvkgOptimisationSpec

    def factory(kind, model, ref_point, **kw):
        if kind == "value_function":
            return hc.Recorder(PosteriorMeanHypervolume(model, ref_point, device=DEV), records, kind)
        kw.pop("seed")
        return hc.Recorder(qHypervolumeKnowledgeGradient(model, ref_point, base_samples=z, device=DEV, **kw), records,
                           kind)

    return HvkgOptimisationSpec(acq_factory=factory, device=DEV, **hc.OPT)


def _finals(records, bits):
    """The final evaluation of the one-shot candidates under a mask: its last value-only record."""
    return [r for r in records if r["tag"] == "hvkg" and r["bits"] == bits and r["value_only"]][-1]


def test_spec_single_objective_on_the_device():
    state, ref, z, _ = hc.opt_problem()
    records = []
    x, best_i, v = _device_spec(records, z).optimize_for_single_objective(state, list(hc.OPT_COSTS), 2, hv_refpoint=ref)
    vf = [r for r in records if r["tag"] == "value_function"]
    current = float(vf[-1]["val"].max())  # the current optimum: the best of the value function's candidates
    total, skipped, wv, wg = hc.replay(records, costs=hc.OPT_COSTS, current=current)
    print(f"single objective: {total} evaluated restarts, {skipped} skipped, worst err/bound {wv:.3g} (value) "
          f"{wg:.3g} (gradient)")
    assert skipped <= hc.SKIP_CAP * total
    finals = [_finals(records, 1 << i) for i in range(2)]
    bests = [float(f["val"].max()) for f in finals]
    want_i = max(range(2), key=lambda i: bests[i])
    f = finals[want_i]
    assert best_i == want_i and float(v) == bests[want_i]
    assert torch.equal(x, f["X"][int(f["val"].argmax())][:1])


def test_spec_full_evaluation_on_the_device():
    state, ref, z, _ = hc.opt_problem()
    records = []
    x, v = _device_spec(records, z).optimize_for_full_evaluation(state, 2, hv_refpoint=ref)
    vf = [r for r in records if r["tag"] == "value_function"]
    total, skipped, wv, wg = hc.replay(records, current=float(vf[-1]["val"].max()))
    print(f"full evaluation: {total} evaluated restarts, {skipped} skipped, worst err/bound {wv:.3g} (value) "
          f"{wg:.3g} (gradient)")
    assert skipped <= hc.SKIP_CAP * total
    f = _finals(records, None)
    assert float(v) == float(f["val"].max()) and torch.equal(x, f["X"][int(f["val"].argmax())][:1])
