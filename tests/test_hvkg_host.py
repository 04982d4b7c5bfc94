"""Host-side tests of the hypervolume knowledge gradient (no GPU): the identities the restatement of
tests/hvkg_oracle.py rests on, the C ABI's refusals, the class surface of dkg_amd/hvkg.py and the optimisation
layer of dkg_amd/optim.py on CPU callables."""

import ctypes
import logging

import pytest
import torch

import hvkg_cases as hc
import hvkg_oracle as ho

EPS = 2.0 ** -52


# ---- the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", list(hc.CASES))
def test_fantasy_mean_is_append_and_refactorise(cid):
    """The closed form mu(x') + z c(x', x) / sigma~(x) against the model with the fantasised row appended and
    refactorised, restart 0, every observed output, the first and the last fantasy."""
    c = hc.CASES[cid]
    state, z, X, _ = hc.problem(cid)
    models = ho.models_of(state)
    Y = hc.reference(cid)["Y"]
    worst = 0.0
    for i in c["mask"]:
        for f in sorted({0, c["Nf"] - 1}):
            rows = X[0, 1 + f * c["Np"]: 1 + (f + 1) * c["Np"]]
            want = ho.fantasy_mean_by_refactorising(models[i], X[0, 0], rows, float(z[f, i]))
            worst = max(worst, float((Y[0, f, :, i] - want).abs().max()))
    print(f"{cid}: closed form against refactorising {worst:.3g}")
    assert worst <= 1e-10


def _sets(kind, g, Np, m):
    if kind == "random":
        return torch.rand(Np, m, generator=g, dtype=torch.double)
    if kind == "tied":
        return torch.randint(0, 4, (Np, m), generator=g).double() / 4.0
    if kind == "dominated":
        Y = 0.8 * torch.rand(Np, m, generator=g, dtype=torch.double)
        Y[Np // 2] = 0.9
        return Y
    Y = torch.rand(Np, m, generator=g, dtype=torch.double)  # below-ref: half the points under ref in one objective
    Y[::2, 0] = 0.01
    return Y


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("kind", ["random", "tied", "dominated", "below-ref"])
def test_oracle_hypervolume_is_the_metrics_hypervolume(kind, m):
    from dkg_amd.metrics import hypervolume

    g = torch.Generator().manual_seed(7 + m)
    ref = torch.full((m,), 0.25 if kind == "tied" else 0.05, dtype=torch.double)
    for Np in (1, 2, 9, 32):
        Y = _sets(kind, g, Np, m)
        got = float(ho.hypervolume(Y, ref))
        want = hypervolume(Y.numpy(), ref.numpy())
        assert abs(got - want) <= 64 * EPS * float((Y.max(0).values - ref).clamp_min(0).prod()), (kind, m, Np)


def test_oracle_hypervolume_conventions():
    ref = [0.0, 0.0]
    Y = torch.tensor([[3.0, 1.0], [3.0, 1.0], [1.0, 0.5], [2.0, 0.0], [1.0, 3.0]], requires_grad=True)
    hv = ho.hypervolume(Y, ref)
    (g,) = torch.autograd.grad(hv, Y)
    assert float(hv.detach()) == 3.0 * 1.0 + 1.0 * 2.0
    assert g[0].tolist() == [1.0, 2.0]          # the lower index of the duplicates takes the derivative
    assert g[1].tolist() == [0.0, 0.0]
    assert g[2].tolist() == [0.0, 0.0]          # strictly dominated
    assert g[3].tolist() == [0.0, 0.0]          # on ref in one objective: not strictly above
    assert g[4].tolist() == [2.0, 1.0]


@pytest.mark.parametrize("cid", ["n17-d2-m2-f2p2", "n130-d6-m3-f3p4"])
def test_oracle_gradient_agrees_with_central_differences(cid):
    c = hc.CASES[cid]
    state, z, X, ref = hc.problem(cid)
    r = hc.reference(cid)
    assert r["kink"] >= hc.KINK_MIN
    models = ho.models_of(state)
    cur, cost = (0.0 if c["current"] is None else c["current"]), hc.case_cost(c)
    X0 = X[:1]
    g = torch.Generator().manual_seed(3)
    h = 1e-6
    for _ in range(3):
        direction = torch.randn(X0.shape, generator=g, dtype=torch.double)
        with torch.no_grad():
            up = ho.acquisition(models, X0 + h * direction, z, hc.mask_bits(c["mask"]), c["Nf"], c["Np"], ref, cur, cost)[0]
            dn = ho.acquisition(models, X0 - h * direction, z, hc.mask_bits(c["mask"]), c["Nf"], c["Np"], ref, cur, cost)[0]
        fd = float((up - dn) / (2 * h))
        an = float((r["grad"][:1] * direction).sum())
        assert abs(fd - an) <= 1e-6 * float(r["grad"][:1].abs().max()) * float(direction.abs().sum()) + 1e-8


# ---- the C ABI -------------------------------------------------------------------------------------------------

def _fake_outputs(m, n=5):
    from dkg_amd import _lib

    outs = (_lib.DkgOutput * m)()
    for o in outs:
        o.n, o.kernel, o.outputscale, o.noise, o.y_std = n, 2, 1.0, 1e-2, 1.0
        o.inv_lengthscale = o.train_x = o.alpha = o.root_frag = 64  # never followed: the checks come first
    return outs


def test_abi_version_is_still_9():
    from dkg_amd import _lib

    assert _lib.load().dkg_abi_version() == 9 == _lib.ABI_VERSION


def test_argument_refusals_come_before_any_device_work():
    from dkg_amd import _lib

    lib = _lib.load()
    ARG, UNS, WS = _lib.DKG_ERR_ARG, _lib.DKG_ERR_UNSUPPORTED, _lib.DKG_ERR_WORKSPACE
    host = ctypes.create_string_buffer(lib.dkg_hvkg_plan_bytes())
    ref = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    z = (ctypes.c_double * (65 * 4))()
    fake_ws = 256

    def init(outs, m=2, d=2, ref_=ref, Nf=2, Np=2, z_=z, mask=1, cur=0.0, cost=1.0, max_B=16, ws=fake_ws, bytes_=1 << 40,
             host_=host):
        return lib.dkg_hvkg_init(outs, m, d, ref_, Nf, Np, z_, mask, cur, cost, max_B, ws, bytes_, host_, None)

    outs = _fake_outputs(4)
    assert init(None) == ARG
    assert init(outs, ref_=None) == ARG and init(outs, z_=None) == ARG and init(outs, ws=None) == ARG
    assert init(outs, host_=None) == ARG
    assert init(outs, Nf=0) == ARG and init(outs, Np=0) == ARG and init(outs, d=0) == ARG and init(outs, max_B=0) == ARG
    assert init(outs, m=0) == ARG
    for m in (1, 4):
        assert init(outs, m=m) == UNS
        assert b"m = 2 and m = 3" in lib.dkg_last_error()
    assert init(outs, Nf=65) == UNS and init(outs, Np=33) == UNS and init(outs, max_B=4097) == UNS
    assert init(outs, d=17) == UNS
    assert init(outs, mask=4) == ARG and init(outs, m=3, mask=8) == ARG       # out of range
    assert init(outs, mask=0, Nf=2) == ARG                                       # the value function takes Nf = 1
    assert init(outs, cost=0.0) == ARG and init(outs, cost=-1.0) == ARG and init(outs, cost=float("nan")) == ARG
    assert init(_fake_outputs(2, n=0)) == ARG and init(_fake_outputs(2, n=1025)) == UNS
    assert init(outs, bytes_=16) == WS
    for args in ((2, 2, 65, 2, 16), (2, 2, 2, 33, 16), (4, 2, 2, 2, 16), (1, 2, 2, 2, 16), (2, 2, 2, 2, 4097),
                 (2, 0, 2, 2, 16)):
        assert lib.dkg_hvkg_workspace(*args) == 0
    assert lib.dkg_hvkg_workspace(2, 2, 32, 10, 16) > 0
    # forward: NULL pointers and a plan that was never initialised
    assert lib.dkg_hvkg_forward(None, 64, 1, 64, None, None, None) == ARG
    blank = ctypes.create_string_buffer(lib.dkg_hvkg_plan_bytes())
    assert lib.dkg_hvkg_forward(blank, 64, 1, 64, None, None, None) == ARG
    assert b"not initialised" in lib.dkg_last_error()
    assert lib.dkg_hvkg_forward(blank, None, 1, 64, None, None, None) == ARG
    # the hypervolume stage alone
    assert lib.dkg_hypervolume(None, 1, 2, 2, ref, 64, None, None) == ARG
    assert lib.dkg_hypervolume(64, 0, 2, 2, ref, 64, None, None) == ARG
    assert lib.dkg_hypervolume(64, 1, 0, 2, ref, 64, None, None) == ARG
    assert lib.dkg_hypervolume(64, 1, 2, 4, ref, 64, None, None) == UNS
    assert lib.dkg_hypervolume(64, 1, 2, 1, ref, 64, None, None) == UNS
    assert lib.dkg_hypervolume(64, 1, 33, 2, ref, 64, None, None) == UNS


# ---- the classes -----------------------------------------------------------------------------------------------

def _small_state():
    return hc.build_state(hc.CASES["n17-d2-m2-f2p2"])


def test_class_validation_and_shapes():
    from dkg_amd import PosteriorMeanHypervolume, UnsupportedError, qHypervolumeKnowledgeGradient

    state = _small_state()
    ref = [0.0, 0.0]
    dev = "cuda:0"  # nothing touches the device before the first evaluation
    for name in ("sampler", "objective", "inner_sampler", "X_pending"):
        with pytest.raises(UnsupportedError, match=name):
            qHypervolumeKnowledgeGradient(state, ref, device=dev, **{name: object()})
    with pytest.raises(UnsupportedError, match="use_posterior_mean"):
        qHypervolumeKnowledgeGradient(state, ref, use_posterior_mean=False, device=dev)
    with pytest.raises(ValueError, match="Cost-aware HV-KG requires current_value to be specified."):
        qHypervolumeKnowledgeGradient(state, ref, cost_aware_utility=[1.0, 2.0], device=dev)
    with pytest.raises(ValueError, match="reference point"):
        qHypervolumeKnowledgeGradient(state, [0.0, 0.0, 0.0], device=dev)
    with pytest.raises(ValueError, match="base_samples"):
        qHypervolumeKnowledgeGradient(state, ref, num_fantasies=4, base_samples=torch.zeros(3, 2), device=dev)
    with pytest.raises(UnsupportedError, match="ROCm"):
        qHypervolumeKnowledgeGradient(state, ref, device="cpu")
    acq = qHypervolumeKnowledgeGradient(state, ref, num_fantasies=3, num_pareto=4, current_value=0.5,
                                        cost_aware_utility=[1.5, 2.5], seed=5, device=dev)
    assert acq.get_augmented_q_batch_size(1) == 13 and acq.num_pseudo_points == 12
    X = torch.rand(7, 13, 2)
    assert acq.extract_candidates(X).shape == (7, 1, 2) and torch.equal(acq.extract_candidates(X), X[:, :1])
    assert acq.extract_candidates(X[0]).shape == (1, 2)
    # the mask: [1, m] booleans, settable, None = all outputs; the cost follows it
    assert acq.X_evaluation_mask is None and acq.cost == 4.0
    mask = torch.tensor([[False, True]])
    acq.X_evaluation_mask = mask
    assert acq.X_evaluation_mask is mask and acq.cost == 2.5 and acq._mask_bits == 2
    for bad in (torch.tensor([True, False]), torch.ones(2, 2, dtype=torch.bool), torch.ones(1, 3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="Expected X_evaluation_mask of shape"):
            acq.X_evaluation_mask = bad
    with pytest.raises(ValueError, match="at least one output"):
        acq.X_evaluation_mask = torch.zeros(1, 2, dtype=torch.bool)
    # the shape of X is checked before any device work
    with pytest.raises(ValueError, match=r"n_f\*num_pareto \(12\) must be less than the q-batch dimension of X \(12\)"):
        acq(torch.rand(2, 12, 2))
    with pytest.raises(UnsupportedError, match="only q = 1"):
        acq(torch.rand(2, 14, 2))
    with pytest.raises(RuntimeError, match="last dimension"):
        acq(torch.rand(2, 13, 3))
    with pytest.raises(UnsupportedError, match="q=33"):
        PosteriorMeanHypervolume(state, ref, device=dev)(torch.rand(1, 33, 2))


def test_default_base_samples_are_seeded_and_leave_the_global_generator_alone():
    from dkg_amd import qHypervolumeKnowledgeGradient

    state = _small_state()
    before = torch.random.get_rng_state()
    a = qHypervolumeKnowledgeGradient(state, [0.0, 0.0], num_fantasies=16, seed=11, device="cuda:0").base_samples
    b = qHypervolumeKnowledgeGradient(state, [0.0, 0.0], num_fantasies=16, seed=11, device="cuda:0").base_samples
    c = qHypervolumeKnowledgeGradient(state, [0.0, 0.0], num_fantasies=16, seed=12, device="cuda:0").base_samples
    qHypervolumeKnowledgeGradient(state, [0.0, 0.0], num_fantasies=16, device="cuda:0")
    assert torch.equal(torch.random.get_rng_state(), before)
    assert a.shape == (16, 2) and torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[:, 0], a[:, 1])            # one engine per output
    assert bool(torch.isfinite(a).all()) and abs(float(a.mean())) < 0.2 and 0.7 < float(a.std()) < 1.3


# ---- the optimisation layer ------------------------------------------------------------------------------------

def test_optimize_acqf_takes_a_q_batch():
    from dkg_amd.optim import optimize_acqf

    target = torch.tensor([[0.2, 0.7], [0.9, 0.1], [0.5, 0.5]])

    def acq(X):  # [*batch, 3, 2] -> [*batch]
        return -((X - target) ** 2).sum(dim=(-1, -2))

    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]])
    x, v = optimize_acqf(acq, bounds, q=3, num_restarts=2, raw_samples=8, options={"seed": 3, "batch_limit": 2})
    assert x.shape == (3, 2) and float((x - target).abs().max()) < 1e-5 and float(v) > -1e-9
    xs, vs = optimize_acqf(acq, bounds, q=3, num_restarts=2, raw_samples=8, options={"seed": 3}, return_best_only=False)
    assert xs.shape == (2, 3, 2) and vs.shape == (2,)
    with pytest.raises(ValueError):
        optimize_acqf(acq, bounds, q=0, num_restarts=2, raw_samples=8)


class _StubHvkg:
    """value = peak_t - |x - centre_t|^2 for the masked objective t (all outputs: t = m), whatever the fantasy rows."""

    def __init__(self, peaks, centres, log):
        self.peaks, self.centres, self.log = peaks, centres, log
        self._mask = None
        self.R = 4

    @property
    def X_evaluation_mask(self):
        return self._mask

    @X_evaluation_mask.setter
    def X_evaluation_mask(self, mask):
        self.log.append(None if mask is None else mask.clone())
        self._mask = mask

    def extract_candidates(self, X):
        return X[..., : -self.R, :]

    def __call__(self, X):
        t = len(self.peaks) - 1 if self._mask is None else int(self._mask.reshape(-1).long().argmax())
        return self.peaks[t] - ((X[..., 0, :] - self.centres[t]) ** 2).sum(-1)


def _stub_spec(peaks, log, made):
    from dkg_amd.optim import HvkgOptimisationSpec

    centres = torch.tensor([[0.2, 0.3], [0.8, 0.6], [0.5, 0.5]])

    def factory(kind, model, ref_point, **kw):
        made.append((kind, kw))
        if kind == "value_function":
            return lambda X: -((X - 0.5) ** 2).sum(dim=(-1, -2)) + 1.25
        return _StubHvkg(peaks, centres, log)

    spec = HvkgOptimisationSpec(num_pareto=2, num_fantasies=2, num_restarts=2, raw_samples=4, curr_opt_num_restarts=2,
                                curr_opt_raw_samples=8, batch_limit=2, max_iter=50, seed=1, acq_factory=factory)
    return spec, centres


def test_spec_takes_the_argmax_and_sets_the_mask_per_objective(caplog):
    state = _small_state()
    log, made = [], []
    # objective 1 has the larger value; under _choose_best_objective's value / cost rule objective 0 would win
    spec, centres = _stub_spec([0.5, 0.9, 0.7], log, made)
    x, best_i, value = spec.optimize_for_single_objective(state, [1.0, 10.0], 2, hv_refpoint=torch.zeros(2))
    assert best_i == 1 and x.shape == (1, 2) and float((x[0] - centres[1]).abs().max()) < 1e-5
    assert abs(float(value) - 0.9) < 1e-9
    assert [mk.tolist() for mk in log] == [[[True, False]], [[False, True]]]
    kinds = [k for k, _ in made]
    assert kinds == ["value_function", "hvkg"]
    kw = made[1][1]
    assert kw["num_fantasies"] == 2 and kw["num_pareto"] == 2 and kw["cost_aware_utility"] == [1.0, 10.0]
    assert abs(float(kw["current_value"]) - 1.25) < 1e-9     # the value function's optimum
    # full evaluation: no mask is set and no cost-aware utility is passed
    log.clear(); made.clear()
    x, value = spec.optimize_for_full_evaluation(state, 2, hv_refpoint=torch.zeros(2))
    assert log == [] and made[1][1]["cost_aware_utility"] is None
    assert float((x[0] - centres[2]).abs().max()) < 1e-5 and abs(float(value) - 0.7) < 1e-9
    # hv_refpoint is a required keyword of both entry points
    with pytest.raises(TypeError, match="hv_refpoint"):
        spec.optimize_for_single_objective(state, [1.0, 1.0], 2)
    with pytest.raises(TypeError, match="hv_refpoint"):
        spec.optimize_for_full_evaluation(state, 2)
    # the reference's warnings
    spec, _ = _stub_spec([-0.5, 0.0, -0.1], [], [])
    with caplog.at_level(logging.WARNING, logger="dkg_amd.optim"):
        spec.optimize_for_single_objective(state, [1.0, 1.0], 2, hv_refpoint=torch.zeros(2))
        spec.optimize_for_full_evaluation(state, 2, hv_refpoint=torch.zeros(2))
    text = caplog.text
    assert "not strictly positive (after clipping to be at least zero): obj_index=0" in text
    assert "obj_index=1" in text and "Optimal acquisition function value is negative: acq_value=" in text


def test_spec_runs_on_the_cpu_restatement_and_stays_off_the_kinks():
    """Both entry points end to end on the CPU acquisitions of tests/hvkg_oracle.py, on the problem and with the
    sizes and seeds of the GPU optimisation tests (hvkg_cases.OPT): at most one in ten of the evaluated points
    fails the kink condition, so the GPU tests' replay compares nearly all of them."""
    from dkg_amd.optim import HvkgOptimisationSpec

    state, ref, z, _ = hc.opt_problem()
    records = []

    def factory(kind, model, ref_point, **kw):
        if kind == "value_function":
            return hc.Recorder(ho.OracleValueFunction(model, ref_point), records, kind)
        return hc.Recorder(ho.OracleHvkg(model, ref_point, kw["num_fantasies"], kw["num_pareto"], z,
                                         kw["current_value"], kw["cost_aware_utility"]), records, kind)

    spec = HvkgOptimisationSpec(acq_factory=factory, **hc.OPT)
    x, i, v = spec.optimize_for_single_objective(state, list(hc.OPT_COSTS), 2, hv_refpoint=ref)
    assert x.shape == (1, 2) and i in (0, 1) and bool(torch.isfinite(v)) and bool(((x >= 0) & (x <= 1)).all())
    x, v = spec.optimize_for_full_evaluation(state, 2, hv_refpoint=ref)
    assert x.shape == (1, 2) and bool(torch.isfinite(v)) and bool(((x >= 0) & (x <= 1)).all())
    total, skipped, _, _ = hc.replay(records, check=False)
    print(f"{total} evaluated restarts, {skipped} fail the kink condition")
    assert total > 0 and skipped <= hc.SKIP_CAP * total
