"""The marginal log-likelihood and its gradient on the device (dkg_mll_value_grad; dkg_amd.fit's device route)
against the difference-form fp64 yardstick of tests/mll_cases.py, and the MAP fit through it.

Tolerances (tests/mll_cases.py): gradient |dg|_inf / max|g| <= TOL = 1e-8 (100 x the yardstick's own spread of
3.3e-10, capped at 1e-8), value relative error <= VALUE_TOL = 3.1e-10.

Fit-objective gap: on the CPU, fit_map as shipped and fit_map with the difference-form kernel (fit.matern replaced
by mll_cases.kernel_torch) end, on test_fit's _data(n=150, seed=3), at objectives 6.2e-13 apart (both re-evaluated
by the CPU neg_mll: 0.38439356477243886 and 0.3843935647718223, 25 iterations each).  The device fit is allowed
4 x that gap, 2.5e-12, to the CPU fit's objective.

Measured on an MI355X: worst gradient error 1.6e-10 of max|g| (n = 130, Matern-5/2, d = 1, noise 1e-4), worst value
error 1.2e-12 relative (n = 1000); the first objective evaluation of the two routes agrees to 5.4e-13 of max|g| and
5.9e-13 relative in the loss; the device fit ends 7.3e-13 from the CPU fit's objective, 25 iterations both."""

import functools

import numpy as np
import pytest
import torch

import mll_cases as mc
from dkg_amd import fit
from dkg_amd.bo_smoke import GPProblem, reference_model_config, run_smoke
from dkg_amd.fit import DeviceMll, fit_map, mll_value_and_grad, neg_mll
from helpers import load_golden
from test_fit import _data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CPU_FIT_GAP = 6.2e-13
KEYS = ("means", "length_scales", "output_scales", "noises")


@functools.lru_cache(maxsize=None)
def device(name):
    ds = mc.data(name)
    return mll_value_and_grad([o["X"] for o in ds], [o["y"] for o in ds], mc.hyper_of(name), mc.config_of(name), DEV,
                              return_jitter=True)


def evaluator(name, outputs=None):
    ds = mc.data(name)
    ds = ds if outputs is None else [ds[i] for i in outputs]
    ev = DeviceMll([o["X"] for o in ds], [o["y"] for o in ds], [o["nu"] for o in ds], DEV)
    args = ([o["mean"] for o in ds], [o["ls"].tolist() for o in ds], [o["os"] for o in ds], [o["noise"] for o in ds])
    return ev, args


@pytest.mark.parametrize("name", list(mc.CASES))
def test_value_and_gradient_match_the_yardstick(name):
    val, grad, jit = device(name)
    rv, rg = mc.reference(name)
    assert list(jit) == [mc.CASES[name][1]] * len(rg)  # the jitter the factorisation needed
    for i in range(len(rg)):
        d = len(rg[i]) - 3
        assert grad.shape[1] == d + 3
        eg = np.abs(grad[i] - rg[i]).max() / np.abs(rg[i]).max()
        ev = abs(val[i] - rv[i]) / abs(rv[i])
        print(f"{name} output {i}: gradient error {eg:.3e} of max|g|, value error {ev:.3e} relative")
        assert eg <= mc.TOL, (name, i, eg, grad[i], rg[i])
        assert ev <= mc.VALUE_TOL, (name, i, ev, val[i], rv[i])


@pytest.mark.parametrize("name", ["n130_m32_d6", "m3_mixed", "jitter_rbf"])
def test_two_calls_give_the_same_bits(name):
    ev, args = evaluator(name)
    a = ev.evaluate(*args)
    b = ev.evaluate(*args)
    c = device(name)  # another workspace
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_inputs_are_left_intact():
    ev, args = evaluator("m3_mixed")
    ev.evaluate(*args)
    data0, ils0 = ev.flat.clone(), ev.inv_ls.clone()
    ev.evaluate(*args)
    torch.cuda.synchronize()
    assert torch.equal(ev.flat, data0) and torch.equal(ev.inv_ls, ils0)
    ds = mc.data("m3_mixed")
    host = torch.cat([o["X"].reshape(-1) for o in ds] + [o["y"] for o in ds])
    assert torch.equal(ev.flat.cpu(), host)
    assert torch.equal(ev.inv_ls.cpu(), torch.stack([1.0 / o["ls"] for o in ds]))


def test_a_batched_call_equals_single_calls():
    val, grad, jit = device("m3_mixed")
    for i in range(3):
        ev, args = evaluator("m3_mixed", [i])
        v1, g1, j1 = ev.evaluate(*args)
        assert v1.tobytes() == val[i:i + 1].tobytes() and g1.tobytes() == grad[i:i + 1].tobytes()
        assert j1[0] == jit[i]


def test_not_positive_definite_is_a_linalg_error():
    """A matrix made indefinite on purpose (negative noise beyond the jitters): DKG_ERR_NOT_PD -> LinAlgError, an
    ordinary status path; the evaluator keeps working afterwards."""
    ev, args = evaluator("n33_rbf_d2")
    good = ev.evaluate(*args)
    with pytest.raises(torch.linalg.LinAlgError, match="not positive definite"):
        ev.evaluate(args[0], args[1], args[2], [-5.0])
    again = ev.evaluate(*args)
    assert good[1].tobytes() == again[1].tobytes()


def _first_evaluation(monkeypatch, device_arg, X, y, cfg):
    import scipy.optimize

    seen = {}

    def fake(fun, x0, jac=None, method=None, bounds=None, options=None):
        seen["f"], seen["g"] = fun(np.asarray(x0))
        return scipy.optimize.OptimizeResult(x=np.asarray(x0), fun=seen["f"], success=True, nit=0)

    monkeypatch.setattr(scipy.optimize, "minimize", fake)
    fit_map([X], [y], cfg, device=device_arg)
    monkeypatch.undo()
    return seen["f"], np.asarray(seen["g"])


def test_host_and_device_objective_agree(monkeypatch):
    """The first objective evaluation of fit_map (priors, softplus chain rule, / n included) on both routes;
    Matern-5/2, where the distance form does not matter."""
    cfg = reference_model_config(1, [[0, 0], [1, 1]], "once")
    X, y = _data(n=150, seed=3)
    fh, gh = _first_evaluation(monkeypatch, None, X, y, cfg)
    fd, gd = _first_evaluation(monkeypatch, DEV, X, y, cfg)
    eg, ev = np.abs(gd - gh).max() / np.abs(gh).max(), abs(fd - fh) / abs(fh)
    print(f"first evaluation: gradient error {eg:.3e} of max|g|, loss error {ev:.3e} relative")
    assert gd.shape == gh.shape
    assert eg <= mc.TOL and ev <= mc.VALUE_TOL


@functools.lru_cache(maxsize=None)
def _fits():
    cfg = reference_model_config(1, [[0, 0], [1, 1]], "once")
    X, y = _data(n=150, seed=3)
    return cfg, X, y, fit_map([X], [y], cfg, device=DEV), fit_map([X], [y], cfg)


def test_device_fit_against_the_generating_truth():
    """test_fit.py's test_fit_beats_the_generating_hyperparameters on the device route, judged by the CPU neg_mll."""
    cfg, X, y, res, _ = _fits()
    assert res["success"]
    truth = {"means": [0.3], "length_scales": [[0.15, 0.5]], "output_scales": [2.0], "noises": [1e-4]}
    fitted = {k: res[k] for k in KEYS}
    base = -neg_mll([X], [y], cfg, fitted)
    assert base >= -neg_mll([X], [y], cfg, truth) - 1e-9
    ls = res["length_scales"][0]
    assert ls[0] < ls[1]
    assert res["noises"] == [1e-4]  # fix_zero_noise: pinned at MIN_NOISE_SE**2, not fitted
    assert base == pytest.approx(res["mll"], rel=1e-9)
    for scale in (0.97, 1.03):
        moved = dict(fitted, output_scales=[fitted["output_scales"][0] * scale])
        assert -neg_mll([X], [y], cfg, moved) <= base + 1e-9


def test_device_fit_reaches_the_cpu_fits_objective():
    """Both fits' objectives re-evaluated by the CPU neg_mll: the device fit within 4 x the CPU's own gap between
    the expansion-form and the difference-form fit (module docstring)."""
    cfg, X, y, res, cpu = _fits()
    fd = -neg_mll([X], [y], cfg, {k: res[k] for k in KEYS})
    fc = -neg_mll([X], [y], cfg, {k: cpu[k] for k in KEYS})
    print(f"device fit {fd!r} ({res['iterations']} iterations), CPU fit {fc!r} ({cpu['iterations']}), "
          f"gap {abs(fd - fc):.3e}")
    assert abs(fd - fc) <= 4.0 * CPU_FIT_GAP


def test_fixed_means_are_kept_on_the_device_route():
    cfg = reference_model_config(2, [[0, 0], [1, 1]], "always")
    X, y = _data(n=60, seed=1)
    res = fit_map([X, X], [y, 2 * y], cfg, fixed_means=[0.123, -4.0], device=DEV)
    assert res["means"] == [0.123, -4.0]
    assert res["noises"] == [1e-4, 1e-4]


def test_mll_value_and_grad_checks_its_sizes():
    from dkg_amd.errors import UnsupportedError

    X = torch.rand(1025, 2)
    with pytest.raises(UnsupportedError):
        mll_value_and_grad([X], [X[:, 0]], {"means": [0.0], "length_scales": [[0.3, 0.3]], "output_scales": [1.0],
                                            "noises": [1e-2]}, {"outputs": [{}]}, DEV)


def test_smoke_pipeline_fits_on_the_device(tmp_path):
    """run_smoke(fit_hyperparams="always", fit_on_device=True) on the lengthscales/0 fixture: runs clean, writes the
    files test_smoke_pipeline_fitted_hyperparameters checks, KG > 0 at each chosen candidate."""
    from dkg_amd.catalog import DataCatalog

    state, *_ = load_golden("lengthscales0")
    hyper = dict(length_scales=[0.2, 1.8], output_scales=[1, 50], means=[0, 0])
    cat = DataCatalog("fit_device", data_dir=str(tmp_path))
    calls = []
    orig = fit._device_objective
    fit._device_objective = lambda outs, dev: calls.append(dev) or orig(outs, dev)
    try:
        res = run_smoke(GPProblem(state, device=DEV), hyper, seed=0, catalog=cat, fit_hyperparams="always",
                        fit_on_device=True)
    finally:
        fit._device_objective = orig
    assert len(calls) == 6 and all(c == DEV for c in calls)  # two runs, the first model and one per step
    for h in (res["separate"], res["full"]):
        assert len(h["x"]) == 2 and all(a == a and a > 0.0 for a in h["acq"])
    for key in ("eval_separate", "eval_full"):
        cat.uncompress_checkpoints(key)
        ck = cat.load_checkpoint(key, 2)
        sd = ck["model_state_dict"]
        assert float(sd["models.1.likelihood.noise_covar.raw_noise"]) == pytest.approx(1e-4)
        assert ck["model_config"]["fit_hyperparams"] == "always"
        raw = sd["models.0.covar_module.base_kernel.raw_lengthscale"]
        assert not torch.allclose(torch.nn.functional.softplus(raw), torch.tensor([[0.2, 0.2]], dtype=torch.double))
