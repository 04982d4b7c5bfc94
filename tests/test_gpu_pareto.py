"""The device NSGA-II and the BO metrics on the GPU (csrc/dkg_pareto.hip, dkg_amd.pareto, dkg_amd.metrics,
bo_smoke's metrics=True): the posterior-mean kernel against an extended-precision sum over the device's own alpha,
rank / crowding / order and one generation against the numpy restatement (tests/pareto_ref.py) exactly, variation
against it to a few ulp of its terms, the whole call against its stages bit for bit, the sampled front against the
committed CPU quality yardstick, and the SMOKE pipeline with metrics."""

import functools
import json
import os

import numpy as np
import pytest
import torch

import pareto_ref
from dkg_amd import nondominated_rank, posterior_mean, sample_points_on_pareto_front
from dkg_amd.pareto import PreparedModel, pareto_draws, pareto_nsga2, pareto_variation
from helpers import ALL_FAMILIES, grad_case, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


# ---------------------------------------------------------------- posterior mean

MEAN_MODELS = {
    # the parity suite's odd shapes: 3 outputs, n = 37 / 50 / 23, d = 3, Standardize (y_mean != 0, y_std != 1)
    "odd-M52-M32-M12": dict(m=3, d=3, ns=(37, 50, 23), families=ALL_FAMILIES, seed=22),
    "odd-RBF-M12-M52": dict(m=3, d=3, ns=(37, 50, 23), families=("RBF", "M12", "M52"), seed=23),
    "n1": dict(m=2, d=2, ns=(1, 5), families=("M52", "RBF"), seed=24),
    "n1024-d16": dict(m=2, d=16, ns=(1024, 70), families=("M52", "M32"), seed=25),
}


@functools.lru_cache(maxsize=None)
def mean_model(name):
    kw = MEAN_MODELS[name]
    state = grad_case(kw["m"], kw["d"], kw["ns"], kw["families"], 4, 2, 1000, kw["seed"])[0]
    X = torch.rand(1000, kw["d"], dtype=torch.double, generator=torch.Generator().manual_seed(kw["seed"]))
    return state, PreparedModel(state, DEV), X


def longdouble_mean(pm, X):
    """y_mean + y_std (c + sum_j s k_j alpha_j) in extended precision from the device's own alpha and inverse
    lengthscales, distances in difference form; -> (value [P, m], magnitude |c| + sum_j |s k_j alpha_j| [P, m])."""
    ld = np.longdouble
    x = X.numpy().astype(ld)
    vals, mags = [], []
    for c in pm.outputs:
        st = c.state
        n = st.num_train
        il = c.inv_ls.cpu().numpy().astype(ld)
        z = c.train_x.cpu().numpy().astype(ld)
        al = c.alpha.cpu().numpy()[:n].astype(ld)
        t = (x[:, None, :] - z[None, :, :]) * il
        r2 = (t * t).sum(-1)
        if st.kernel == "rbf":
            k = np.exp(-r2 / 2)
        else:
            r = np.sqrt(r2)
            a = np.sqrt(ld(2 * st.nu)) * r
            poly = {0.5: 1.0, 1.5: 1.0 + a, 2.5: 1.0 + a + ld(5) / 3 * r2}[float(st.nu)]
            k = poly * np.exp(-a)
        terms = ld(float(st.outputscale)) * k * al
        s = ld(float(st.mean_constant)) + terms.sum(-1)
        vals.append(ld(float(st.y_mean)) + ld(float(st.y_std)) * s)
        mags.append(float(st.y_std) * (abs(float(st.mean_constant)) + np.abs(terms).sum(-1)))
    return np.stack(vals, -1), np.stack(mags, -1).astype(np.float64)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", list(MEAN_MODELS))
def test_posterior_mean_against_extended_precision(name, P):
    """Tolerance 64 eps y_std (|c| + sum_j |s k_j alpha_j|) + eps |result|: the rounding bound of an n <= 1024 term
    sum (16 fma per lane, a 6-step tree) of kernel terms good to a few ulp; derived, not tuned."""
    state, pm, X = mean_model(name)
    got = posterior_mean(pm, X[:P]).cpu().numpy()
    want, mag = longdouble_mean(pm, X[:P])
    tol = 64 * EPS * mag + EPS * np.abs(want).astype(np.float64)
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f"{name} P={P}: worst err/tol {float((err / tol).max()):.3g}")
    assert got.shape == (P, state.num_outputs) and (err <= tol).all(), float((err / tol).max())


def test_posterior_mean_end_to_end_against_the_oracle():
    state, om, D, W, X, _ = load_golden("lengthscales0")
    got = posterior_mean(state, X, device=DEV).cpu()
    ref = torch.stack([p[0] for p in om.posterior_list(X, observation_noise=False)], dim=-1)
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-9 * float(ref.abs().max()))


@pytest.mark.parametrize("name", ["odd-M52-M32-M12", "n1024-d16"])
def test_posterior_mean_bits_do_not_depend_on_the_batch(name):
    _, pm, X = mean_model(name)
    x = X[5:6]
    alone = bits(posterior_mean(pm, x))
    for P in (18, 64, 65, 1000):
        for row in (0, 17, P - 1):
            B = X[:P].clone()
            B[row] = x[0]
            assert bits(posterior_mean(pm, B)[row:row + 1]) == alone, (P, row)


# ---------------------------------------------------------------- rank, crowding, order

def rank_input(kind, Q, m):
    g = np.random.default_rng(1000 * Q + m)
    if kind == "gauss":
        return g.standard_normal((Q, m))
    if kind == "equal":
        return np.full((Q, m), 1.25)
    if kind == "chain":
        return np.repeat(np.arange(Q, dtype=np.float64)[:, None], m, 1)
    if kind == "grid":
        return g.integers(0, 5, size=(Q, m)).astype(np.float64)
    if kind == "dup":
        half = g.standard_normal(((Q + 1) // 2, m))
        return np.concatenate([half, half])[:Q]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def rank_reference(kind, Q, m, keep):
    return pareto_ref.rank_crowd_order(rank_input(kind, Q, m), keep)


def check_rank(kind, Q, m):
    F = rank_input(kind, Q, m)
    Fd = torch.from_numpy(F).to(DEV)
    for keep in sorted({Q, max(Q // 2, 1), 1}):
        rank, crowd, order = nondominated_rank(Fd, keep)
        r, c, o = rank_reference(kind, Q, m, keep)
        assert rank.dtype == torch.int32 and order.dtype == torch.int32 and crowd.dtype == torch.double
        assert rank.cpu().numpy().tolist() == r.tolist(), (kind, Q, m, keep)
        assert bits(crowd) == c.tobytes(), (kind, Q, m, keep)
        assert order.cpu().numpy().tolist() == o.tolist(), (kind, Q, m, keep)
        unranked = r < 0
        assert (rank.cpu().numpy()[unranked] == -1).all() and (crowd.cpu().numpy()[unranked] == 0.0).all()
        assert int((r >= 0).sum()) >= keep


@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("Q", [1, 2, 63, 64, 65, 257, 2048])
def test_rank_gaussian(Q, m):
    check_rank("gauss", Q, m)


@pytest.mark.parametrize("kind,Q,m", [("equal", 65, 3), ("equal", 2048, 2), ("chain", 257, 2), ("chain", 257, 1),
                                      ("grid", 257, 2), ("grid", 2048, 3), ("grid", 64, 8), ("dup", 130, 2),
                                      ("dup", 2048, 3), ("dup", 63, 1)])
def test_rank_structured_inputs(kind, Q, m):
    check_rank(kind, Q, m)


# ---------------------------------------------------------------- variation

def population(P, d, seed):
    g = np.random.default_rng(seed)
    lb, ub = -0.5 - g.random(d), 1.0 + g.random(d)
    X = lb + g.random((P, d)) * (ub - lb)
    rank, crowd, _ = pareto_ref.rank_crowd_order(g.standard_normal((P, 2)))
    u = torch.rand(pareto_ref.draws(P, d), dtype=torch.double, generator=torch.Generator().manual_seed(seed)).numpy()
    return X, rank, crowd, lb, ub, u


def device_variation(X, rank, crowd, lb, ub, u, **prm):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return pareto_variation(t(X), t(rank), t(crowd), lb, ub, t(u), **prm).cpu().numpy()


@pytest.mark.parametrize("P,d", [(8, 1), (12, 2), (64, 3), (1024, 16)])
def test_variation_against_the_restatement(P, d):
    """Per coordinate within 256 eps ((ub - lb) + max(|lb|, |ub|)): both sides evaluate the same fp64 expressions
    on the same uniforms except pow, whose arguments are conditioned by exponents of at most eta_m + 1 = 51 and on
    which libm and the device differ by a few ulp."""
    assert pareto_draws(P, d) == pareto_ref.draws(P, d)
    X, rank, crowd, lb, ub, u = population(P, d, 7 * P + d)
    tol = 256 * EPS * ((ub - lb) + np.maximum(np.abs(lb), np.abs(ub)))
    for prm in (pareto_ref.DEFAULTS, dict(cr=1.0, eta_c=10.0, m=1.0, eta_m=50.0)):
        got = device_variation(X, rank, crowd, lb, ub, u, **prm)
        want = pareto_ref.variation(X, rank, crowd, lb, ub, u, **prm)
        err = np.abs(got - want)
        print(f"P={P} d={d} {prm}: worst err/tol {float((err / tol).max()):.3g}")
        assert (err <= tol).all(), float((err / tol).max())
        assert (got >= lb).all() and (got <= ub).all()
        assert device_variation(X, rank, crowd, lb, ub, u, **prm).tobytes() == got.tobytes()  # same uniforms, same bits
    winners = X[pareto_ref.tournament_winners(rank, crowd, u, P)]
    copies = device_variation(X, rank, crowd, lb, ub, u, cr=0.0, eta_c=10.0, m=0.0, eta_m=50.0)
    assert copies.tobytes() == winners.tobytes()
    moved = device_variation(X, rank, crowd, lb, ub, u, cr=1.0, eta_c=10.0, m=1.0, eta_m=50.0)
    assert (moved != winners).mean() > 0.9


# ---------------------------------------------------------------- one generation, the whole call

# (12, 5, 2) and (8, 9, 1): d below its bucket of 8 / 16, where the fused normalisation's clamped coordinate is live
GEN_SHAPES = [(8, 1, 1), (12, 2, 2), (64, 3, 3), (1024, 16, 8), (12, 5, 2), (8, 9, 1)]
GEN_NS = (20, 31, 16, 45, 27, 38, 18, 52)


@functools.lru_cache(maxsize=None)
def gen_model(d, m):
    state = grad_case(m, d, GEN_NS[:m], ALL_FAMILIES, 4, 2, 4, 100 * d + m)[0]
    g = np.random.default_rng(d + m)
    lb, ub = -0.25 - 0.5 * g.random(d), 1.0 + 0.5 * g.random(d)
    return PreparedModel(state, DEV), lb, ub


def uniforms_for(P, d, gens, seed):
    return torch.rand(P * d + gens * pareto_ref.draws(P, d), dtype=torch.double,
                      generator=torch.Generator().manual_seed(seed))


def manual_step(pm, lb, ub, X, F, rank, crowd, u):
    """One generation from the three stage entries; the glue (normalise, concatenate, gather) in torch."""
    lbt, ubt = torch.from_numpy(lb).to(DEV), torch.from_numpy(ub).to(DEV)
    C = pareto_variation(X, rank, crowd, lb, ub, u)
    FC = posterior_mean(pm, (C - lbt) / (ubt - lbt))
    X2, F2 = torch.cat([X, C]), torch.cat([F, FC])
    r2, c2, order = nondominated_rank(F2, X.shape[0])
    sel = order[:X.shape[0]].long()
    return (X2[sel], F2[sel], r2[sel], c2[sel]), (X2, F2, order)


@pytest.mark.parametrize("P,d,m", GEN_SHAPES)
def test_one_generation_against_the_restatement(P, d, m):
    """The device's children and their device objectives through pareto_ref's rank and survival: exactly the
    device's survivors, in order, with their ranks and crowding."""
    pm, lb, ub = gen_model(d, m)
    u = uniforms_for(P, d, 1, 3 * P + d).to(DEV)
    X0, F0, r0, c0 = pareto_nsga2(pm, lb, ub, P, 0, u)
    (X1, F1, r1, c1), (X2, F2, order) = manual_step(pm, lb, ub, X0, F0, r0, c0, u[P * d:])
    Xr, Fr, rr, cr_, orr = pareto_ref.survive(X2.cpu().numpy(), F2.cpu().numpy(), P)
    assert order.cpu().numpy().tolist() == orr.tolist()
    assert bits(X1) == Xr.tobytes() and bits(F1) == Fr.tobytes()
    assert r1.cpu().numpy().tolist() == rr.tolist() and bits(c1) == cr_.tobytes()
    Xn, Fn, rn, cn = pareto_nsga2(pm, lb, ub, P, 1, u)
    assert bits(Xn) == bits(X1) and bits(Fn) == bits(F1) and bits(rn) == bits(r1) and bits(cn) == bits(c1)
    lbt, ubt = torch.from_numpy(lb).to(DEV), torch.from_numpy(ub).to(DEV)
    assert bool(((Xn >= lbt) & (Xn <= ubt)).all())


def test_whole_call_equals_its_stages():
    P, d, m, gens = 64, 3, 3, 3
    pm, lb, ub = gen_model(d, m)
    u = uniforms_for(P, d, gens, 99).to(DEV)
    n = pareto_ref.draws(P, d)
    # gens = 0: the ranked initial sample, in sampled order
    X, F, rank, crowd = pareto_nsga2(pm, lb, ub, P, 0, u)
    X0 = np.clip(lb + u[:P * d].cpu().numpy().reshape(P, d) * (ub - lb), lb, ub)
    assert bits(X) == X0.tobytes()
    assert bits(F) == bits(posterior_mean(pm, torch.from_numpy((X0 - lb) / (ub - lb))))
    r, c, _ = pareto_ref.rank_crowd_order(F.cpu().numpy(), P)
    assert rank.cpu().numpy().tolist() == r.tolist() and bits(crowd) == c.tobytes()
    for g in range(gens):
        (X, F, rank, crowd), _ = manual_step(pm, lb, ub, X, F, rank, crowd, u[P * d + g * n:P * d + (g + 1) * n])
    whole = pareto_nsga2(pm, lb, ub, P, gens, u)
    again = pareto_nsga2(pm, lb, ub, P, gens, u)
    for a, b, c2 in zip((X, F, rank, crowd), whole, again):
        assert bits(a) == bits(b) and bits(b) == bits(c2)
    # a test problem's model takes the points as they are
    raw = pareto_nsga2(pm, lb, ub, P, 0, u, raw_inputs=True)
    assert bits(raw[0]) == X0.tobytes() and bits(raw[1]) == bits(posterior_mean(pm, torch.from_numpy(X0)))


# ---------------------------------------------------------------- the sampled front, the pipeline

def quality():
    return json.load(open(os.path.join(HERE, "golden", "pareto_quality.json")))


def test_sampled_front_of_the_golden_surrogate():
    q = quality()
    state, *_ = load_golden("lengthscales0")
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]])
    before = torch.random.get_rng_state()
    x, f = sample_points_on_pareto_front(state, bounds, npoints=q["P"], gen=q["gen"], seed=0, device=DEV)
    sample_points_on_pareto_front(state, bounds, npoints=8, gen=1, seed=None, device=DEV)
    assert torch.equal(before, torch.random.get_rng_state())  # the global torch RNG is never touched
    assert isinstance(x, np.ndarray) and isinstance(f, np.ndarray)
    assert x.shape == (100, 2) and f.shape == (100, 2) and x.dtype == np.float64 and f.dtype == np.float64
    assert (x >= 0.0).all() and (x <= 1.0).all()
    assert bits(posterior_mean(state, torch.from_numpy(x), device=DEV)) == f.tobytes()
    rank = pareto_ref.rank_crowd_order(f)[0]
    ratio = pareto_ref.hypervolume_2d(f[rank == 0], q["ref_point"]) / q["H_grid"]
    print(f"HV(front) / H_grid = {ratio:.6f} (CPU seeds {q['r']}, t = {q['t']:.6f})")
    assert ratio >= q["t"]
    x2, f2 = sample_points_on_pareto_front(state, bounds, npoints=q["P"], gen=q["gen"], seed=0, device=DEV)
    assert x2.tobytes() == x.tobytes() and f2.tobytes() == f.tobytes()


def test_smoke_pipeline_with_metrics(tmp_path):
    from dkg_amd.bo_smoke import METRICS_COLUMNS, TIMINGS_COLUMNS, GPProblem, run_smoke
    from dkg_amd.catalog import DataCatalog

    hyper = dict(length_scales=[0.2, 1.8], output_scales=[1, 50], means=[0, 0])
    state, *_ = load_golden("lengthscales0")
    shared = DataCatalog.load_shared_gp_test_problem_data("lengthscales/0", data_dir=os.path.join(HERE, "golden"))
    cat = DataCatalog("metrics", data_dir=str(tmp_path))
    problem = GPProblem(state, device=DEV, ref_point=shared["ref_point"], max_hv=shared["max_hv"])
    assert problem.max_hv == shared["max_hv"] and problem.ref_point.tolist() == list(shared["ref_point"])
    res = run_smoke(problem, hyper, seed=0, metrics=True, catalog=cat)
    plain = run_smoke(GPProblem(state, device=DEV), hyper, seed=0)
    assert res["full"]["x"] == plain["full"]["x"] and res["separate"]["x"] == plain["separate"]["x"]
    assert "metrics_history" not in plain["full"]
    pset, pfront = cat.load_true_pareto()
    assert pset.shape == (100, 2) and pfront.shape == (100, 2)
    best = cat.load_problem_max_possible_expected_scalarisation()
    assert np.isfinite(best) and best == res["max_possible_expected_scalarisation"]
    for key, mode in (("eval_separate", "separate"), ("eval_full", "full")):
        assert cat.num_posterior_pareto_iterations(key) == 3
        for it in range(3):
            ps, pf = cat.load_posterior_pareto(key, it)
            assert ps.shape == (100, 2) and pf.shape == (100, 2)
        df = cat.load_metrics(key)
        assert tuple(df.columns) == METRICS_COLUMNS and len(df) == 3
        assert np.isfinite(df.to_numpy(dtype=np.float64)).all()
        assert (df["pfront_hv_lo"] <= df["pfront_hv_hi"]).all()
        qh = cat.load_bo_run(key)
        assert df["cost"].tolist() == [float(qh.loc[qh["iteration"] <= it, "cost"].sum()) for it in range(3)]
        assert (df["actual_scalarperf"] <= best + 1e-9 * abs(best)).all()
        tm = cat.load_timings(key)
        assert tuple(tm.columns) == TIMINGS_COLUMNS and tm["iteration"].tolist() == [0, 1, 2]
        assert len(res[mode]["metrics_history"]) == 3 and len(res[mode]["timings_history"]) == 3
