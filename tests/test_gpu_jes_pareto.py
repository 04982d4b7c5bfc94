"""The JES Pareto sampler on the GPU (csrc/dkg_rff.hip, dkg_amd.jes_pareto): the weight posterior against the
numpy restatement (tests/rff_ref.py) on the same draws, the path evaluation against an extended-precision sum under a
derived rounding model and bit for bit across batch shapes, the batched generations against the stage entries and
the restatement, the pruning exactly, the sampler end to end, and the quality yardstick."""

import functools
import json
import os

import numpy as np
import pytest
import torch

import pareto_ref
import rff_cases
import rff_ref
from dkg_amd import _lib, nondominated_rank
from dkg_amd.jes import compute_sample_box_decomposition
from dkg_amd.jes_pareto import (RffPaths, pareto_nsga2_paths, pareto_prune, prune_pareto_front, rff_weights,
                                sample_discrete_pareto_optimal_points, sample_rff_paths)
from dkg_amd.optim import JesOptimisationSpec
from dkg_amd.pareto import pareto_draws, pareto_variation
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def as_dict(p: RffPaths):
    return {k: getattr(p, k).cpu().numpy() for k in ("omega", "bias", "coef", "offset")}


# ---------------------------------------------------------------- weights

@pytest.mark.parametrize("name", list(rff_cases.WEIGHT_CASES))
def test_weights_against_the_restatement(name):
    """Path values from the device's theta against the restatement's at 64 Sobol points and the training points, on
    the same draws: within 4 spread + 64 eps sum_r |coef_r| per (sample, output), spread the restatement's own floor
    (rows as given against rows reversed; tests/test_jes_pareto_host.py asserts spread <= 1e-6 y_std sqrt(s) for
    every case here).  omega and bias are two roundings of the draws."""
    state, draws, pts, ref, spread = rff_cases.weight_case(name)
    paths = rff_weights(state, *draws, device=DEV)
    got = as_dict(paths)
    assert float(paths.jitter.max()) == 0.0
    np.testing.assert_allclose(got["omega"], ref["omega"], rtol=4 * EPS, atol=0)
    np.testing.assert_allclose(got["bias"], ref["bias"], rtol=4 * EPS, atol=0)
    np.testing.assert_allclose(got["offset"], ref["offset"], rtol=0, atol=4 * EPS)  # |y_mean| + |y_std c| < 2
    Fd = paths(torch.from_numpy(pts)).cpu().numpy()
    Fr = rff_ref.evaluate(ref, pts)
    err = np.abs(Fd - Fr).max(1)  # [S, m]
    tol = 4.0 * spread + 64.0 * EPS * np.abs(ref["coef"]).sum(-1)
    print(f"{name}: worst err/tol {float((err / tol).max()):.3g} (err {err.max():.3g}, spread {spread.max():.3g})")
    assert (err <= tol).all(), float((err / tol).max())


def test_weights_gram_kernels_agree():
    """The VALU tiles of dkg_debug_rff_gram form the same matrix to rounding: the paths agree within the bound of
    the test above."""
    name = "n40-R100-d2-m2"
    state, draws, pts, ref, spread = rff_cases.weight_case(name)
    lib = _lib.load()
    a = rff_weights(state, *draws, device=DEV)(torch.from_numpy(pts)).cpu().numpy()
    assert lib.dkg_debug_rff_gram(1) == 0
    try:
        b = rff_weights(state, *draws, device=DEV)(torch.from_numpy(pts)).cpu().numpy()
    finally:
        lib.dkg_debug_rff_gram(0)
    tol = 4.0 * spread + 64.0 * EPS * np.abs(ref["coef"]).sum(-1)
    assert (np.abs(a - b).max(1) <= 2 * tol).all()


def test_weights_jitter_retries():
    """A rank-deficient system: 5 training rows under 64 features of which the second 32 repeat the first 32, at
    noise 1e-30, so Phi^T Phi + noise I has equal columns and rank 5 and its Cholesky meets a pivot <= 0.  With no
    retries the call reports NOT_PD; with three, a problem is factorised with the policy's absolute jitter
    (1e-8 * 10^i) and the path is finite."""
    from dkg_amd.errors import NotPSDError
    from dkg_amd.jes_pareto import draw_rff_randomness

    state = rff_cases.make_state((5, 5), 2, ("RBF", "M52"), False, 1e-30, 1.0, 0.4, 77)
    wn, g, ub, z = draw_rff_randomness(torch.Generator().manual_seed(78), [None, 2.5], 2, 64, 2)
    for t in (wn, g, ub):
        t[:, :, 32:] = t[:, :, :32]
    with pytest.raises(NotPSDError, match="not positive definite after 0 jitter"):
        rff_weights(state, wn, g, ub, z, device=DEV, max_tries=0)
    paths = rff_weights(state, wn, g, ub, z, device=DEV, max_tries=3)
    jit = paths.jitter
    print(f"jitter used: {jit.tolist()}")
    assert jit.shape == (2, 2) and bool((jit > 0).any())  # the refusal above shows that a first attempt fails
    assert all(v == 0.0 or any(abs(v / j - 1) < 1e-12 for j in (1e-8, 1e-7, 1e-6)) for v in jit.reshape(-1).tolist())
    X = torch.rand(9, 2, dtype=torch.double, generator=torch.Generator().manual_seed(1))
    assert bool(torch.isfinite(paths.coef).all()) and bool(torch.isfinite(paths(X)).all())
    # the next call on a well-conditioned model is unaffected
    state2, draws2 = rff_cases.weight_case("n10-R64-d1-m1")[:2]
    assert float(rff_weights(state2, *draws2, device=DEV).jitter.max()) == 0.0


# ---------------------------------------------------------------- evaluation

EVAL_SHAPES = [(3, 2, 2, 64), (2, 3, 6, 100), (3, 1, 16, 512), (1, 2, 1, 1024), (2, 8, 3, 65)]  # S, m, d, R


@functools.lru_cache(maxsize=None)
def random_paths(S, m, d, R):
    g = torch.Generator().manual_seed(1000 * S + 100 * m + 10 * d + R)
    r = lambda *s: torch.randn(*s, dtype=torch.double, generator=g)  # noqa: E731
    omega = 4.0 * r(S, m, R, d)
    bias = 2 * np.pi * torch.rand(S, m, R, dtype=torch.double, generator=g)
    coef = r(S, m, R) / np.sqrt(R)
    offset = r(S, m)
    X = torch.rand(S, 40, d, dtype=torch.double, generator=g)
    return RffPaths(*(t.to(DEV) for t in (omega, bias, coef, offset))), X


@pytest.mark.parametrize("S,m,d,R", EVAL_SHAPES)
def test_eval_against_extended_precision(S, m, d, R):
    """The bound is rff_ref.evaluate_longdouble's rounding model (derived there, u = 2^-53): the phase's d + 1
    roundings through cos, the 2 ulp of cos, ceil(R / 64) + 7 roundings of the sum, one of the result; twice the
    first-order sum."""
    paths, X = random_paths(S, m, d, R)
    got = paths(X).cpu().numpy()
    want, bound = rff_ref.evaluate_longdouble(as_dict(paths), X.numpy())
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f"S={S} m={m} d={d} R={R}: worst err/bound {float((err / bound).max()):.3g}")
    assert got.shape == (S, 40, m) and (err <= bound).all(), float((err / bound).max())
    shared = paths(X[0]).cpu().numpy()
    want0, bound0 = rff_ref.evaluate_longdouble(as_dict(paths), X[0].numpy())
    assert (np.abs(shared.astype(np.longdouble) - want0).astype(np.float64) <= bound0).all()


@pytest.mark.parametrize("S,m,d,R", [(3, 2, 2, 64), (3, 1, 16, 512), (3, 3, 6, 100)])
def test_eval_bits_do_not_depend_on_the_batch(S, m, d, R):
    paths, X = random_paths(S, m, d, R)
    full = paths(X[:, :17])  # [S, 17, m]
    for P in (1, 15, 16, 17):
        assert bits(paths(X[:, :P])) == bits(full[:, :P])
    # across rows: the points in reverse order
    assert bits(paths(X[:, :17].flip(1)).flip(1)) == bits(full)
    # across samples: each sample alone (S = 1), and shared points
    for s in range(S):
        assert bits(paths.sample(s)(X[s:s + 1, :17])) == bits(full[s:s + 1])
    shared = paths(X[1, :17])
    assert bits(shared[1]) == bits(full[1])
    assert bits(paths.sample(2)(X[1, :17])[0]) == bits(shared[2])


# ---------------------------------------------------------------- generations

GEN_SHAPES = [(3, 8, 1, 1), (3, 12, 2, 2), (2, 64, 3, 3), (3, 100, 2, 2), (1, 8, 5, 2)]  # S, P, d, m
PRM = dict(cr=0.9, eta_c=15.0, eta_m=20.0)


@functools.lru_cache(maxsize=None)
def gen_case(S, d, m):
    paths, _ = random_paths(S, m, d, 100)
    g = np.random.default_rng(d + m)
    return paths, -0.25 - 0.5 * g.random(d), 1.0 + 0.5 * g.random(d)


def uniforms_for(S, P, d, gens, seed):
    return torch.rand(S, P * d + gens * pareto_ref.draws(P, d), dtype=torch.double,
                      generator=torch.Generator().manual_seed(seed)).to(DEV)


def manual_step(path, lb, ub, X, F, rank, crowd, u, pm):
    """One generation of one sample from the stage entries; the glue (normalise, concatenate, gather) in torch."""
    lbt, ubt = torch.from_numpy(lb).to(DEV), torch.from_numpy(ub).to(DEV)
    C = pareto_variation(X, rank, crowd, lb, ub, u, cr=PRM["cr"], eta_c=PRM["eta_c"], m=pm, eta_m=PRM["eta_m"])
    FC = path((C - lbt) / (ubt - lbt))[0]
    X2, F2 = torch.cat([X, C]), torch.cat([F, FC])
    r2, c2, order = nondominated_rank(F2, X.shape[0])
    sel = order[:X.shape[0]].long()
    return (X2[sel], F2[sel], r2[sel], c2[sel]), (X2, F2, order)


@pytest.mark.parametrize("S,P,d,m", GEN_SHAPES)
def test_one_batched_generation(S, P, d, m):
    """Sample s of one batched generation equals the per-sample stage sequence bit for bit, and its survivors are
    the restatement's survivors of the device's [parents; children] and their device objectives."""
    paths, lb, ub = gen_case(S, d, m)
    pm = min(0.5, 1.0 / d)
    u = uniforms_for(S, P, d, 1, 5 * P + d)
    X0, F0, r0, c0 = pareto_nsga2_paths(paths, lb, ub, P, 0, u[:, :P * d].contiguous())
    X1, F1, r1, c1 = pareto_nsga2_paths(paths, lb, ub, P, 1, u)
    lbt, ubt = torch.from_numpy(lb).to(DEV), torch.from_numpy(ub).to(DEV)
    for s in range(S):
        Xi = np.clip(lb + u[s, :P * d].cpu().numpy().reshape(P, d) * (ub - lb), lb, ub)
        assert bits(X0[s]) == Xi.tobytes()
        assert bits(F0[s]) == bits(paths.sample(s)((X0[s] - lbt) / (ubt - lbt))[0])
        r, c, _ = pareto_ref.rank_crowd_order(F0[s].cpu().numpy(), P)
        assert r0[s].cpu().numpy().tolist() == r.tolist() and bits(c0[s]) == c.tobytes()
        (Xm, Fm, rm, cm), (X2, F2, order) = manual_step(paths.sample(s), lb, ub, X0[s], F0[s], r0[s], c0[s],
                                                        u[s, P * d:], pm)
        for a, b in ((Xm, X1[s]), (Fm, F1[s]), (rm, r1[s]), (cm, c1[s])):
            assert bits(a) == bits(b)
        Xr, Fr, rr, cr_, orr = pareto_ref.survive(X2.cpu().numpy(), F2.cpu().numpy(), P)
        assert order.cpu().numpy().tolist() == orr.tolist()
        assert bits(X1[s]) == Xr.tobytes() and bits(F1[s]) == Fr.tobytes()
        assert r1[s].cpu().numpy().tolist() == rr.tolist() and bits(c1[s]) == cr_.tobytes()
    assert bool(((X1 >= lbt) & (X1 <= ubt)).all())


@pytest.mark.parametrize("P", [8, 100])
def test_whole_call_equals_single_sample_calls(P):
    S, d, m, gens = 3, 2, 2, 3
    paths, lb, ub = gen_case(S, d, m)
    u = uniforms_for(S, P, d, gens, 77 + P)
    whole = pareto_nsga2_paths(paths, lb, ub, P, gens, u)
    again = pareto_nsga2_paths(paths, lb, ub, P, gens, u)
    for s in range(S):
        one = pareto_nsga2_paths(paths.sample(s), lb, ub, P, gens, u[s:s + 1].contiguous())
        for a, b, c in zip(whole, again, one):
            assert bits(a[s]) == bits(b[s]) == bits(c[0])
    raw = pareto_nsga2_paths(paths, lb, ub, P, 0, u[:, :P * d].contiguous(), raw_inputs=True)
    assert bits(raw[1]) == bits(paths(raw[0]))


def test_exact_copies_get_equal_objectives():
    """cr = 0 and m = 0: every child is a bit-exact copy of a parent and must get its parent's objectives' bits."""
    S, P, d, m = 3, 12, 2, 2
    paths, lb, ub = gen_case(S, d, m)
    u = uniforms_for(S, P, d, 2, 9)
    X, F, _, _ = pareto_nsga2_paths(paths, lb, ub, P, 2, u, cr=0.0, m=0.0)
    X0, F0, _, _ = pareto_nsga2_paths(paths, lb, ub, P, 0, u[:, :P * d].contiguous())
    for s in range(S):
        rows = {bits(x): bits(f) for x, f in zip(X0[s], F0[s])}
        for x, f in zip(X[s], F[s]):
            assert rows[bits(x)] == bits(f)


# ---------------------------------------------------------------- pruning

def front_like(Q, m, seed, dup=False):
    g = np.random.default_rng(seed)
    if m == 1:
        F = g.random((Q, 1))
    else:
        t = np.sort(g.random(Q))
        F = np.stack([t, 1.0 - t ** 2] + [g.random(Q) for _ in range(m - 2)], -1)
        F[::5] -= 0.3 * g.random((len(F[::5]), m))  # some dominated members
    if dup and Q >= 4:
        F[Q // 2] = F[1]
        F[Q - 1] = F[1]
    return F


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("Q", [1, 2, 9, 200])
def test_prune_is_the_restatement(Q, m):
    for dup in (False, True):
        F = front_like(Q, m, 10 * Q + m, dup)
        rank = pareto_ref.rank_crowd_order(F, 1)[0]
        Fd, rd = torch.from_numpy(F).to(DEV)[None], torch.from_numpy(rank).to(DEV)[None]
        for k in sorted({1, 2, 10, Q}):
            count, index = pareto_prune(Fd, rd, k)
            want = rff_ref.prune(F, rank, k)
            assert int(count[0]) == len(want) <= k
            assert index[0].cpu().tolist() == want + [-1] * (k - len(want))


def test_prune_samples_of_different_sizes():
    Q, m, k = 40, 2, 6
    Fs = np.stack([front_like(Q, m, 3), front_like(Q, m, 4, dup=True), front_like(Q, m, 5)])
    ranks = np.stack([pareto_ref.rank_crowd_order(F, 1)[0] for F in Fs])
    ranks[1, 10:] = -1  # a short sample
    ranks[2] = -1
    ranks[2, 7] = 0  # a front of one point
    count, index = pareto_prune(torch.from_numpy(Fs).to(DEV), torch.from_numpy(ranks).to(DEV), k)
    for s in range(3):
        want = rff_ref.prune(Fs[s], ranks[s], k)
        assert int(count[s]) == len(want) and index[s].cpu().tolist() == want + [-1] * (k - len(want))
    assert int(count[2]) == 1
    ps, pf = prune_pareto_front(np.arange(Q, dtype=np.float64)[:, None], Fs[0], k, device=DEV)
    want = rff_ref.prune(Fs[0], pareto_ref.rank_crowd_order(Fs[0], 1)[0], k)
    assert ps[:, 0].astype(int).tolist() == want and pf.tobytes() == Fs[0][want].tobytes()


# ---------------------------------------------------------------- end to end

def nondominated(F):
    return not pareto_ref.dominance_matrix(F).any()


def test_sampler_end_to_end():
    state, *_ = load_golden("lengthscales0")
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.double)
    kw = dict(num_rffs=128, nsga2_pop_size=40, nsga2_generations=30, seed=0, device=DEV)
    before = torch.random.get_rng_state()
    sets, fronts = sample_discrete_pareto_optimal_points(state, bounds, 3, 5, **kw)
    sets2, fronts2 = sample_discrete_pareto_optimal_points(state, bounds, 3, 5, **kw)
    assert torch.equal(before, torch.random.get_rng_state())  # the global torch RNG is never touched
    paths = sample_rff_paths(state, 3, 128, seed=0, device=DEV)  # the sampler's first draws are the paths'
    assert len(sets) == len(fronts) == 3
    for s, (ps, pf) in enumerate(zip(sets, fronts)):
        assert torch.equal(ps, sets2[s]) and torch.equal(pf, fronts2[s])
        k = ps.shape[0]
        assert 1 <= k <= 5 and ps.shape == (k, 2) and pf.shape == (k, 2) and ps.dtype == torch.double
        assert bool(((ps >= 0) & (ps <= 1)).all())
        assert nondominated(pf.numpy())
        assert bits(paths.sample(s)(ps)[0]) == bits(pf)
    boxes = compute_sample_box_decomposition(fronts)
    assert boxes.shape[0] == 3 and boxes.shape[1] == 2 and boxes.shape[3] == 2
    # one output: one point per sample
    one = type(state)(state.models[0])
    s1, f1 = sample_discrete_pareto_optimal_points(one, torch.tensor([[0.0, 0.0], [1.0, 1.0]]), 2, 5,
                                                   num_rffs=64, nsga2_pop_size=16, nsga2_generations=5, seed=1,
                                                   device=DEV)
    assert [tuple(t.shape) for t in s1] == [(1, 2)] * 2 and [tuple(t.shape) for t in f1] == [(1, 1)] * 2


def test_spec_with_device_sampler_optimises():
    import jes_cases

    state = jes_cases.problem(jes_cases.OPT_CASE)[0]  # the model test_gpu_jes.py's spec test optimises on
    d = state.input_dim
    spec = JesOptimisationSpec.with_device_sampler("LB", 3, 5, 2, 8, 1, 5, device=DEV, seed=0, num_rffs=64,
                                                   nsga2_pop_size=24, nsga2_generations=10)
    x, i, v = spec.optimize_for_single_objective(state, [1.0] * state.num_outputs, d)
    assert x.shape == (1, d) and bool(((x >= 0) & (x <= 1)).all()) and 0 <= int(i) < state.num_outputs
    assert bool(torch.isfinite(v).all())


# ---------------------------------------------------------------- quality

def test_quality_of_the_evolved_front():
    """HV(non-dominated final population) / HV(the same path's front on a 129 x 129 grid) at seed 0 against the
    threshold of the CPU restatement over seeds 0-4 (tests/golden/jes_pareto_quality.json, made by
    tests/golden/make_jes_pareto_quality.py): t = r_min - 2 (r_max - r_min)."""
    q = json.load(open(os.path.join(HERE, "golden", "jes_pareto_quality.json")))
    state, *_ = load_golden("lengthscales0")
    gen = torch.Generator().manual_seed(0)
    paths = sample_rff_paths(state, 1, q["R"], device=DEV, generator=gen)
    P, gens = q["P"], q["gen"]
    u = torch.rand(1, P * 2 + gens * pareto_draws(P, 2), dtype=torch.double, generator=gen)
    X, F, rank, _ = pareto_nsga2_paths(paths, [0.0, 0.0], [1.0, 1.0], P, gens, u)
    ax = torch.linspace(0.0, 1.0, q["grid"], dtype=torch.double)
    G = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    FG = paths(G)[0].cpu().numpy()
    ref = FG.min(0) - 0.1 * (FG.max(0) - FG.min(0))
    f = F[0].cpu().numpy()[rank[0].cpu().numpy() == 0]
    ratio = pareto_ref.hypervolume_2d(f, ref) / pareto_ref.hypervolume_2d(FG, ref)
    print(f"HV(front) / HV(grid) = {ratio:.6f} (CPU seeds {q['r']}, t = {q['t']:.6f})")
    assert ratio >= q["t"]
