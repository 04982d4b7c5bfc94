"""The dominated-space box kernels on the GPU (csrc/dkg_boxes.hip, dkg_amd.boxes): the boxes against
the restatement of the specification (tests/boxes_ref.py) bit for bit, the hypervolume against the exact sum of
the restatement's boxes under the rounding bound of include/dkg.h, the JES acquisition at three objectives on
the device boxes against tests/jes_oracle.py, the spec, and the metrics' device route.

Measured on MI355X: the worst |hv - exact| / bound is in DESIGN.md 8g.
"""

import math

import numpy as np
import pytest
import torch

import boxes_jes_case as jc
import boxes_ref as br
import jes_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 3, 63, 64, 65, 257)
SHAPES = [(m, K) for m in (1, 2, 3) for K in SIZES]


def device_boxes(fronts, ref, K=None):
    """The sets padded to K rows with ref itself -> (bounds [S, 2, bound, m], count [S]) as numpy."""
    from dkg_amd.boxes import dominated_boxes_device

    m = fronts[0].shape[1]
    K = K or max(f.shape[0] for f in fronts)
    Y = np.tile(np.asarray(ref, dtype=np.float64), (len(fronts), K, 1))
    for s, f in enumerate(fronts):
        Y[s, : f.shape[0]] = f
    bounds, count = dominated_boxes_device(torch.from_numpy(Y).to(DEV), list(ref))
    assert bounds.shape == (len(fronts), 2, br.count_bound(K, m), m)
    return bounds.cpu().numpy(), count.cpu().numpy()


def device_hv(fronts, ref, K=None):
    from dkg_amd.boxes import hypervolume_front_device

    K = K or max(f.shape[0] for f in fronts)
    Y = np.tile(np.asarray(ref, dtype=np.float64), (len(fronts), K, 1))
    for s, f in enumerate(fronts):
        Y[s, : f.shape[0]] = f
    return hypervolume_front_device(torch.from_numpy(Y).to(DEV), list(ref)).cpu().numpy()


def same(got, count, fronts, ref):
    want, want_count = br.padded(fronts, ref, J=got.shape[2])
    assert count.tolist() == want_count.tolist()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("m,K", SHAPES)
def test_boxes_equal_the_restatement_bit_for_bit(m, K):
    for kind in br.KINDS:
        Y, ref = br.case(kind, K, m)
        got, count = device_boxes([Y], ref)
        same(got, count, [Y], ref)
        assert int(count[0]) <= br.count_bound(K, m)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_boxes_of_three_sets_of_unequal_valid_counts(m):
    for kinds, Ks in ((("cloud", "lattice", "front"), (65, 3, 257)), (("ref", "equal", "cloud"), (64, 257, 1))):
        ref = br.case(kinds[0], Ks[0], m)[1]
        fronts = [br.case(kind, K, m, seed=2)[0] for kind, K in zip(kinds, Ks)]
        got, count = device_boxes(fronts, ref)
        same(got, count, fronts, ref)


@pytest.mark.parametrize("which", ["lattice-n63", "sphere-2048"])
def test_large_sets(which):
    Y, ref = br.antichain(63) if which == "lattice-n63" else br.spherical_front(2048)
    got, count = device_boxes([Y], ref)
    same(got, count, [Y], ref)
    n = int(count[0])
    if which == "lattice-n63":
        assert Y.shape[0] == 2016 and n == 2016
    else:
        print(f"sphere-2048: {n} boxes")
        assert 3 * 2048 // 2 < n <= 4095
    lo, hi = got[0, 0, :n], got[0, 1, :n]
    assert (lo < hi).all()
    assert br.pairwise_disjoint(lo, hi)
    assert br.hi_dominated(Y, hi)
    assert not got[0, :, n:].any()


@pytest.mark.parametrize("maximize", [True, False])
def test_two_objective_boxes_equal_the_host_function(maximize):
    from dkg_amd import compute_sample_box_decomposition, dominated_boxes

    fronts = [torch.from_numpy(br.case(kind, K, 2, seed=1)[0])
              for kind, K in (("cloud", 14), ("front", 65), ("lattice", 257), ("equal", 3), ("cloud", 1))]
    want = compute_sample_box_decomposition(fronts, maximize=maximize)
    got = dominated_boxes(fronts, maximize=maximize, device=DEV)
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device
    assert got.numpy().tobytes() == want.numpy().tobytes()
    one = [f[:, :1] for f in fronts]
    assert dominated_boxes(one, device=DEV).numpy().tobytes() == compute_sample_box_decomposition(one).numpy().tobytes()
    f32 = dominated_boxes([f.float() for f in fronts], device=DEV)
    assert f32.dtype == torch.float32 and f32.shape == want.shape


# ---------------------------------------------------------------------------------------------- hypervolume

WORST = {"ratio": 0.0}


def check_hv(got, ref, K, what):
    """|got - ref| <= (L + 4) eps ref, the difference taken exactly; ref a Fraction or a float."""
    from fractions import Fraction

    bound = br.hv_bound(K, float(ref))
    err = float(abs(Fraction(float(got)) - Fraction(ref)))
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: |hv - ref| / bound = {ratio:.3g} (worst so far {WORST['ratio']:.3g})")
    assert err <= bound, (what, float(got), float(ref), err, bound)


@pytest.mark.parametrize("m,K", SHAPES)
def test_hypervolume_against_the_exact_sum_of_the_restatements_boxes(m, K):
    for kind in br.KINDS:
        Y, ref = br.case(kind, K, m)
        exact = br.volume_exact(*br.boxes(Y, ref))
        got = device_hv([Y], ref)[0]
        check_hv(got, exact, K, f"m={m} K={K} {kind}")
        if m >= 2 and K <= 32:  # dkg_hypervolume's own bound: 64 eps prod(ideal - ref)
            from dkg_amd.hvkg import hypervolume_device

            old = float(hypervolume_device(torch.from_numpy(Y[None]).to(DEV), list(ref))[0])
            q = br.qualifying(Y, ref)
            ideal = Y[q].max(0) if q else ref
            assert abs(old - float(got)) <= 64 * br.EPS * float(np.prod(ideal - ref)), (old, float(got))


def test_hypervolume_of_the_large_lattice_is_exact():
    Y, ref = br.antichain(180)
    assert Y.shape[0] == 16290
    assert device_hv([Y], ref)[0] == 988260.0 == float(math.comb(182, 3))


def test_hypervolume_of_large_sets_within_the_bound():
    Y, ref = br.antichain(180)
    scale = np.array([0.1 * math.pi, math.e, math.sqrt(2.0)])
    Ys, refs = Y * scale, ref * scale
    check_hv(device_hv([Ys], refs)[0], br.volume_fsum(*br.boxes(Ys, refs)), Ys.shape[0], "scaled lattice n=180")
    Y, ref = br.spherical_front(2048)
    check_hv(device_hv([Y], ref)[0], br.volume_fsum(*br.boxes(Y, ref)), 2048, "sphere-2048")


def test_bits():
    m, sets = 3, []
    for kind, K in (("cloud", 65), ("front", 257), ("lattice", 64)):
        sets.append(br.case(kind, K, m, seed=4)[0])
    ref = br.case("cloud", 65, m)[1]
    # two calls give the same bits
    b1, c1 = device_boxes(sets, ref)
    b2, c2 = device_boxes(sets, ref)
    h1, h2 = device_hv(sets, ref), device_hv(sets, ref)
    assert b1.tobytes() == b2.tobytes() and c1.tobytes() == c2.tobytes() and h1.tobytes() == h2.tobytes()
    # a set's result is the same whatever S is and whichever row holds it
    for s, Y in enumerate(sets):
        bs, cs = device_boxes([Y], ref, K=257)
        assert cs[0] == c1[s] and bs[0].tobytes() == b1[s].tobytes()
        assert device_hv([Y], ref, K=257)[0].tobytes() == h1[s].tobytes()
    b3, c3 = device_boxes(sets[::-1], ref)
    assert b3[::-1].tobytes() == b1.tobytes() and device_hv(sets[::-1], ref)[::-1].tobytes() == h1.tobytes()
    # appended rows that do not qualify change no bit (K = 257 -> 1300: another number of strided additions)
    below = [np.concatenate([Y, np.full((3, m), -7.0), np.full((2, m), np.nan)]) for Y in sets]
    assert device_hv(below, ref, K=1300).tobytes() == h1.tobytes()
    b4, c4 = device_boxes(below, ref, K=300)
    n = b1.shape[2]
    assert c4.tobytes() == c1.tobytes() and b4[:, :, :n].tobytes() == b1.tobytes() and not b4[:, :, n:].any()


# ---------------------------------------------------------------------------------------------- JES at m = 3

def test_jes_on_three_objectives_against_the_oracle_on_the_same_boxes():
    from dkg_amd import dominated_boxes
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    ref = jc.reference()  # the conditions on the inputs are asserted there, on the CPU
    state, sets, fronts, X = jc.problem()
    bounds = dominated_boxes(fronts, device=DEV)
    assert bounds.numpy().tobytes() == jc.bounds_of(fronts).numpy().tobytes()  # the boxes the reference used
    worst_v = worst_g = 0.0
    for (est, t), (acq_ref, g_ref, acq_slab) in ref.items():
        val, g = JES(state, sets, fronts, bounds, estimation_type=est, target_output_ix=t,
                     device=DEV).value_and_grad_host(X)
        tol = jc.value_tol(acq_ref)
        err, err_s = (val - acq_ref).abs(), (val - acq_slab).abs()
        gerr = (g - g_ref).abs().amax(-1)
        gtol = jc.RTOL * g_ref.abs().amax(-1) + 4 * jc.SPREAD_GRAD
        worst_v, worst_g = max(worst_v, float((err / tol).max())), max(worst_g, float((gerr / gtol).max()))
        print(f"{est} t={t}: |d acq| {float(err.max()):.3g}, on slabs {float(err_s.max()):.3g}, "
              f"|d g| {float(gerr.max()):.3g}")
        assert bool((err <= tol).all()), (est, t, float(err.max()))
        assert bool((err_s <= jc.value_tol(acq_slab)).all()), (est, t, float(err_s.max()))
        assert bool((gerr <= gtol).all()), (est, t, float(gerr.max()))
    print(f"JES m=3: worst value ratio {worst_v:.3g}, gradient ratio {worst_g:.3g}")


def test_spec_with_device_sampler_on_three_outputs():
    from dkg_amd.optim import JesOptimisationSpec

    state = jc.problem()[0]
    seen = []

    def oracle_factory(model, ps, pf, hb, est, target):
        seen.append(tuple(hb.shape))
        return jes_oracle.OracleJES(model, ps, pf, hb, est, target)

    out, full = [], []
    for factory in (None, oracle_factory):
        spec = JesOptimisationSpec.with_device_sampler("LB2", 3, 5, 2, 4, 1, 30, device=DEV, seed=3,
                                                       acq_factory=factory, num_rffs=64, nsga2_pop_size=24,
                                                       nsga2_generations=10)
        torch.manual_seed(11)
        out.append(spec.optimize_for_single_objective(state, [1.0, 2.0, 3.0], 2))
        torch.manual_seed(11)
        full.append(spec.optimize_for_full_evaluation(state, 2))
    assert seen and all(s[0] == 3 and s[1] == 2 and s[3] == 3 for s in seen)
    (xd, i_d, vd), (xo, i_o, vo) = out
    assert i_d == i_o
    assert bool(((xd - xo).abs() <= 1e-4).all()) and abs(float(vd - vo)) <= 1e-6 * abs(float(vo)) + 1e-8
    (xd, vd), (xo, vo) = full
    assert bool(((xd - xo).abs() <= 1e-4).all()) and abs(float(vd - vo)) <= 1e-6 * abs(float(vo)) + 1e-8


# ---------------------------------------------------------------------------------------------- metrics

@pytest.mark.parametrize("m", [2, 3])
def test_metrics_device_route_against_the_host_route(m):
    """Each key is a sum or a difference of volumes of at most prod(ideal - ref); each route rounds it within the
    hypervolume bound on that scale, so the two differ by at most twice that."""
    from dkg_amd.metrics import estimate_hypervolume_from_posterior_mean, hypervolume

    rng = np.random.default_rng(5)
    front = np.abs(rng.normal(size=(100, m))) + 1e-3
    front /= np.linalg.norm(front, axis=1, keepdims=True)
    pset = rng.uniform(size=(100, 2))
    ref = np.full(m, -0.1)

    def problem(x):
        x = torch.as_tensor(x)
        cols = [torch.sin(3.0 * x[:, 0] + i) * torch.cos(2.0 * x[:, 1] - i) for i in range(m)]
        return torch.stack(cols, dim=-1)

    host = estimate_hypervolume_from_posterior_mean(pset, front, problem, ref)
    dev = estimate_hypervolume_from_posterior_mean(pset, front, problem, ref, device=DEV)
    assert list(host) == list(dev)
    image = problem(torch.from_numpy(pset)).numpy()
    for key in host:
        pts = front if key.startswith("pfront") else image
        scale = float(np.prod(np.maximum(pts.max(0) - ref, 0.0)))
        tol = 2 * br.hv_bound(100, scale)
        print(f"m={m} {key}: host {host[key]:.17g} device {dev[key]:.17g} tol {tol:.3g}")
        assert abs(host[key] - dev[key]) <= tol, (key, host[key], dev[key])
    assert host["pfront_hv_lo"] > 0 and host["pset_hv_lo"] > 0
    assert hypervolume(front, ref, device=DEV) == dev["pfront_hv_lo"]


def test_smoke_run_with_device_metrics_makes_the_same_decisions():
    import os

    from dkg_amd.bo_smoke import GPProblem, run_smoke
    from dkg_amd.catalog import DataCatalog
    from helpers import load_golden

    hyper = dict(length_scales=[0.2, 1.8], output_scales=[1, 50], means=[0, 0])
    state, *_ = load_golden("lengthscales0")
    here = os.path.dirname(os.path.abspath(__file__))
    shared = DataCatalog.load_shared_gp_test_problem_data("lengthscales/0", data_dir=os.path.join(here, "golden"))

    def run(**kw):
        problem = GPProblem(state, device=DEV, ref_point=shared["ref_point"], max_hv=shared["max_hv"])
        return run_smoke(problem, hyper, seed=0, metrics=True, **kw)

    host, dev = run(), run(metrics_on_device=True)
    for mode in ("separate", "full"):
        assert dev[mode]["x"] == host[mode]["x"] and dev[mode]["obj_index"] == host[mode]["obj_index"]
        for a, b in zip(host[mode]["metrics_history"], dev[mode]["metrics_history"]):
            assert list(a) == list(b)
            for key in a:  # the four volumes to rounding (the bound is ~5e-14 of the ideal box), the rest to the bit
                tol = 1e-9 * max(abs(a[key]), 1.0) if key.endswith(("_hv_lo", "_hv_hi")) else 0.0
                assert abs(a[key] - b[key]) <= tol, (mode, key, a[key], b[key])
