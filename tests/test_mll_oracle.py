"""The yardstick of the marginal log-likelihood tests against a second, independent fp64 evaluation (no GPU):
per case of tests/mll_cases.py, the difference-form torch restatement's autograd against numpy with an explicit
L^{-1} and the W-contraction formulas the device evaluates (include/dkg.h, dkg_mll_value_grad).  This pins the
formulas without a GPU and measures the yardstick's own spread, from which the device tolerance is derived.

Measured: the worst spread is 3.3e-10 of max|g| (n = 1000, Matern-5/2, d = 2, noise 1e-4); among the cases up
to n = 272 it is 1.1e-10 (n = 130, Matern-5/2, d = 1, noise 1e-4); the values agree to 3.1e-12 relative.
mll_cases.CPU_SPREAD / CPU_VALUE_SPREAD record these; the test below asserts the bounds they were measured under
(gradient spread < 1e-9 of max|g|, value spread < 1e-11 relative)."""

import numpy as np
import pytest

import mll_cases as mc


def _spreads(name):
    v, g = mc.reference(name)
    v2, g2 = mc.numpy_reference(name)
    return ([np.abs(a - b).max() / np.abs(a).max() for a, b in zip(g, g2)],
            [abs(a - b) / abs(a) for a, b in zip(v, v2)])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_autograd_matches_the_w_contraction(name):
    sg, sv = _spreads(name)
    print(f"{name}: gradient spread {max(sg):.3e} of max|g|, value spread {max(sv):.3e} relative")
    assert max(sg) < 1e-9
    assert max(sv) < 1e-11


def test_device_tolerance_follows_from_the_spread():
    assert mc.TOL == min(100.0 * mc.CPU_SPREAD, 1e-8) and mc.TOL <= 1e-8
    assert mc.VALUE_TOL == min(100.0 * mc.CPU_VALUE_SPREAD, 1e-8)
    assert mc.FLOOR == 1e3 * mc.TOL


def test_case_matrix_covers_the_shapes():
    outs = [o for spec, _ in mc.CASES.values() for o in spec]
    assert {1, 15, 16, 17, 33, 100, 130, 272, 1000} <= {o["n"] for o in outs}
    assert {1, 2, 6, 16} <= {o["d"] for o in outs}
    for key, want in (("fam", set(mc.NU)), ("noise", {1e-4, 1e-2})):
        assert want <= {o[key] for o in outs}
    assert sum(o["n"] == 1000 for o in outs) == 1
    assert {o["fam"] for o in outs if o["dup"]} >= {"m12", "m52"}
    assert [o["n"] for o in mc.CASES["m3_mixed"][0]] == [17, 130, 64]
    assert len({o["fam"] for o in mc.CASES["m3_mixed"][0]}) == 3
    assert [o["n"] for o in mc.CASES["m8_n16"][0]] == [16] * 8
    assert mc.CASES["jitter_rbf"][1] == 1e-8
    assert all(o["mean"] != 0.0 for name in mc.CASES for o in mc.data(name))


def test_evaluation_points_sit_away_from_the_generating_hyperparameters():
    """10-30 % away in the lengthscales, the outputscale and the noise (the mean: a quarter of sqrt(outputscale))."""
    for name, (spec, _) in mc.CASES.items():
        for o, s in zip(mc.data(name), spec):
            d = s["d"]
            gen = np.array([(0.25 + 0.2 * (j % 3)) * np.sqrt(d) for j in range(d)])
            rel = np.abs(o["ls"].numpy() / gen - 1.0)
            assert rel.min() >= 0.1 - 1e-12 and rel.max() <= 0.3 + 1e-12
            assert o["os"] / s["os"] == pytest.approx(1.2)


def test_jitter_case_fails_without_jitter_and_is_well_conditioned_with_it():
    import torch

    (o,) = mc.data("jitter_rbf")
    n = o["X"].shape[0]
    K = o["os"] * mc.kernel_torch(o["X"], o["ls"], o["nu"]) + o["noise"] * torch.eye(n)
    assert float(torch.linalg.eigvalsh(K).min()) < -1e-9  # indefinite beyond any rounding
    assert int(torch.linalg.cholesky_ex(K).info) != 0
    ev = torch.linalg.eigvalsh(K + 1e-8 * torch.eye(n))
    assert float(ev.min()) > 0.5e-8 and float(ev.max() / ev.min()) < 1e5


def test_every_gradient_component_is_pinned_on_most_rows():
    """The mutation floor: a wrong factor anywhere moves a component by order 1 of itself, which the device test
    sees only where the component exceeds FLOOR x max|g|.  Per component (the mean, the smallest lengthscale
    entry, the outputscale, the noise) that holds on at least 90 % of the rows (one row per output of a case);
    the rows that miss are n = 1 (no lengthscale dependence), the jitter row, and the two noise-1e-4 rows whose
    noise derivative is ~1e5 times the others."""
    rows = []
    for name in mc.CASES:
        for g in mc.reference(name)[1]:
            a = np.abs(g) / np.abs(g).max()
            rows.append((a[0], a[1:-2].min(), a[-2], a[-1]))
    rows = np.array(rows)
    share = (rows > mc.FLOOR).mean(axis=0)
    print("rows", len(rows), "share above the floor (mean, lengthscales, outputscale, noise):", share)
    assert (share >= 0.9).all(), share
