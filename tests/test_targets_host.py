"""The host side of the plans of several targets: the argument checks of dkg_plan_init_targets and
dkg_plan_workspace_targets (they come before any HIP call, so they need no GPU: with the fake device pointers
used here a HIP call would fail with DKG_ERR_HIP, not the status asserted), the Python target normalisation of
DiscreteKnowledgeGradient.forward_targets, and the decision logic of optimize_for_single_objective(joint=True)
on stub acquisitions with analytic per-target values."""

import ctypes
import os

import pytest
import torch

from dkg_amd import _lib, normalise_targets
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from dkg_amd.optim import DiscreteKgOptimisationSpec, JointDecoupledAcquisition, joint_best_per_cost


def fake_outputs(m, n=40):
    outs = (_lib.DkgOutput * m)()
    for o in outs:
        o.n = n
        o.kernel = 2
        o.outputscale, o.noise, o.y_std = 1.0, 1e-3, 1.0
        # never dereferenced: the checks come first
        o.inv_lengthscale = o.train_x = o.alpha = o.root_frag = o.disc_frag = o.disc_mean = 64
    return outs


def init_targets(lib, m, targets, T=None, flags=0, N=100, S=8, max_B=19):
    outs = fake_outputs(m)
    tl = (ctypes.c_int * max(len(targets), 1))(*targets)
    host = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    return lib.dkg_plan_init_targets(outs, m, 3, 64, N, 64, S, tl, len(targets) if T is None else T, max_B, flags,
                                     64, 1 << 40, host, 64, None)


def test_abi_version_is_9():
    assert _lib.ABI_VERSION == 9 and _lib.load().dkg_abi_version() == 9


@pytest.mark.parametrize("targets,T,word", [
    ((0,), 0, b"T=0"),                    # no target
    ((-1, 0, 1, 0), None, b"T=4"),        # m + 2 targets
    ((0, 1, 0), None, b"repeats"),        # a duplicate
    ((-1, -1), None, b"repeats"),
    ((0, 2), None, b"targets[1]=2"),      # an entry = m
    ((-2,), None, b"targets[0]=-2"),      # an entry < -1
])
def test_bad_targets_are_argument_errors_before_any_device_call(targets, T, word):
    lib = _lib.load()
    assert init_targets(lib, 2, targets, T) == _lib.DKG_ERR_ARG
    msg = lib.dkg_last_error()
    assert word in msg and (b"targets" in msg or b"T=" in msg), msg


def test_null_targets_and_plan_pointers():
    lib = _lib.load()
    outs = fake_outputs(2)
    host = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    args = (outs, 2, 3, 64, 100, 64, 8)
    assert lib.dkg_plan_init_targets(*args, None, 1, 19, 0, 64, 1 << 40, host, 64, None) == _lib.DKG_ERR_ARG
    assert b"targets" in lib.dkg_last_error()
    tl = (ctypes.c_int * 1)(0)
    assert lib.dkg_plan_init_targets(*args, tl, 1, 19, 0, 64, 1 << 40, None, 64, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_plan_init_targets(*args, tl, 1, 19, 0, 64, 1 << 40, host, None, None) == _lib.DKG_ERR_ARG


def test_fused_plans_take_one_target():
    lib = _lib.load()
    assert init_targets(lib, 2, (-1, 0), flags=_lib.DKG_PLAN_FUSED) == _lib.DKG_ERR_UNSUPPORTED
    assert b"DKG_PLAN_FUSED" in lib.dkg_last_error()
    # the checks of the single-target entry still come first: too small a workspace is reported as such
    outs = fake_outputs(2)
    tl = (ctypes.c_int * 2)(-1, 0)
    host = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    assert lib.dkg_plan_init_targets(outs, 2, 3, 64, 100, 64, 8, tl, 2, 19, 0, 64, 8, host, 64,
                                     None) == _lib.DKG_ERR_WORKSPACE


@pytest.mark.parametrize("flags", [0, _lib.DKG_PLAN_GRAD, _lib.DKG_PLAN_F32])
@pytest.mark.parametrize("S", [8, 12, 24])
def test_workspace_of_one_target_is_the_single_target_workspace(flags, S):
    lib = _lib.load()
    m, d, N, B = 3, 3, 150, 19
    outs = fake_outputs(m)
    single = lib.dkg_plan_workspace(outs, m, d, N, B, S, flags)
    sizes = [lib.dkg_plan_workspace_targets(outs, m, d, N, B, S, T, flags) for T in range(1, m + 2)]
    assert single > 0 and sizes[0] == single
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # T outside 1 .. m + 1: no such plan
    assert lib.dkg_plan_workspace_targets(outs, m, d, N, B, S, 0, flags) == 0
    assert lib.dkg_plan_workspace_targets(outs, m, d, N, B, S, m + 2, flags) == 0


def test_signatures_cover_the_new_entries():
    assert "dkg_plan_init_targets" in _lib.SIGNATURES and "dkg_plan_workspace_targets" in _lib.SIGNATURES
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "dkg.h")) as f:
        header = f.read()
    assert "dkg_plan_init_targets(" in header and "dkg_plan_workspace_targets(" in header
    assert "#define DKG_ABI_VERSION 9" in header


# --------------------------------------------------------------------------------------------------
# Python: the targets of forward_targets

def test_default_targets_are_all_outputs_then_each_output():
    assert normalise_targets(None, 3) == (None, 0, 1, 2)
    assert normalise_targets(None, 1) == (None, 0)


def test_negative_targets_count_from_the_end():
    assert normalise_targets([-1, None, 0], 3) == (2, None, 0)
    assert normalise_targets([-3], 3) == (0,)
    assert normalise_targets((1,), 2) == (1,)


def test_duplicates_after_normalisation_raise_value_error():
    with pytest.raises(ValueError):
        normalise_targets([1, -1], 2)
    with pytest.raises(ValueError):
        normalise_targets([None, 0, None], 2)
    with pytest.raises(ValueError):
        normalise_targets([], 2)


def test_out_of_range_targets_raise_index_error():
    for bad in ([2], [0, -3], [None, 5]):
        with pytest.raises(IndexError):
            normalise_targets(bad, 2)


# --------------------------------------------------------------------------------------------------
# joint=True: max_t max(KG_t, 0) / cost_t on stub acquisitions

def test_joint_best_per_cost_rule():
    kg = torch.tensor([[0.2, -0.5, 0.1, 0.3],
                       [0.1, -0.1, 0.3, 0.3]], dtype=torch.double)
    best, win = joint_best_per_cost(kg, [2.0, 1.0])
    # 0.2 / 2 = 0.1 / 1: the cheaper objective; both negative: 0, the cheaper objective; then plain maxima
    assert win.tolist() == [1, 1, 1, 1]
    torch.testing.assert_close(best, torch.tensor([0.1, 0.0, 0.3, 0.3], dtype=torch.double), rtol=0, atol=0)
    best, win = joint_best_per_cost(kg, [1.0, 2.0])
    assert win.tolist() == [0, 0, 1, 0]
    torch.testing.assert_close(best, torch.tensor([0.2, 0.0, 0.15, 0.3], dtype=torch.double), rtol=0, atol=0)
    # equal costs and equal values: the lower index, as max() over the reference's candidate list
    assert joint_best_per_cost(torch.tensor([[0.3], [0.3]]), [1.0, 1.0])[1].tolist() == [0]
    with pytest.raises(ValueError):
        joint_best_per_cost(kg, [1.0])


class Bump:
    """KG_t(x) = height - scale |x - centre|^2: an analytic acquisition for [*batch, 1, d] -> [*batch]."""

    def __init__(self, centre, height, scale=1.0):
        self.c = torch.as_tensor(centre, dtype=torch.double)
        self.h, self.s = float(height), float(scale)

    def __call__(self, X):
        return self.h - self.s * ((X.squeeze(-2) - self.c) ** 2).sum(-1)


def two_output_model():
    x = torch.rand(5, 2, dtype=torch.double, generator=torch.Generator().manual_seed(0))
    return ModelListGPState(SingleTaskGPState(x, x.sum(-1), 0.5, 1.0, 1e-3, 0.0),
                            SingleTaskGPState(x, x[:, 0], 0.5, 1.0, 1e-3, 0.0))


def stub_spec(bumps, seen=None):
    def factory(model, disc, W, target):
        if seen is not None:
            seen.append((tuple(disc.shape), target))
        return bumps[target]

    return DiscreteKgOptimisationSpec(3, 4, 16, 4, 100, seed=0, acq_factory=factory)


def test_joint_acquisition_value_and_gradient_are_the_winners():
    bumps = [Bump([0.2, 0.2], 0.5), Bump([0.8, 0.8], 0.9)]
    acq = JointDecoupledAcquisition(bumps, [1.0, 3.0], 2)
    assert not hasattr(acq, "value_and_grad_host")  # stubs without the multi-target entries: autograd
    X = torch.tensor([[[0.2, 0.25]], [[0.8, 0.7]], [[0.2, 1.0]]], dtype=torch.double, requires_grad=True)
    A = acq(X)
    kg = acq.per_target(X.detach())
    torch.testing.assert_close(A.detach(), torch.maximum(kg[0].clamp_min(0) / 1.0, kg[1].clamp_min(0) / 3.0))
    (g,) = torch.autograd.grad(A.sum(), X)
    # candidate 0: objective 0 wins, d/dx (0.5 - |x - c0|^2); candidate 1: objective 1, scaled by 1 / 3;
    # candidate 2: KG_0 = 0.5 - 0.64 clips to 0, objective 1 (0.5 / 3) wins
    assert joint_best_per_cost(kg, [1.0, 3.0])[1].tolist() == [0, 1, 1]
    torch.testing.assert_close(g[0, 0], -2 * (X[0, 0].detach() - bumps[0].c))
    torch.testing.assert_close(g[1, 0], -2 * (X[1, 0].detach() - bumps[1].c) / 3.0)
    far = torch.tensor([[[0.2, 1.9]]], dtype=torch.double, requires_grad=True)  # both negative: A = 0, flat
    assert float(acq(far).detach()) == 0.0
    (gf,) = torch.autograd.grad(acq(far).sum(), far)
    assert float(gf.abs().max()) == 0.0


def test_joint_search_returns_the_best_objectives_best_point_per_cost():
    seen = []
    bumps = [Bump([0.2, 0.3], 0.5), Bump([0.7, 0.6], 0.9)]
    spec = stub_spec(bumps, seen)
    model = two_output_model()
    W = torch.tensor([[0.5, 0.5]], dtype=torch.double)
    # costs (1, 3): 0.5 / 1 > 0.9 / 3 -> objective 0 at its centre
    x, i, v = spec.optimize_for_single_objective(model, [1.0, 3.0], 2, scalarisation_weights=W, joint=True)
    assert i == 0 and x.shape == (1, 2)
    torch.testing.assert_close(x, torch.tensor([[0.2, 0.3]], dtype=torch.double), atol=1e-5, rtol=0)
    assert float(v) == pytest.approx(0.5, abs=1e-9)
    assert seen == [((9, 2), 0), ((9, 2), 1)]  # one acquisition per objective from the factory, combined
    # costs (1, 1.5): 0.9 / 1.5 = 0.6 > 0.5 -> objective 1; the value is KG_1(x) / cost_1
    x, i, v = spec.optimize_for_single_objective(model, [1.0, 1.5], 2, scalarisation_weights=W, joint=True)
    assert i == 1
    torch.testing.assert_close(x, torch.tensor([[0.7, 0.6]], dtype=torch.double), atol=1e-5, rtol=0)
    assert float(v) == pytest.approx(0.6, abs=1e-9)
    # the same decision as the per-objective search
    x2, i2, v2 = spec.optimize_for_single_objective(model, [1.0, 1.5], 2, scalarisation_weights=W)
    assert i2 == 1 and float(v2) == pytest.approx(float(v), abs=1e-9)
    torch.testing.assert_close(x2, x, atol=1e-5, rtol=0)


def test_joint_search_ties_go_to_the_cheaper_objective_and_negatives_clip():
    model = two_output_model()
    W = torch.tensor([[0.5, 0.5]], dtype=torch.double)
    # KG_b = 2 KG_a exactly (doubling commutes with rounding) at twice the cost: equal value per cost at every
    # x, so wherever the search stops the tie goes to the cheaper objective
    a, b = Bump([0.5, 0.5], 0.4), Bump([0.5, 0.5], 0.8, scale=2.0)
    x, i, v = stub_spec([a, b]).optimize_for_single_objective(model, [1.0, 2.0], 2, scalarisation_weights=W,
                                                              joint=True)
    assert i == 0 and float(v) == pytest.approx(0.4, abs=1e-9)
    x, i, v = stub_spec([b, a]).optimize_for_single_objective(model, [2.0, 1.0], 2, scalarisation_weights=W,
                                                              joint=True)
    assert i == 1 and float(v) == pytest.approx(0.4, abs=1e-9)
    # every KG negative everywhere: A = 0 for all x, the cheaper objective, its (unclipped) value per cost
    spec = stub_spec([Bump([0.5, 0.5], -1.0), Bump([0.5, 0.5], -2.0)])
    with pytest.warns(RuntimeWarning):  # constant raw-sample values: initial conditions chosen at random
        x, i, v = spec.optimize_for_single_objective(model, [1.0, 4.0], 2, scalarisation_weights=W, joint=True)
    assert i == 0 and float(v) < 0
    assert float(v) == pytest.approx(float(Bump([0.5, 0.5], -1.0)(x.unsqueeze(0))), rel=1e-12)


def test_joint_false_is_the_per_objective_search():
    seen = []
    spec = stub_spec([Bump([0.2, 0.3], 0.5), Bump([0.7, 0.6], 0.9)], seen)
    W = torch.tensor([[0.5, 0.5]], dtype=torch.double)
    torch.manual_seed(5)  # (the Boltzmann draw of the initial conditions reads the global generator)
    a = spec.optimize_for_single_objective(two_output_model(), [1.0, 3.0], 2, scalarisation_weights=W)
    torch.manual_seed(5)
    b = spec.optimize_for_single_objective(two_output_model(), [1.0, 3.0], 2, scalarisation_weights=W, joint=False)
    assert a[1] == b[1] == 0 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
