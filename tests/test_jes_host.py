"""Joint entropy search without a device: the restatement against the reference's own entropy function
(tests/golden/jes_entropy.npz, written by tests/golden/make_jes_golden.py), the box decomposition against
hand-worked fronts, the constructor's validation and messages (joint_entropy_search.py:99-148), the C ABI's
argument checks (which return before any HIP call), and the committed cases' conditions."""

import ctypes
import os

import numpy as np
import pytest
import torch

import jes_cases
import jes_oracle
from dkg_amd import UnsupportedError, _lib, compute_sample_box_decomposition
from dkg_amd.jes import conditioned_states, qLowerBoundMultiObjectiveJointEntropySearch as JES
from dkg_amd.model import ModelListGPState, SingleTaskGPState
from dkg_amd.optim import JesOptimisationSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jes_entropy.npz")


# ---- the restatement against the reference's function ---------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("J", [1, 7, 70])
def test_restatement_matches_the_reference_entropy_bound(m, J):
    z = np.load(GOLDEN)
    key = f"m{m}_J{J}"
    bounds, mean, var, noise = (torch.from_numpy(z[f"{key}_{k}"]) for k in ("bounds", "mean", "variance", "noise"))
    assert bool((bounds[:, 0] == -1e10).any())                       # lower bounds at -1e10
    if J > 1:
        assert bool((bounds[1, :, (J + 1) // 2:] == 0).all())         # sample 1 is padded with [0, 0] boxes
    for est in ("LB", "LB2"):
        for t in jes_cases.targets_of(m):
            ref = torch.from_numpy(z[f"{key}_{est}_t{'all' if t is None else t}"])
            H, W = jes_oracle.entropy_bound(bounds, mean, var, noise, t, est == "LB2")
            assert float(W.min()) >= jes_cases.W_MIN                 # the condition on the inputs
            # two fp64 evaluations of one formula: the largest term of the moments is mu^2 + v <= 1, the
            # log's argument is >= 1e-3 of it on these inputs, so 1e-10 is ~1e3 roundings of room
            torch.testing.assert_close(H.mean(-1), ref, rtol=0, atol=1e-10)


# ---- the box decomposition ------------------------------------------------------------------------------------

def test_box_decomposition_one_objective():
    b = compute_sample_box_decomposition([torch.tensor([[0.3], [1.5], [0.7]]), torch.tensor([[-2.0]])])
    assert b.shape == (2, 2, 1, 1)
    assert b[:, 0].flatten().tolist() == [-1e10, -1e10] and b[:, 1].flatten().tolist() == [1.5, -2.0]


def test_box_decomposition_two_objectives_by_hand():
    # (2, 2) is dominated by (3, 3); the staircase of (1, 5), (3, 3), (4, 1) sorted by the first objective
    front = torch.tensor([[3.0, 3.0], [1.0, 5.0], [2.0, 2.0], [4.0, 1.0], [3.0, 3.0]])
    single = torch.tensor([[0.5, -0.5]])
    b = compute_sample_box_decomposition([front, single])
    assert b.shape == (2, 2, 3, 2)
    assert b[0, 0].tolist() == [[-1e10, -1e10], [1.0, -1e10], [3.0, -1e10]]
    assert b[0, 1].tolist() == [[1.0, 5.0], [3.0, 3.0], [4.0, 1.0]]
    # a single-point front: one box, then [0, 0] padding to the longest sample
    assert b[1, 0].tolist() == [[-1e10, -1e10], [0.0, 0.0], [0.0, 0.0]]
    assert b[1, 1].tolist() == [[0.5, -0.5], [0.0, 0.0], [0.0, 0.0]]
    # minimisation: the mirror image
    bm = compute_sample_box_decomposition([-front], maximize=False)
    assert torch.equal(bm[0, 0], -b[0, 1]) and torch.equal(bm[0, 1], -b[0, 0])


def test_box_decomposition_refuses_three_objectives():
    with pytest.raises(UnsupportedError, match="1 or 2 objectives"):
        compute_sample_box_decomposition([torch.rand(4, 3)])


# ---- constructor validation -----------------------------------------------------------------------------------

def small():
    state, sets, fronts, bounds, X = jes_cases.problem(jes_cases.OPT_CASE)
    return state, sets, fronts, bounds, X


def test_constructor_messages_are_the_references():
    state, sets, fronts, bounds, _ = small()
    with pytest.raises(ValueError, match="The number of Pareto fronts and Pareto sets should be equal"):
        JES(state, sets[:2], fronts, bounds, device="cpu")
    with pytest.raises(ValueError, match="The Pareto sets and fronts should have shapes of"):
        JES(state, [s[0] for s in sets], fronts, bounds, device="cpu")
    with pytest.raises(ValueError, match="Expected each pair of Pareto set and Pareto front to have the same"):
        JES(state, [sets[1], sets[1], sets[2]], fronts, bounds, device="cpu")
    with pytest.raises(UnsupportedError, match="The hypercell_bounds should have a shape of"):
        JES(state, sets, fronts, bounds[0], device="cpu")
    with pytest.raises(NotImplementedError, match='Currently the only supported estimation type are: "0", "LB", "LB2", "MC"'):
        JES(state, sets, fronts, bounds, estimation_type="LB3", device="cpu")
    with pytest.raises(UnsupportedError, match="Currently only estimation types 'LB' and 'LB2' are supported when"):
        JES(state, sets, fronts, bounds, estimation_type="0", target_output_ix=0, device="cpu")
    for est in ("0", "MC"):
        with pytest.raises(UnsupportedError, match='supported: "LB", "LB2"'):
            JES(state, sets, fronts, bounds, estimation_type=est, device="cpu")
    with pytest.raises(UnsupportedError, match="X_pending"):
        JES(state, sets, fronts, bounds, X_pending=torch.rand(1, 2), device="cpu")
    with pytest.raises(ValueError, match="Expected hypercell_bounds of shape 3 x 2 x num_boxes x 2"):
        JES(state, sets, fronts, bounds[:2], device="cpu")
    # everything valid: a device that is not a ROCm device is refused, not replaced by a CPU evaluation
    with pytest.raises(UnsupportedError, match="ROCm"):
        JES(state, sets, fronts, bounds, device="cpu")


def test_conditioned_states_append_the_standardised_front():
    state, sets, fronts, _, _ = small()
    cond = conditioned_states(state, sets, fronts)
    assert len(cond) == 3
    for p, c in enumerate(cond):
        for i, (o, n) in enumerate(zip(state.models, c.models)):
            k = sets[p].shape[0]
            assert n.num_train == o.num_train + k and (n.noise, n.outputscale, n.y_mean, n.y_std) == (
                o.noise, o.outputscale, o.y_mean, o.y_std)
            assert torch.equal(n.train_x[-k:], sets[p]) and torch.equal(n.train_x[:-k], o.train_x)
            assert torch.equal(n.train_y[-k:], (fronts[p][:, i] - o.y_mean) / o.y_std)


def test_spec_needs_a_sampler_and_keeps_the_references_rule():
    with pytest.raises(TypeError):
        JesOptimisationSpec("LB", 10, 10, 10, 512, 50, 200, pareto_sampler=None)
    spec = JesOptimisationSpec("LB", 10, 10, 10, 512, 50, 200, pareto_sampler=lambda *a, **k: None)
    x = torch.zeros(1, 2)
    # negative values are clipped to 0 and ties go to the cheaper objective; else value per cost
    assert spec._choose_best_objective([(0, x, torch.tensor(-1.0)), (1, x, torch.tensor(-2.0))], [2.0, 1.0])[0] == 1
    i, _, v = spec._choose_best_objective([(0, x, torch.tensor(3.0)), (1, x, torch.tensor(2.0))], [2.0, 1.0])
    assert i == 1 and float(v) == 2.0


# ---- the C ABI's argument checks (no HIP call is reached) -----------------------------------------------------

def _states(count, n=8):
    arr = (_lib.DkgOutput * count)()
    for o in arr:
        o.n, o.kernel, o.outputscale, o.noise, o.y_std = n, 2, 1.0, 1e-2, 1.0
        o.inv_lengthscale = o.train_x = o.alpha = o.root_frag = 64   # never followed by the checks
    return arr


def _init(lib, states, m=2, P=3, d=2, bounds=64, J=4, target=-1, diag=0, max_B=16, ws=64, ws_bytes=1 << 30, plan="own"):
    if plan == "own":
        plan = ctypes.create_string_buffer(lib.dkg_jes_plan_bytes())
    return lib.dkg_jes_init(states, m, P, d, bounds, J, target, diag, max_B, ws, ws_bytes, plan, None)


def test_abi_version_is_still_9():
    assert _lib.load().dkg_abi_version() == 9 == _lib.ABI_VERSION


def test_jes_init_argument_checks():
    lib = _lib.load()
    st = _states(8)
    assert _init(lib, None) == _lib.DKG_ERR_ARG
    assert _init(lib, st, bounds=None) == _lib.DKG_ERR_ARG
    assert _init(lib, st, ws=None) == _lib.DKG_ERR_ARG
    assert _init(lib, st, plan=None) == _lib.DKG_ERR_ARG
    for kw in (dict(m=0), dict(P=0), dict(d=0), dict(J=0), dict(max_B=0), dict(target=2), dict(target=-2)):
        assert _init(lib, st, **kw) == _lib.DKG_ERR_ARG, kw
    assert b"target=2" in lib.dkg_last_error() or b"target=-2" in lib.dkg_last_error()
    big = _states((_lib.DKG_JES_MAX_SAMPLES + 2) * 9)
    for kw in (dict(m=9), dict(d=17), dict(P=_lib.DKG_JES_MAX_SAMPLES + 1), dict(J=_lib.DKG_JES_MAX_BOXES + 1),
               dict(max_B=_lib.DKG_JES_MAX_CANDIDATES + 1)):
        assert _init(lib, big, **kw) == _lib.DKG_ERR_UNSUPPORTED, kw
    assert _init(lib, _states(8, n=1025)) == _lib.DKG_ERR_UNSUPPORTED
    assert _init(lib, _states(8, n=0)) == _lib.DKG_ERR_ARG
    null = _states(8)
    null[5].root_frag = None
    assert _init(lib, null) == _lib.DKG_ERR_ARG and b"state 2 output 1" in lib.dkg_last_error()
    need = lib.dkg_jes_workspace(2, 3, 2, 4, 16)
    assert need > 0 and _init(lib, st, ws_bytes=need - 1) == _lib.DKG_ERR_WORKSPACE
    assert lib.dkg_jes_workspace(9, 3, 2, 4, 16) == 0 and lib.dkg_jes_workspace(2, 0, 2, 4, 16) == 0
    assert lib.dkg_jes_workspace(2, 3, 2, 4, 32) > need                 # grows with the candidates


def test_jes_forward_argument_checks():
    lib = _lib.load()
    plan = ctypes.create_string_buffer(lib.dkg_jes_plan_bytes())
    assert lib.dkg_jes_forward(None, 64, 1, 64, None, None, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_jes_forward(plan, None, 1, 64, None, None, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_jes_forward(plan, 64, 1, None, None, None, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_jes_forward(plan, 64, 1, 64, None, None, None) == _lib.DKG_ERR_ARG   # never initialised
    assert b"not initialised" in lib.dkg_last_error()


# ---- the committed cases --------------------------------------------------------------------------------------

def test_cases_cover_the_shapes_and_meet_the_condition():
    cs = jes_cases.CASES.values()
    assert {c["m"] for c in cs} == {1, 2, 3, 8} and {c["d"] for c in cs} == {1, 2, 6}
    assert {c["J"] for c in cs} == {1, 6, 70} and {len(c["ks"]) for c in cs} == {1, 3}
    assert {k for c in cs for k in c["ks"]} == {1, 3, 5} and {c["B"] for c in cs} == {17, 40}
    assert {c["noise"] for c in cs} == {1e-8, 1e-2} and {c["std"] for c in cs} == {True, False}
    assert {f for c in cs for f in c["fam"]} == {"M12", "M32", "M52", "RBF"}
    for cid, c in jes_cases.CASES.items():
        state, sets, fronts, bounds, X = jes_cases.problem(cid)
        assert all(o.num_train % 16 for o in state.models)
        # Matern-1/2 outputs stay on torch.cdist's exact path in the oracle (jes_oracle.CHUNK)
        assert all(o.num_train + max(c["ks"]) + 1 <= 25 for o in state.models if (o.kernel, o.nu) == ("matern", 0.5))
        assert torch.equal(X[0], sets[0][0]) and torch.equal(X[1], state.models[0].train_x[3])
        assert bool((bounds[:, 0] == -1e10).any())
        if len(sets) > 1:
            assert bool((bounds[1:, :, -1] == 0).all())                 # the shorter samples are padded
        jes_cases.reference(cid)                                         # asserts W >= 1e-3 for every estimator


def _tiles(cid, conditioned=True):
    """The column-tile counts pad16(rows) // 16 of the case's state-outputs: the conditioned ones, or state 0's."""
    ns = [o.num_train for o in jes_cases.problem(cid)[0].models]
    ks = jes_cases.SHAPE_CASES[cid]["ks"] if conditioned else (0,)
    return {(n + k + 15) // 16 for n in ns for k in ks}


def test_shape_cases_reach_the_loops_they_promise():
    sc = jes_cases.SHAPE_CASES
    cs = sc.values()
    assert not set(sc) & (set(jes_cases.CASES) | set(jes_cases.EXTRA_CASES))
    assert {c["m"] for c in cs} == {1, 2, 4, 5, 7} and {c["d"] for c in cs} == {1, 2, 3, 4, 8, 9, 16}
    assert {c["J"] for c in cs} == {1, 6, 64, 65, 129, _lib.DKG_JES_MAX_BOXES}
    assert {len(c["ks"]) for c in cs} == {1, 3, 4, 7, 9, _lib.DKG_JES_MAX_SAMPLES} and {c["B"] for c in cs} == {2, 5, 16, 17}
    assert all(c["noise"] == 1e-2 and c["std"] for c in cs)
    # the moments stage's column tiles: 8 | 9 (s = 1 on wave 7 alone), 16 and 17 (s = 2 on wave 0 alone), 64 (all)
    assert _tiles("n127-P4-d3", False) == {8} and _tiles("n127-P4-d3") == {9}
    assert _tiles("n253-P7-d4") == {16, 17, 9}
    assert _tiles("n1019-k5") == {64} and _tiles("n1019-k5", False) == {64}
    c = sc["n253-P7-d4"]
    assert 144 in {n + k for n in c["ns"] for k in c["ks"]}                # a conditioned output with no padded row


@pytest.mark.parametrize("cid", list(jes_cases.SHAPE_CASES))
def test_shape_case_meets_the_condition_and_sets_no_bound(cid):
    import test_gpu_jes as t

    c = jes_cases.SHAPE_CASES[cid]
    state, sets, fronts, bounds, X = jes_cases.problem(cid)
    assert [o.num_train for o in state.models] == list(c["ns"]) and bounds.shape[0] == len(c["ks"])
    assert bounds.shape[2] == (2 if c.get("overlap") else 1) * c["J"] and X.shape == (c["B"], c["d"])
    # Matern-1/2 outputs stay on torch.cdist's exact path in the oracle (jes_oracle.CHUNK)
    assert all(o.num_train + max(c["ks"]) + 1 <= 25 for o in state.models if (o.kernel, o.nu) == ("matern", 0.5))
    assert torch.equal(X[0], sets[0][0]) and torch.equal(X[1], state.models[0].train_x[3])
    ref = jes_cases.reference(cid)                                   # asserts W >= 1e-3 for every estimator
    # no shape case sets the bounds of test_gpu_jes.py
    sv, sg = jes_cases.spreads(cid)
    print(f"{cid}: reference-side spread: value {sv:.3g}, gradient {sg:.3g}")
    assert sv <= t.SPREAD_VALUE and sg <= t.SPREAD_GRAD, (cid, sv, sg)
    _, Wsum = jes_oracle.acq_from_moments(bounds, *ref["moments"], None, False, return_w=True)
    if c.get("overlap"):                                             # both arms of W = min(sum_j W_j, 1)
        assert bool((Wsum > 1.0).any()) and bool((Wsum < 1.0).any())
        assert int((Wsum > 1.0 + 1e-9).sum()) >= 5 and int((Wsum < 1.0 - 1e-9).sum()) >= 5


def test_recorded_spreads_cover_a_fresh_measurement():
    import test_gpu_jes as t

    sv = sg = 0.0
    for cid in jes_cases.CASES:
        a, b = jes_cases.spreads(cid)
        sv, sg = max(sv, a), max(sg, b)
    print(f"reference-side spread: value {sv:.3g}, gradient {sg:.3g}")
    # rounding noise: another BLAS or thread count moves it by a small factor, not by an order of magnitude
    assert sv / 5 <= t.SPREAD_VALUE <= 5 * sv and sg / 5 <= t.SPREAD_GRAD <= 5 * sg
