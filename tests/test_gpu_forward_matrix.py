"""The production forward envelope (ForwardPlan.forward without kg_pairs: the kernel bench.py measures) against
the oracle in every output bucket and envelope instantiation (needs a real MI355X).

With kg_pairs the envelope walks every pair (env_extremes); without it, it first tries to settle the pair without
a walk (env_flat), takes T from the plan's top hint (Plan::itop / itopk, computed at plan init by
intercepts_kernel) where that decides it, and otherwise runs env_top + env_span.  The parity tests elsewhere pass
kg_pairs, so this file holds the other path to the same references:

  1. helpers.FORWARD_MATRIX: every (M, geometry) cell, production KG against the batched oracle at the stated
     tolerance, helpers.parity_case on the same inputs (lines, envelope on identical lines, KG), production KG
     against the mean of the walked pairs, and exact zeros where helpers.forward_classes calls a pair flat;
  2. the plans' envelopes are the reference walk, in the 33-slot and streaming kernels of M = 1, 4, 8;
  3. the states of the top hint no matrix row reaches (helpers.hint_case): line 0 on top, a tied top grid
     intercept, a0 == A1;
  4. the intercept cache: the argmax grid line moved across lanes and slots by permuting D; the hinted KG is
     the bits of the walked one in every plan, and the same bits across them;
  5. the streaming forward's staged chain against its overflow path at small shapes (M = 2, 3, 4);
  6. streaming forwards over lists longer than LIST_CAP_STREAM = 512.

(1) found a bug at M4-S40, target 3: a pair whose top line also has the smallest slope and whose first filter
leaves more than ENV_CAP lines lost its top line in the second filter and came out as KG = 0 (both paths);
test_top_line_at_the_end_of_the_slope_range_in_an_overflowing_list holds the case on its own.  (4) and (5) found
that the successor-table walk (dkg_walk.h walk_table) summed a pair's edge terms in the order of the survivor
list, so KG moved by an ulp with the order of D's rows and with the filter that built the list; the table now
leaves each edge on the lane of its walk step, as the step-by-step walks do, and both checks are bit for bit.

Tolerances are the project's stated ones, unchanged (helpers.stated_tol, LINE_RTOL, check_parity_case); which
inputs reach which branch is asserted on the oracle alone in tests/test_forward_matrix_oracle.py.  With
DKG_FORWARD_MATRIX_REPORT=<path> the worst err/tol per case of (1) is written there as JSON
(profiles/forward_matrix/parity.json)."""

import functools
import json
import os

import pytest
import torch

from dkg_amd.gp_state import DeviceGPState
from helpers import (EPS, FORWARD_CASES, FORWARD_LONG, FORWARD_LONG_ROWS, FORWARD_MATRIX, FORWARD_ROWS, HINT_KINDS,
                     HINT_NS, HINT_STATES, LINE_RTOL, assert_envelopes_are_reference_walk, assert_within, check_parity_case,
                     forward_classes, forward_row_problem, hint_case, parity_case, stated_tol, to_oracle)
from oracle.discretekg import discrete_kg_batched, lines_batched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("DKG_FORWARD_MATRIX_REPORT")
    if out and _REPORT:
        worst = {k: max(c[k] for c in _REPORT.values())
                 for k in ("line_rel_a", "line_rel_b", "envelope_ratio", "kg_ratio_stated_only", "production_kg_ratio")}
        with open(out, "w") as f:
            json.dump({"line_rtol": LINE_RTOL, "cases": _REPORT, "worst": worst}, f, indent=1)


@functools.lru_cache(maxsize=None)
def _problem(row_id, B=None):
    row = FORWARD_ROWS.get(row_id) or FORWARD_LONG_ROWS[row_id]
    return forward_row_problem(row, B)


@functools.lru_cache(maxsize=None)
def _device_state(row_id):
    state, D, _, _ = _problem(row_id)
    return DeviceGPState(state, D, device=DEV)


def _assert_geometry(plan, row):
    geo = plan.envelope_geometry()
    assert geo["stream"] == row["stream"] and geo["slots"] == row["slots"] and geo["split"] == row["split"], (
        f"{row['id']}: envelope {geo}, expected slots {row['slots']} stream {row['stream']} split {row['split']}")
    assert geo["sw"] == min(8, row["S"])


def _assert_mean_of_pairs(kg, pairs):
    """The production KG is the mean of the walked pairs: the bound of test_headline_pairs_and_mean (the pair
    values are >= 0, so two summation orders of S <= 40 of them differ by at most (S + 1) eps < 1e-14 relative)."""
    torch.testing.assert_close(kg.cpu(), pairs.cpu().mean(-1), rtol=1e-14, atol=1e-300)


# ---------------------------------------------------------------- 1. every (M, geometry) cell
@pytest.mark.parametrize("row_id,target", FORWARD_CASES, ids=[f"{r}-t{t}" for r, t in FORWARD_CASES])
def test_forward_matrix_vs_oracle(row_id, target):
    row = FORWARD_ROWS[row_id]
    state, D, W, X = _problem(row_id)
    plan = _device_state(row_id).plan(W, target, X.shape[0])  # the forward plan, not the gradient plan
    _assert_geometry(plan, row)
    kg = plan.forward(X.to(DEV)).cpu()                        # production: no kg_pairs
    res = parity_case(state, D, W, X, target, DEV)
    check_parity_case(res)
    # parity_case's reference is discrete_kg_batched's (lines_batched, the reference walk per pair, the mean)
    # and its tolerance stated_tol on the oracle's max |a|: computed once, shared with the production value
    kg_walked, kg_ref, tol_kg, pairs, _, _ = res["_tensors"]
    ratio = assert_within(kg, kg_ref, tol_kg, f"{row_id} target={target}: production KG (stated tolerance)")
    _assert_mean_of_pairs(kg, pairs)
    # the two paths differ only in how they find T and in not walking flat pairs (exact zeros either way)
    assert torch.equal(kg, kg_walked), "production KG differs in bits from the KG of the walked (kg_pairs) path"
    a, b = lines_batched(to_oracle(state), X, D, W, target)
    flat = forward_classes(a, b, torch.ones(a.shape[:2]))["flat"]
    assert bool((pairs[flat] == 0.0).all()), f"{int((pairs[flat] != 0).sum())} flat pairs walked to KG != 0"
    assert bool((kg[flat.all(-1)] == 0.0).all()), "a candidate whose pairs are all flat has production KG != 0"
    print(f"{row_id} target={target}: production KG worst err/tol {ratio:.3g}; {int(flat.sum())} flat pairs, "
          f"{int(flat.all(-1).sum())} all-flat candidates")
    _REPORT[f"{row_id}-t{target}"] = {**{k: v for k, v in res.items() if not k.startswith("_")},
                                      "cell": list(row["cell"]), "production_kg_ratio": ratio,
                                      "flat_pairs": int(flat.sum())}


# ---------------------------------------------------------------- 2. the envelopes are the reference walk
WALK_ROWS = [r["id"] for r in FORWARD_MATRIX
             if r["cell"][0] in ("M1", "M4", "M8p", "M8f") and r["cell"][1] in ("slots33", "stream")]


@pytest.mark.parametrize("row_id", WALK_ROWS)
def test_forward_envelopes_are_the_reference_walk_per_bucket(row_id):
    """test_gpu_epigraph.py's test_forward_envelopes_are_the_reference_walk on the plans of the 33-slot and
    streaming rows of M = 1, 4, 8 (4 candidates, the last target): hull sizes, indices and intersections are
    ref_epigraph's on the plan's own exported lines."""
    row = FORWARD_ROWS[row_id]
    _, _, W, X = _problem(row_id)
    plan = _device_state(row_id).plan(W, row["targets"][-1], 4)
    Xd = X[:4].to(DEV)
    _, _, hull = plan.forward_stats(Xd)
    a, b = plan.lines(Xd)
    sizes = assert_envelopes_are_reference_walk(a, b, hull)
    print(f"{row_id}: envelopes of {sizes[0]}..{sizes[-1]} lines")


# ---------------------------------------------------------------- 3. the states of the top hint
@functools.lru_cache(maxsize=None)
def _hint_problem(mk, slots, kind):
    state, D, W, X = hint_case(mk, slots, kind)
    return state, to_oracle(state), D, W, X, DeviceGPState(state, D, device=DEV)


@pytest.mark.parametrize("kind", HINT_KINDS)
@pytest.mark.parametrize("slots", [2, 8, 17])
@pytest.mark.parametrize("mk", list(HINT_NS))
def test_top_hint_states(mk, slots, kind):
    """line0: a0 > A1 in some pairs; tied: the top grid intercept attained twice (no hint: env_top); equal /
    equal-tied: candidates on the argmax rows of D, a0 == A1 (no hint), D undoubled and doubled.  Under targets
    (None, m - 1): production KG at the stated tolerance of the batched oracle, equal to the mean of the walked
    pairs, and the bits of a plan of both targets."""
    state, om, D, W, X, dstate = _hint_problem(mk, slots, kind)
    m = len(HINT_NS[mk])
    Xd = X.to(DEV)
    assert dstate.plan(W, None, X.shape[0]).envelope_geometry()["slots"] == slots
    both = dstate.plan(W, None, X.shape[0], targets=(None, m - 1)).forward(Xd)
    for tau, target in enumerate((None, m - 1)):
        plan = dstate.plan(W, target, X.shape[0])
        kg = plan.forward(Xd)
        # the state holds on the device's own lines too (exported bit for bit), not only on the oracle's
        a_dev, b_dev = plan.lines(Xd)
        n = torch.bincount(forward_classes(a_dev.cpu(), b_dev.cpu(), torch.ones(a_dev.shape[:2]))["state"].reshape(-1),
                           minlength=4).tolist()
        want = {"line0": n[0] >= 8 and sum(n) - n[0] >= 8, "tied": n[2] >= 8, "equal": n[3] >= 2,
                "equal-tied": n[3] >= 2 and n[2] >= 8}[kind]
        assert want, f"device lines: {dict(zip(HINT_STATES, n))}"
        kg_ref, _ = discrete_kg_batched(om, X, D, W, target)
        amax = lines_batched(om, X, D, W, target)[0].abs().amax((-1, -2))
        r = assert_within(kg, kg_ref, stated_tol(kg_ref, amax), f"{mk} slots {slots} {kind} target={target}: KG")
        kg_walked, pairs, _ = plan.forward_stats(Xd)
        _assert_mean_of_pairs(kg, pairs)
        assert torch.equal(kg, kg_walked), "hinted KG differs in bits from the KG of the walked (kg_pairs) path"
        assert torch.equal(both[tau], kg), f"target {target}: the 2-target plan's row differs from the single plan"
        print(f"{mk} slots {slots} {kind} target={target}: {dict(zip(HINT_STATES, n))}, KG worst err/tol {r:.3g}")


# ---------------------------------------------------------------- 4. the intercept cache
CACHE_ROWS = [r["id"] for r in FORWARD_MATRIX if r["cell"][1] == "slots8"]


@pytest.mark.parametrize("row_id", CACHE_ROWS)
def test_intercept_cache_is_the_line_build(row_id):
    """Plan::itop / itopk (intercepts_kernel's own fma loop per M, no export) must be the bits of the envelope's
    line build.  The same problem is built under permutations of D that send the argmax grid line of a
    scalarisation to k = 1, to lanes 63 and 0 of the first two slots and to k = N.  From the exported lines:
    the permuted plan's lines are the permutation of the original bits, and its argmax sits where it was sent,
    once.  Then, in every plan, the production KG (T from the hint) is bit for bit the KG of the forward_stats
    call (T by env_extremes' wave reduction over the built lines; both then run the same filter, walk and
    sums), and the permuted plans' production KG is the unpermuted run's bit for bit: a pair's KG is a sum of
    non-negative edge terms, one per lane in envelope order, whatever the order of the lines.

    Regression: the successor table (dkg_walk.h walk_table) left each edge on its winning lane, a position of
    the survivor list, which is in line-index order; 2 + 1 of the 2 x 76 values of M8p-slots8 and 2 + 0 of
    M8f-slots8 changed bits under these permutations (by a reordered sum of at most h terms, h the envelope
    size) until the table moved each edge to the lane of its walk step."""
    row = FORWARD_ROWS[row_id]
    state, D, W, X = _problem(row_id)
    N, S, Xd = D.shape[0], W.shape[0], X.to(DEV)
    changed = {}
    for target in row["targets"]:
        plan = _device_state(row_id).plan(W, target, X.shape[0])
        kg = plan.forward(Xd)
        kg_walked, _, hull = plan.forward_stats(Xd)
        assert torch.equal(kg, kg_walked)
        rtol = (int(hull.max()) + S + 1) * EPS
        a0, b0 = (t.cpu() for t in plan.lines(Xd))
        top = a0[0, :, 1:].argmax(-1)                         # per scalarisation, row of D (first index)
        moved = 0
        for j, dest in enumerate((0, 63, 64, N - 1)):
            src = int(top[j])
            assert int((a0[0, j, 1:] == a0[0, j, 1 + src]).sum()) == 1
            perm = torch.arange(N)
            perm[dest], perm[src] = src, dest
            plan_p = DeviceGPState(state, D[perm], device=DEV).plan(W, target, X.shape[0])
            ap, bp = (t.cpu() for t in plan_p.lines(Xd))
            lperm = torch.cat([torch.zeros(1, dtype=torch.long), 1 + perm])
            assert torch.equal(ap, a0[..., lperm]) and torch.equal(bp, b0[..., lperm])
            assert int(ap[0, j, 1:].argmax()) == dest and int((ap[0, j, 1:] == ap[0, j, 1 + dest]).sum()) == 1
            kg_p = plan_p.forward(Xd)
            assert torch.equal(kg_p, plan_p.forward_stats(Xd)[0]), (
                f"{row_id} target={target}: argmax line at k={dest + 1}, hinted KG differs from the walked one")
            torch.testing.assert_close(kg_p, kg, rtol=rtol, atol=0.0)
            moved += int((kg_p != kg).sum())
        print(f"{row_id} target={target}: {moved} of {4 * X.shape[0]} KG values change bits with the line order")
        changed[target] = moved
    assert not any(changed.values()), f"KG values whose bits change with the order of D's rows, per target: {changed}"


# ---------------------------------------------------------------- 5. staged chain against its overflow path
@pytest.mark.parametrize("row_id", ["M2-stream", "M3-stream", "M4-stream"])
def test_small_stream_chain_matches_overflow_path(row_id):
    """The few-second twin of test_stress_sample_chain_matches_overflow_path (test_gpu_parity.py): the
    streaming forward's one staged pass against DKG_PLAN_NO_CHAIN, which sends every pair through the overflow
    path; both walks are the reference walk, so pairs, envelope sizes and KG agree bit for bit.

    Regression: at these shapes 8, 8 and 9 of 152 pairs (target None) differed by at most 2.05e-16 relative with
    every envelope size equal.  The two filters leave different survivor lists around the same envelope; a list
    of up to 32 entries is walked by the successor table (dkg_walk.h walk_table), which left each edge term on
    the lane of its list position, so finish_edges summed the same non-negative terms in another order.  The
    table now moves each edge to the lane of its walk step, the order of the step-by-step walks."""
    row = FORWARD_ROWS[row_id]
    _, _, W, X = _problem(row_id)
    Xd = X.to(DEV)
    for target in row["targets"]:
        chain = _device_state(row_id).plan(W, target, X.shape[0])
        plain = _device_state(row_id).plan(W, target, X.shape[0], no_chain=True)
        assert chain.envelope_geometry()["stream"] == 1 and plain.envelope_geometry()["stream"] == 1
        kg_c, pairs_c, hull_c = chain.forward_stats(Xd)
        kg_p, pairs_p, hull_p = plain.forward_stats(Xd)
        diff = pairs_c != pairs_p
        rel = ((pairs_c - pairs_p).abs() / pairs_p.abs().clamp_min(1e-300))[diff]
        print(f"{row_id} target={target}: {int(diff.sum())} of {diff.numel()} pairs differ in bits, largest "
              f"relative difference {float(rel.max()) if rel.numel() else 0.0:.3g} ({EPS:.3g} = 1 eps); "
              f"{int((hull_c != hull_p).sum())} envelope sizes differ; envelopes of up to {int(hull_c.max())} lines")
        assert int((pairs_c > 0).sum()) > 0
        assert torch.equal(hull_c, hull_p)
        assert torch.equal(pairs_c, pairs_p)
        assert torch.equal(kg_c, kg_p)
        assert torch.equal(chain.forward(Xd), plain.forward(Xd))


# ---------------------------------------------------------------- the bug the matrix found (M4-S40, target 3)
@pytest.mark.parametrize("mirror", [False, True], ids=["T-is-L", "T-is-R"])
def test_top_line_at_the_end_of_the_slope_range_in_an_overflowing_list(mirror):
    """The line with the largest intercept also has the smallest slope (T = L), and more than ENV_CAP = 128
    lines pass the L-T-R chord filter: 24 tangents of z^2 / 2 at slopes 0..3 (all on the envelope, T the one
    at slope 0) and 300 lines between the chord T-R and the chain T-V2-R.  The staged envelope then filters
    the lines again in two halves, slopes <= b_T against the chords L-V1 and V1-T; with T = L both are
    degenerate and keep nothing, so T itself was dropped, the list walk found no L and returned one line and
    KG = 0 (M4-S40 target 3, candidate 17, pairs 18 and 39: 0.0 for 2.4e-13 and 6.6e-6).  ``mirror``: the slopes
    negated (T = R).  Index work: the device walk is the reference walk exactly."""
    from dkg_amd import calculate_epigraph_indices
    from oracle.discretekg import calculate_epigraph_indices as ref_epigraph

    g = torch.Generator().manual_seed(7)
    s = torch.linspace(0.0, 3.0, 24, dtype=torch.double)
    bi = 0.05 + 2.9 * torch.rand(300, generator=g, dtype=torch.double)
    a = torch.cat([-0.5 * s * s, -1.5 * bi + 0.02])       # inner lines: 0.02 above the chord a = -1.5 b
    b = torch.cat([s, bi])
    perm = torch.randperm(a.numel(), generator=g)
    a, b = a[perm], (-b if mirror else b)[perm]
    gi, gx = calculate_epigraph_indices(a.to(DEV), b.to(DEV))
    ri, rx = ref_epigraph(a, b)
    assert len(ri) == 24
    assert torch.equal(gi.cpu(), ri), f"indices {gi.tolist()} != {ri.tolist()}"
    assert torch.equal(gx.cpu(), rx)


# ---------------------------------------------------------------- 6. lists longer than LIST_CAP_STREAM
@pytest.mark.parametrize("row_id", [r["id"] for r in FORWARD_LONG])
def test_streaming_long_lists(row_id):
    """d = 1 grids whose envelopes exceed 512 lines (test_forward_matrix_oracle.py): M = 1 on the older streaming
    path (refine_stream, walk_stream), M = 2 on the staged chain and then its overflow.  Production KG at the
    stated tolerance; the forward's hull sizes are the reference walk's on the plan's own lines."""
    row = FORWARD_LONG_ROWS[row_id]
    state, D, W, X = _problem(row_id)
    om, Xd = to_oracle(state), X.to(DEV)
    plan = _device_state(row_id).plan(W, None, X.shape[0])
    _assert_geometry(plan, row)
    kg = plan.forward(Xd)
    kg_ref, _ = discrete_kg_batched(om, X, D, W, None)
    amax = lines_batched(om, X, D, W, None)[0].abs().amax((-1, -2))
    r = assert_within(kg, kg_ref, stated_tol(kg_ref, amax), f"{row_id}: production KG (stated tolerance)")
    kg_s, pairs, hull = plan.forward_stats(Xd)
    _assert_mean_of_pairs(kg, pairs)
    sizes = assert_envelopes_are_reference_walk(*plan.lines(Xd), hull)
    print(f"{row_id}: KG worst err/tol {r:.3g}, envelopes of {sizes[0]}..{sizes[-1]} lines")
    assert sizes[-1] > 512
