"""The reference side of the value+gradient case matrix (helpers.GRAD_MATRIX), on the oracle alone (no GPU):

(a) the oracle's autograd gradient against central differences of the oracle's own KG, so the reference
    tests/test_gpu_grad_matrix.py compares the device with is itself checked on every row's inputs;
(b) the inputs exercise what the row claims: gradients far above the tolerance's floor (a wrong device
    gradient cannot hide under it), and envelopes longer than the flush queue on the long-envelope rows.

The bound of (a), max |fd - g| <= 1e-5 max |g| with h = 1e-6 (1e-7 on the d = 1 long-envelope rows, whose
Matern-1/2 lines have kinks at the training points a wider stencil would straddle), is about 50 times the worst
value measured and five orders below any formula error.  (b) holds by the choice of seeds: conditions on the
inputs, not tolerances."""

import functools

import pytest
import torch

from helpers import (GRAD_CASES, GRAD_MATRIX, GRAD_ROWS, grad_row_problem, grad_scale, grad_tol,
                     oracle_value_and_grad, to_oracle)
from oracle.discretekg import calculate_epigraph_indices, discrete_kg_batched, lines_batched


@functools.lru_cache(maxsize=None)
def _problem(row_id):
    state, D, W, X = grad_row_problem(GRAD_ROWS[row_id])
    return to_oracle(state), D, W, X


@pytest.mark.parametrize("row_id,target", GRAD_CASES, ids=[f"{r}-t{t}" for r, t in GRAD_CASES])
def test_oracle_gradient_and_inputs(row_id, target):
    row = GRAD_ROWS[row_id]
    om, D, W, X = _problem(row_id)
    _, g = oracle_value_and_grad(om, X, D, W, target)
    # (a) central differences of the oracle's KG, every coordinate
    h = 1e-7 if row_id.startswith("long-") else 1e-6
    fd = torch.zeros_like(X)
    for j in range(row["d"]):
        e = torch.zeros_like(X)
        e[:, j] = h
        fd[:, j] = (discrete_kg_batched(om, X + e, D, W, target)[0] -
                    discrete_kg_batched(om, X - e, D, W, target)[0]) / (2 * h)
    rel = float((fd - g).abs().max() / g.abs().max())
    # (b) the share of candidates whose gradient stands 1e3 above its tolerance
    tol = grad_tol(g, grad_scale(om, X, D, W, target))
    big = (g.abs() >= 1e3 * tol).any(-1).double().mean().item()
    print(f"{row_id} target={target}: max|fd - g| / max|g| {rel:.3g}, candidates with |g| >= 1e3 tol {big:.0%}")
    assert rel <= 1e-5
    assert big >= 0.75


LONG_ROWS = [r["id"] for r in GRAD_MATRIX if r["id"].startswith("long-")]


@functools.lru_cache(maxsize=None)
def _envelope_lengths(row_id):
    om, D, W, X = _problem(row_id)
    a, b = lines_batched(om, X, D, W, None)
    return sorted(len(calculate_epigraph_indices(a[i, j], b[i, j])[0])
                  for i in range(a.shape[0]) for j in range(a.shape[1]))


@pytest.mark.parametrize("row_id", LONG_ROWS)
def test_long_envelope_rows_are_long(row_id):
    """At least one (candidate, scalarisation) pair whose upper envelope has more than 128 lines: the
    gradient envelope's queue (HCAP = 128) flushes mid-walk and the hull has more than 125 survivors."""
    longest = _envelope_lengths(row_id)[-1]
    print(f"{row_id}: longest envelope {longest} lines")
    assert longest > 128


def test_long_envelope_rows_also_hold_a_hull_of_65_to_125_lines():
    """Some pair's envelope has more lines than a wave has lanes but fits the survivor list (at most 125): the
    list hull's queue then holds more than 64 lines in one flush (two lines per lane)."""
    mid = {r: [n for n in _envelope_lengths(r) if 65 < n <= 120] for r in LONG_ROWS}
    print(f"envelopes of 66..120 lines: {mid}")
    assert any(mid.values())


def test_every_bucket_family_and_envelope_is_in_the_matrix():
    """The matrix names every output bucket, dimension bucket, kernel family and envelope instantiation."""
    bucket = lambda m: m if m <= 4 else 8  # noqa: E731
    dm = lambda d: 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16  # noqa: E731
    assert {bucket(r["m"]) for r in GRAD_MATRIX} == {1, 2, 3, 4, 8}
    assert {dm(r["d"]) for r in GRAD_MATRIX} == {2, 4, 8, 16}
    assert {f for r in GRAD_MATRIX for f in r["fam"][:max(r["m"], 1)]} == {"M12", "M32", "M52", "RBF"}
    assert {r["slots"] for r in GRAD_MATRIX if not r["stream"]} == {2, 8, 17, 33}
    assert sum(r["stream"] for r in GRAD_MATRIX) >= 2 and {r["split"] for r in GRAD_MATRIX} >= {1, 3, 5}
    for r in GRAD_MATRIX:  # the slot count follows N + 1 (dkg_kernels.h env_slots); streaming rows report 0
        lines = r["N"] + 1
        want = 2 if lines <= 128 else 8 if lines <= 512 else 17 if lines <= 1088 else 33
        assert r["stream"] or r["slots"] == want, r["id"]
        assert r["split"] == (r["S"] + 7) // 8, r["id"]
