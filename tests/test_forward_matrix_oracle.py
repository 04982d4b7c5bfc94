"""The reference side of the forward case matrix (helpers.FORWARD_MATRIX, the hint-state inputs of
helpers.hint_case and the long-list rows helpers.FORWARD_LONG), on the oracle alone (no GPU): the inputs
exercise the branches of the production forward that tests/test_gpu_forward_matrix.py names.

Everything here is a condition on inputs (helpers.forward_classes classifies the oracle's lines), met by the
choice of seeds, not a tolerance:

  * every (output bucket, envelope instantiation) cell is in the matrix, N + 1 in the claimed slot bucket;
  * per output bucket, a staged case with at least 8 flat pairs (env_flat settles them without a walk) and at
    least 8 walked pairs with KG > 0, and somewhere a candidate whose pairs are all flat;
  * the hint-state inputs reach "line 0 on top" (>= 8 pairs with and >= 8 without), "tied top grid intercept"
    (>= 8 pairs) and "a0 == A1" (>= 2 pairs), and no matrix row does so in numbers: they are needed;
  * the long-list rows have an envelope of more than LIST_CAP_STREAM = 512 lines."""

import functools

import pytest
import torch

from helpers import (FORWARD_CASES, FORWARD_GEOMETRIES, FORWARD_LONG, FORWARD_LONG_ROWS, FORWARD_MATRIX, FORWARD_NS,
                     FORWARD_ROWS, HINT_KINDS, HINT_NS, HINT_STATES, forward_classes, forward_row_problem, hint_case,
                     to_oracle)
from oracle.discretekg import calculate_epigraph_indices, kg_pairs_from_lines, lines_batched

BUCKET = {"M1": 1, "M2": 2, "M3": 3, "M4": 4, "M8p": 8, "M8f": 8}


def test_every_bucket_and_envelope_is_in_the_matrix():
    cells = {r["cell"] for r in FORWARD_MATRIX}
    for mk in FORWARD_NS:
        for gk, *_ in FORWARD_GEOMETRIES:
            assert (mk, gk) in cells, (mk, gk)
    assert {("M3", "split3"), ("M4", "split5")} <= cells
    for r in FORWARD_MATRIX:
        mk, gk = r["cell"]
        assert r["m"] == len(FORWARD_NS[mk]) and r["targets"] == (None, r["m"] - 1), r["id"]
        assert len(set(r["ns"])) == r["m"] and max(r["ns"]) <= 64 and r["d"] in (2, 3, 4), r["id"]
        assert r["B"] == 19 and r["S"] == (24 if gk == "split3" else 40 if gk == "split5" else 8), r["id"]
        assert r["split"] == (r["S"] + 7) // 8, r["id"]
        lines = r["N"] + 1  # the slot count follows N + 1 (dkg_kernels.h env_slots)
        want = 2 if lines <= 128 else 8 if lines <= 512 else 17 if lines <= 1088 else 33 if lines <= 2112 else 0
        if gk.startswith("slots"):
            assert want == int(gk[5:]), r["id"]
        if r["stream"]:
            # by N, or (the M = 8 bucket at the 33-slot N: two staged arrays of 64 * 33 * 8 doubles) by its LDS
            assert r["slots"] == 0 and (want == 0 or (BUCKET[mk] == 8 and want == 33)), r["id"]
        else:
            assert r["slots"] == want, r["id"]
    # every bucket's staged and streaming kernels, and the kernel families across the M = 1 rows
    for mk in FORWARD_NS:
        staged = {r["slots"] for r in FORWARD_MATRIX if r["cell"][0] == mk and not r["stream"]}
        assert staged >= ({2, 8, 17} if BUCKET[mk] == 8 else {2, 8, 17, 33}), mk
        assert any(r["stream"] for r in FORWARD_MATRIX if r["cell"][0] == mk), mk
    assert {r["fam"][0] for r in FORWARD_MATRIX if r["m"] == 1} == {"M12", "M32", "M52", "RBF"}


@functools.lru_cache(maxsize=None)
def _classes(row_id, target):
    state, D, W, X = forward_row_problem(FORWARD_ROWS[row_id])
    a, b = lines_batched(to_oracle(state), X, D, W, target)
    pairs = kg_pairs_from_lines(a, b)
    return forward_classes(a, b, pairs), pairs


def test_flat_pairs_have_reference_kg_zero():
    """What the classifier calls flat, the reference walk gives KG = 0 exactly (psi's fp64 cut): the value the
    device tests demand of those pairs."""
    for row_id, target in FORWARD_CASES:
        c, pairs = _classes(row_id, target)
        assert bool((pairs[c["flat"]] == 0.0).all()), (row_id, target)


@pytest.mark.parametrize("bucket", sorted(set(BUCKET)))
def test_every_bucket_has_flat_and_walked_pairs(bucket):
    """A staged case per output bucket with >= 8 flat pairs next to >= 8 walked pairs with KG > 0."""
    found = []
    for row_id, target in FORWARD_CASES:
        row = FORWARD_ROWS[row_id]
        if row["cell"][0] != bucket or row["stream"]:
            continue
        c, pairs = _classes(row_id, target)
        nflat, nwalked = int(c["flat"].sum()), int((~c["flat"] & (pairs > 0)).sum())
        if nflat >= 8 and nwalked >= 8:
            found.append((row_id, target, nflat, nwalked))
    print(f"{bucket}: (row, target, flat pairs, walked pairs with KG > 0) {found}")
    assert found


def test_flat_pairs_with_all_outputs_observed_and_all_flat_candidates():
    """Flat pairs also under target None (every output's deviation small at once), and candidates whose pairs
    are all flat (production KG exactly 0.0) under both kinds of target."""
    none_flat = {r: int(_classes(r, t)[0]["flat"].sum()) for r, t in FORWARD_CASES if t is None}
    assert sum(n >= 8 for n in none_flat.values()) >= 2, none_flat
    for kind in (True, False):
        allflat = sum(int(_classes(r, t)[0]["flat"].all(-1).sum()) for r, t in FORWARD_CASES if (t is None) == kind)
        assert allflat >= 1, kind


def test_the_matrix_alone_leaves_the_hint_states_unreached():
    """Why hint_case exists: over the matrix's staged rows nearly every pair is "grid-unique"."""
    counts = torch.zeros(4, dtype=torch.long)
    for row_id, target in FORWARD_CASES:
        if not FORWARD_ROWS[row_id]["stream"]:
            counts += torch.bincount(_classes(row_id, target)[0]["state"].reshape(-1), minlength=4)
    print(dict(zip(HINT_STATES, counts.tolist())))
    assert int(counts[2]) == 0 and int(counts[3]) == 0 and int(counts[1]) > 0.9 * int(counts.sum())


@pytest.mark.parametrize("kind", HINT_KINDS)
@pytest.mark.parametrize("slots", [2, 8, 17])
@pytest.mark.parametrize("mk", list(HINT_NS))
def test_hint_inputs_reach_their_state(mk, slots, kind):
    state, D, W, X = hint_case(mk, slots, kind)
    lines = D.shape[0] + 1
    assert (2 if lines <= 128 else 8 if lines <= 512 else 17 if lines <= 1088 else 33) == slots
    assert X.shape[0] == 19 and W.shape[0] == 8
    om = to_oracle(state)
    for target in (None, len(HINT_NS[mk]) - 1):
        a, b = lines_batched(om, X, D, W, target)
        st = forward_classes(a, b, torch.ones(a.shape[:2]))["state"]  # the states need no reference KG
        n = dict(zip(HINT_STATES, torch.bincount(st.reshape(-1), minlength=4).tolist()))
        print(f"{mk} slots {slots} {kind} target={target}: {n}")
        if kind == "line0":
            assert n["line0"] >= 8 and st.numel() - n["line0"] >= 8
        elif kind == "tied":
            assert n["grid-tied"] >= 8
        else:
            assert n["equal"] >= 2
            assert bool((st[0] == 3).any()) and bool((st[1] == 3).any())
            if kind == "equal-tied":
                assert n["grid-tied"] >= 8


@pytest.mark.parametrize("row_id", [r["id"] for r in FORWARD_LONG])
def test_long_list_rows_are_long(row_id):
    """Some pair's envelope has more than LIST_CAP_STREAM = 512 lines: the streaming forward's list overflows
    whatever the filter keeps."""
    state, D, W, X = forward_row_problem(FORWARD_LONG_ROWS[row_id])
    assert D.shape[0] + 1 > 64 * 33
    a, b = lines_batched(to_oracle(state), X, D, W, None)
    sizes = sorted(len(calculate_epigraph_indices(a[i, j], b[i, j])[0])
                   for i in range(a.shape[0]) for j in range(a.shape[1]))
    print(f"{row_id}: envelopes of {sizes[0]}..{sizes[-1]} lines, {sum(s > 512 for s in sizes)} over 512")
    assert sizes[-1] > 512
