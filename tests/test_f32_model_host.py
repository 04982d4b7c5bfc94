"""The fp32 rounding model (tests/f32_model.py) checked on the CPU, and the fp32 dispatch query on the host.

For every case of f32_model.MATRIX, per output and per stage (cross: K32 @ R32; covariance: Q_X32 @ QD32^T with
Q_X32 the rounded chunk-of-4 emulation of the cross stage, standing in for the device's exported one):

  * four fp32 emulations of the contraction (sequential, reversed, chunks of 4, chunks of 64) stay within the
    bound; their worst err / bound is printed and asserted <= 0.5;
  * every structured mutation (f32_model.mutate / mutate_stride) puts at least one entry outside the bound by a
    factor >= 4 wherever the shape has a place for it; where it has none is stated in NO_PLACE below and
    asserted, so a mutation cannot silently stop applying;
  * dkg_debug_f32_dispatch names the kernels (and the covariance launch's blocks) the matrix states.
"""

import ctypes
import functools

import pytest
import torch

import f32_model as fm
from dkg_amd import _lib
from dkg_amd.gp_state import f32_dispatch

IDS = [r["id"] for r in fm.MATRIX]
FLAG_FACTOR = 4.0
EMULATION_LIMIT = 0.5

# (mutation -> cases) whose shape has no place for the mutation in either stage of any output:
#   tiles: a single column tile in both stages (n <= 16 and N <= 16);
#   stale: no partial last tile with a tile before it (B <= 16 or B % 16 == 0, and the same of n and N);
#   dmap : no live D row that the map moves (a 1 x 1 output);
#   stride: no output narrower than the widest (m = 1, or every output of one n_pad), or a single row tile
#           (B <= 16: tile 0 starts at word 0 under either stride, so the mistake is harmless there).
NO_PLACE = {
    "drop": set(), "swap": set(),
    "tiles": {"n-min"},
    "stale": {"n-min", "n-496"},
    "dmap": {"n-min"},
    "stride": {"n-min", "n-d16", "n-m5", "n-496", "x-np", "x-rag", "x-d16", "c-edge", "c-below", "c-ord0", "c-d16",
               "xc"},
}


@functools.lru_cache(maxsize=None)
def _stages(case_id):
    """Per output: (name, A, Bm, reference, bound, d_rows_are_columns) of both stages."""
    row = fm.ROWS[case_id]
    state, D, W, X = fm.problem(row)
    out = []
    for i, om in enumerate(fm.oracle_model(state).models):
        op = fm.operands(om, X, D)
        ref1, E1 = fm.cross_reference(op)
        QX32 = fm.fl32(fm.emulate(op["K32"], op["R32"], "c4"))
        ref2 = QX32 @ op["QD32"].mT
        E2 = fm.bound(fm.pad16(QX32.shape[1]), QX32.abs(), op["QD32"].abs().mT)
        out.append([("cross", op["K32"], op["R32"], ref1, E1, True), ("cov", QX32, op["QD32"].mT, ref2, E2, False)])
    return out


@pytest.mark.parametrize("case_id", IDS)
def test_fp32_emulations_stay_within_the_bound(case_id):
    worst = {}
    for stages in _stages(case_id):
        for name, A, Bm, ref, E, _ in stages:
            for order in fm.EMULATIONS:
                got = fm.emulate(A, Bm, order)
                if name == "cross":
                    got = fm.fl32(got)  # (the store; emulate's sums are fp32 already: a no-op kept for the model)
                worst[name, order] = max(worst.get((name, order), 0.0), fm.worst_ratio(got, ref, E))
    print(f"{case_id}: worst err/bound " + ", ".join(f"{s}/{o} {v:.3g}" for (s, o), v in sorted(worst.items())))
    assert max(worst.values()) <= EMULATION_LIMIT, worst


@pytest.mark.parametrize("case_id", IDS)
def test_structured_mutations_are_flagged(case_id):
    row = fm.ROWS[case_id]
    max_np = fm.max_np_of(row)
    placed = {k: False for k in NO_PLACE}
    for stages in _stages(case_id):
        for name, A, Bm, ref, E, dcols in stages:
            for kind in fm.MUTATIONS:
                got = fm.mutate(A, Bm, kind, d_rows_are_columns=dcols)
                if got is None:
                    continue
                placed[kind] = True
                ratio = fm.worst_ratio(got, ref, E)
                assert ratio >= FLAG_FACTOR, f"{case_id} {name} {kind}: worst err/bound {ratio:.3g} < {FLAG_FACTOR}"
            if name == "cross":
                got = fm.mutate_stride(ref, max_np)
                if got is not None:
                    placed["stride"] = True
                    ratio = fm.worst_ratio(got, ref, E)
                    assert ratio >= FLAG_FACTOR, f"{case_id} stride: worst err/bound {ratio:.3g} < {FLAG_FACTOR}"
    for kind, here in placed.items():
        assert here == (case_id not in NO_PLACE[kind]), f"{case_id}: mutation {kind} placed={here}"


def test_an_exact_result_is_inside_and_the_mutations_are_not_vacuous():
    """The unmutated product is inside the bound by construction (ratio 0), so what the mutation test flags is
    the mutation."""
    name, A, Bm, ref, E, _ = _stages("n-odd")[0][0]
    Ap, Bp = fm._padded(A, Bm)
    assert fm.worst_ratio((Ap @ Bp)[:A.shape[0], :Bm.shape[1]], ref, E) <= 1e-6


@pytest.mark.parametrize("case_id", IDS)
def test_dispatch_query_names_the_matrix_kernels(case_id):
    row = fm.ROWS[case_id]
    got = f32_dispatch(fm.max_np_of(row), row["d"], row["N"], row["m"], row["B"])
    assert (got["cross"], got["cov"]) == (row["cross"], row["cov"]), f"{case_id}: {got}"
    assert (got["nbx"], got["nby"], got["order"]) == row["cov_blocks"], f"{case_id}: {got}"
    assert got["DM"] == (2 if row["d"] <= 2 else 4 if row["d"] <= 4 else 8 if row["d"] <= 8 else 16)
    # a launch of several batches takes the kernels one batch would (geom_B), whatever its candidate count
    many = f32_dispatch(fm.max_np_of(row), row["d"], row["N"], row["m"], 8 * row["B"], row["B"])
    assert (many["cross"], many["cov"]) == (row["cross"], row["cov"]), f"{case_id} x 8 batches: {many}"


def test_dispatch_thresholds_and_exclusions():
    """Both sides of every rule: the fill by n_pad (512) and by B (512), cov_big's 256 blocks and N >= 128, and
    d > 8 keeping the narrow covariance kernel."""
    q = lambda *a: f32_dispatch(*a)  # noqa: E731  (max_np, d, N, m, B[, geom_B])
    assert q(496, 2, 64, 1, 511)["cross"] == "narrow" and q(496, 2, 64, 1, 512)["cross"] == "big32"
    assert q(512, 2, 64, 1, 1)["cross"] == "big32" and q(512, 11, 64, 1, 1)["cross"] == "big32"
    assert q(16, 2, 2000, 8, 20)["cov"] == "big32" and q(16, 2, 1984, 8, 20)["cov"] == "narrow"
    assert q(16, 8, 2000, 8, 20)["cov"] == "big32" and q(16, 9, 2000, 8, 20)["cov"] == "narrow"
    assert q(16, 2, 127, 8, 64 * 256)["cov"] == "narrow" and q(16, 2, 128, 8, 64 * 16)["cov"] == "big32"
    # geom_B decides, not the launch's candidate count
    assert q(16, 2, 2000, 7, 20 * 64, 20)["cov"] == "narrow" and q(16, 2, 2000, 7, 20, 20 * 64)["cov"] == "big32"
    assert q(16, 2, 64, 1, 1024, 256)["cross"] == "narrow" and q(16, 2, 64, 1, 1024, 512)["cross"] == "big32"
    assert set(n for r in fm.MATRIX for n in (r["cross"], r["cov"])) == {"narrow", "big32"}
    for key, name in (("cross", "narrow"), ("cross", "big32"), ("cov", "narrow"), ("cov", "big32")):
        assert sum(r[key] == name for r in fm.MATRIX) >= 3, f"fewer than three cases reach the {name} {key} kernel"


def test_debug_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    out = (ctypes.c_int * 6)()
    for bad in ((8, 2, 10, 1, 1, 0), (24, 2, 10, 1, 1, 0), (16, 0, 10, 1, 1, 0), (16, 17, 10, 1, 1, 0),
                (16, 2, -1, 1, 1, 0), (16, 2, 10, 0, 1, 0), (16, 2, 10, 9, 1, 0), (16, 2, 10, 1, 0, 0),
                (16, 2, 10, 1, 1, -1), (2048, 2, 10, 1, 1, 0)):
        assert lib.dkg_debug_f32_dispatch(*bad, out) == -2
        assert b"dkg_debug_f32_dispatch" in lib.dkg_last_error()
    assert lib.dkg_debug_f32_dispatch(16, 2, 10, 1, 1, 0, None) == -2
    assert lib.dkg_debug_f32_dispatch(16, 2, 10, 1, 1, 0, out) == 0
    with pytest.raises(Exception, match="dkg_debug_f32_dispatch"):
        f32_dispatch(8, 2, 10, 1, 1)
    # the Q_X export: NULL pointers, and a plan without fp32 contractions (a blank plan has no DKG_PLAN_F32)
    buf = (ctypes.c_float * 256)()
    blank = ctypes.create_string_buffer(lib.dkg_plan_bytes())
    assert lib.dkg_debug_plan_qx32(None, 0, 1, buf, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_debug_plan_qx32(blank, 0, 1, None, None) == _lib.DKG_ERR_ARG
    assert lib.dkg_debug_plan_qx32(blank, 0, 1, buf, None) == _lib.DKG_ERR_UNSUPPORTED
    assert b"DKG_PLAN_F32" in lib.dkg_last_error()
    assert lib.dkg_abi_version() == _lib.ABI_VERSION


def test_frag32_index_is_a_bijection_and_matches_the_layout():
    """f32_model.frag32_index (the mutation's packing) restates csrc/dkg_common.h: element
    (16 t + (l & 15), 4 kb + (l >> 4)) at ((t KB/4 + kb/4) 64 + l) 4 + (kb & 3)."""
    for rows, np_ in ((16, 16), (32, 48), (48, 208)):
        r = torch.arange(rows)[:, None].expand(rows, np_)
        c = torch.arange(np_)[None, :].expand(rows, np_)
        idx = fm.frag32_index(r >> 4, c >> 2, ((c & 3) << 4) | (r & 15), np_ // 4).reshape(-1)
        assert sorted(idx.tolist()) == list(range(rows * np_))
    assert fm.frag32_index(0, 0, 0, 4) == 0 and fm.frag32_index(0, 1, 0, 4) == 1 and fm.frag32_index(0, 0, 1, 4) == 4
    assert fm.frag32_index(1, 5, 17, 12) == ((1 * 3 + 1) * 64 + 17) * 4 + 1


@pytest.mark.parametrize("case_id", ["n-odd", "n-mixed", "n-m5"])
def test_slope_reference_is_the_oracles_lines_on_fp64_operands(case_id):
    """f32_model.slopes_reference fed the oracle's own fp64 Q_X and Q_D gives oracle.lines_batched's slopes (the
    coincident candidate's copied line 0 included), for the full and the decoupled paths; and fed the fp32
    operands it stays within its own tolerance of itself only through E2 (line 0 of the other candidates: the
    floor alone)."""
    from oracle.discretekg import lines_batched

    row = fm.ROWS[case_id]
    state, D, W, X = fm.problem(row)
    om = fm.oracle_model(state)
    vs, covs, E2s = [], [], []
    for o in om.models:
        n = o.train_x.shape[0]
        c = o.cache()
        Qx = o.covar(X, torch.cat([o.train_x, X], 0))[:, :n] @ c["R"]
        Qd = o.covar(D, torch.cat([o.train_x, D], 0))[:, :n] @ c["R"]
        vs.append(o.outputscale - (Qx * Qx).sum(-1))
        covs.append(o.covar(X, D) - Qx @ Qd.mT)
        E2s.append(fm.bound(fm.pad16(n), Qx.abs(), Qd.abs().mT))
    for target in fm.targets_of(row):
        _, b_ref = lines_batched(om, X, D, W, target)
        b, tol = fm.slopes_reference(om, X, D, W, target, vs, covs, E2s)
        torch.testing.assert_close(b, b_ref, rtol=1e-12, atol=1e-14)
        floor = fm.LINE_RTOL * float(b.abs().max())
        on_d = [bi for bi in range(X.shape[0]) if fm.coincident_index(X[bi], D) is not None]
        assert on_d == ([row["coincide"][0]] if row["coincide"] else [])
        for bi in range(X.shape[0]):
            if bi in on_d:
                assert bool((tol[bi, :, 0] > floor).all())
            else:
                assert bool((tol[bi, :, 0] == floor).all())
        assert bool((tol[:, :, 1:] > floor).all())
