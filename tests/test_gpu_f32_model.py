"""The fp32 plan's kernels (DKG_PLAN_F32: cross_root_plan_kernel<DM, float>, cross_big32_kernel,
posterior_cov_kernel<DM, float>, posterior_cov_big32_kernel<DM>, frag_to_f32_kernel and the quad-packed layout)
held to the rounding model of tests/f32_model.py, stage by stage, at ragged shapes (needs a real MI355X).

Per case of f32_model.MATRIX (the table there states T = n_pad / 16 per output and the covariance launch's
blocks, derived from the launcher; test_f32_model_host.py checks them against the dispatch query) and per target
(None, output 0, the last output):

  1. dispatch: the query says the plan's shape takes the kernels the matrix names (a forcing environment
     variable -- DKG_CROSS_BIG, DKG_COV_BIG, DKG_COV_BIG32 -- makes this fail, as intended);
  2. lines: the intercepts of plan(f32=True).lines(X) against oracle.lines_batched at LINE_RTOL (the means stay
     fp64);
  3. cross stage: the exported fp32 Q_X (dkg_debug_plan_qx32) against K32 @ R32 within E1; its rows
     B .. pad16(B) - 1 and columns n .. n_pad - 1 are exactly zero (both cross kernels write every tile of
     pad16(B) x n_pad; K(x, X) is zero outside B x n and R^T's padding rows are zero: csrc/dkg_stages.h);
  4. covariance stage: the slopes against the slope reference built from that exported Q_X, within E2 carried
     through the slopes' linear map plus the fp64 floor;
  5. envelope: plan.forward(X) at the first (at most 8) candidates against the reference walk on the device's own
     fp32 lines, within helpers.stated_tol: the envelope read the records the fp32 covariance kernel wrote;
  6. the worst err / bound per stage is printed, and with DKG_F32_MODEL_REPORT=<path> written as JSON
     (profiles/f32_model/parity.json).

No bug was found by these tests: every case passes against the derived bound (C0 = 4); the measured worst ratios
are in DESIGN.md 4.6.
"""

import functools
import json
import os

import pytest
import torch

import f32_model as fm
from dkg_amd.gp_state import DeviceGPState
from helpers import LINE_RTOL, assert_within, stated_tol
from oracle.discretekg import kg_pairs_from_lines, lines_batched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(r["id"], t) for r in fm.MATRIX for t in fm.targets_of(r)]
_REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("DKG_F32_MODEL_REPORT")
    if out and _REPORT:
        worst = {k: max(c[k] for c in _REPORT.values()) for k in ("cross_ratio", "cov_ratio", "line_rel_a",
                                                                  "envelope_ratio")}
        with open(out, "w") as f:
            json.dump({"u": fm.U, "c0": fm.C0, "line_rtol": LINE_RTOL, "cases": _REPORT, "worst": worst}, f, indent=1)


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """The case's problem, device state and per-output operands (R from the device's row-major L^-1), once."""
    row = fm.ROWS[case_id]
    state, D, W, X = fm.problem(row)
    dstate = DeviceGPState(state, D, device=DEV)
    om = fm.oracle_model(state)
    ops = [fm.operands(o, X, D, Linv=c.Linv) for o, c in zip(om.models, dstate.outputs)]
    return row, state, D, W, X, dstate, om, ops


@functools.lru_cache(maxsize=None)
def _oracle_lines(case_id, target):
    _, _, D, W, X, _, om, _ = _case(case_id)
    return lines_batched(om, X, D, W, target)


@pytest.mark.parametrize("case_id,target", CASES, ids=[f"{c}-t{t}" for c, t in CASES])
def test_f32_stages_within_the_rounding_model(case_id, target):
    row, state, D, W, X, dstate, om, ops = _case(case_id)
    B = X.shape[0]
    plan = dstate.plan(W, target, B, f32=True)
    assert plan.f32

    # 1. dispatch
    disp = plan.f32_dispatch(B)
    assert (disp["cross"], disp["cov"]) == (row["cross"], row["cov"]), f"{case_id}: dispatch {disp}"
    assert (disp["nbx"], disp["nby"], disp["order"]) == row["cov_blocks"], f"{case_id}: dispatch {disp}"

    # 2. lines: the intercepts are fp64
    a, b = plan.lines(X.to(DEV))
    a, b = a.cpu(), b.cpu()
    a_ref, _ = _oracle_lines(case_id, target)
    rel_a = float((a - a_ref).abs().max() / a_ref.abs().max().clamp_min(1e-300))
    print(f"{case_id} target={target}: intercepts rel {rel_a:.3g}")
    assert rel_a <= LINE_RTOL, f"{case_id}: intercepts vs oracle rel {rel_a:.3e} > {LINE_RTOL}"

    # 3. cross stage, per output
    vs, covs, E2s, cross_ratio = [], [], [], 0.0
    for i, (o, op) in enumerate(zip(om.models, ops)):
        n = o.train_x.shape[0]
        Q = plan.qx32(i, B).double()
        assert Q.shape == (fm.pad16(B), fm.pad16(n))
        assert bool((Q[B:] == 0).all()), f"{case_id} output {i}: Q_X32 rows B.. of the last row tile are not zero"
        assert bool((Q[:, n:] == 0).all()), f"{case_id} output {i}: Q_X32 columns n.. are not zero"
        ref, E1 = fm.cross_reference(op)
        ratio = fm.worst_ratio(Q[:B, :n], ref, E1)
        print(f"{case_id} target={target} output {i} (n {n}): cross err/E1 {ratio:.3g}")
        assert_within(Q[:B, :n], ref, E1, f"{case_id} output {i}: Q_X32 vs K32 @ R32 (E1)")
        cross_ratio = max(cross_ratio, ratio)
        v, cov, E2 = fm.cov_reference(o, op, Q[:B, :n])
        vs.append(v)
        covs.append(cov)
        E2s.append(E2)

    # 4. covariance stage, through the slopes
    b_ref, tol_b = fm.slopes_reference(om, X, D, W, target, vs, covs, E2s)
    cov_ratio = fm.worst_ratio(b, b_ref, tol_b)
    print(f"{case_id} target={target}: slopes err/tol {cov_ratio:.3g} (E2 through the slopes' map + fp64 floor)")
    assert_within(b, b_ref, tol_b, f"{case_id}: slopes vs the reference on the exported Q_X32 (E2)")

    # 5. envelope on the device's own fp32 lines
    nb = min(B, 8)
    kg = plan.forward(X.to(DEV)).cpu()[:nb]
    kg_same = kg_pairs_from_lines(a[:nb], b[:nb]).mean(-1)
    tol_env = stated_tol(kg_same, a[:nb].abs().amax(dim=(-1, -2)))
    env_ratio = assert_within(kg, kg_same, tol_env, f"{case_id}: forward vs the reference walk on its own fp32 lines")

    # 6. report
    print(f"{case_id} target={target}: worst err/bound cross {cross_ratio:.3g}, cov {cov_ratio:.3g}, "
          f"envelope {env_ratio:.3g}")
    _REPORT[f"{case_id}-t{target}"] = {"cross": disp["cross_kernel"], "cov": disp["cov_kernel"],
                                       "cov_blocks": [disp["nbx"], disp["nby"], disp["order"]],
                                       "cross_ratio": cross_ratio, "cov_ratio": cov_ratio, "line_rel_a": rel_a,
                                       "envelope_ratio": env_ratio}


def test_each_fp32_kernel_is_reached_by_at_least_three_cases():
    """By the dispatch query on the matrix's shapes (the per-case test asserts the same of every plan)."""
    from dkg_amd.gp_state import f32_dispatch

    count = {}
    for r in fm.MATRIX:
        got = f32_dispatch(fm.max_np_of(r), r["d"], r["N"], r["m"], r["B"])
        for k in ("cross_kernel", "cov_kernel"):
            count[got[k]] = count.get(got[k], 0) + 1
    assert len(count) == 4 and min(count.values()) >= 3, count


def test_qx32_export_refuses_an_fp64_plan():
    from dkg_amd.errors import UnsupportedError

    _, _, _, W, X, dstate, _, _ = _case("n-odd")
    plan = dstate.plan(W, None, X.shape[0])
    plan.lines(X.to(DEV))
    with pytest.raises(UnsupportedError, match="DKG_PLAN_F32"):
        plan.qx32(0, X.shape[0])
