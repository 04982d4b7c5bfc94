"""Shared test helpers: product <-> oracle model conversion and the parity tolerance."""

import math

import torch

from oracle.gp import ModelList, OutputGP

EPS = torch.finfo(torch.double).eps


def to_oracle(state) -> ModelList:
    """dkg_amd ModelListGPState -> oracle ModelList (same fitted state)."""
    return ModelList([OutputGP(m.train_x, m.train_y, m.lengthscale, m.outputscale, m.noise, m.mean_constant,
                               m.kernel, m.nu, m.y_mean, m.y_std) for m in state.models])


def to_state(oracle_model):
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    return ModelListGPState(*[SingleTaskGPState(o.train_x, o.train_y, o.lengthscale.reshape(-1), o.outputscale,
                                                o.noise, o.mean_constant, o.kernel, o.nu, o.y_mean, o.y_std)
                              for o in oracle_model.models])


def stated_tol(ref: torch.Tensor, amax: torch.Tensor, rtol: float = 1e-6) -> torch.Tensor:
    """The parity tolerance BASELINE.md "Accuracy" and SURVEY.md 8(d) state, per value:
    1e-6 |KG| + 64 eps max_k |a_k| (the fp64 cancellation floor of E - max a, discretekg.py:233)."""
    return rtol * ref.abs() + 64.0 * EPS * amax


def grad_scale(om, X, D, W, target=None, h: float = 1e-6) -> torch.Tensor:
    """Per candidate, the magnitude G of the terms dKG/dx sums: with the envelope fixed,
    dKG_w/dx = sum_e [dPhi_e da_e/dx - dphi_e db_e/dx] - [line 0 attains max a] da_0/dx, where only line 0's
    intercept and the slopes depend on x, so every term is bounded by
    G = |da_0/dx|_inf + max_k |db_k/dx|_inf (max over the scalarisations).  Central differences of the
    oracle's lines (a magnitude for the tolerance, not a parity value)."""
    from oracle.discretekg import lines_batched

    B, d = X.shape
    G = torch.zeros(B, dtype=torch.double)
    for j in range(d):
        e = torch.zeros_like(X)
        e[:, j] = h
        ap, bp = lines_batched(om, X + e, D, W, target)
        am, bm = lines_batched(om, X - e, D, W, target)
        da0 = ((ap[..., 0] - am[..., 0]) / (2 * h)).abs()             # [B, S]
        db = ((bp - bm) / (2 * h)).abs().amax(-1)                      # [B, S]
        G = torch.maximum(G, (da0 + db).amax(-1))
    return G


def grad_tol(g_ref: torch.Tensor, G: torch.Tensor, rtol: float = 1e-6) -> torch.Tensor:
    """The gradient's tolerance, stated like the KG's: 1e-6 |g| + 64 eps G per coordinate, G the magnitude of
    the terms the gradient sums (grad_scale): the fp64 cancellation floor of that sum."""
    return rtol * g_ref.abs() + 64.0 * EPS * G.reshape(-1, 1)


SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def line_gap(a_dev, b_dev, a_ref, b_ref):
    """Per candidate, the largest |a_dev - a_ref| and |b_dev - b_ref| over its scalarisations and lines
    (two fp64 builds of the same lines [B, S, L])."""
    da = (a_dev.cpu() - a_ref).abs().amax(dim=(-1, -2))
    db = (b_dev.cpu() - b_ref).abs().amax(dim=(-1, -2))
    return da, db


def kg_line_floor(da, db):
    """How far KG can move when its lines move by at most da (intercepts) and db (slopes):
    E[max_k (a_k + b_k Z)] is 1-Lipschitz in a and E|Z| = sqrt(2/pi)-Lipschitz in b (sup norms), and
    max_k a_k is 1-Lipschitz, so |dKG_w| <= 2 da + sqrt(2/pi) db; the mean over w keeps the bound."""
    return 2.0 * da + SQRT_2_OVER_PI * db


def assert_within(got, ref, tol, what: str = "KG") -> float:
    """|got - ref| <= tol elementwise; returns the worst err/tol ratio."""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    tol = tol.detach().cpu().double().reshape(-1).expand_as(ref)
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
    bad = err > tol
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{bad.numel()} values outside tolerance, worst err/tol "
        f"{float(ratio.max()):.3g}; got {got[bad][:4].tolist()} ref {ref[bad][:4].tolist()}")
    return float(ratio.max()) if ratio.numel() else 0.0


# Relative agreement required of the device lines with the oracle's (max |da| / max |a|, max |db| / max |b|):
# any algorithmic error is O(1) relative; two fp64 builds of an ill-conditioned posterior (s = 50,
# lengthscale 1.8, noise 1e-4: kappa(K) ~ 1e6) differ by rounding amplified by the conditioning.  The
# measured values are in profiles/r02_parity.json.
LINE_RTOL = 1e-8


def parity_case(state, D, W, X, target, dev="cuda"):
    """One end-to-end parity measurement of the HIP forward against the oracle on identical inputs.

    Returns a dict of the worst err/tol ratios and line gaps; the asserts are the caller's:
      lines   : device lines (dkg_plan_lines, the envelope's own) vs oracle.lines_batched;
      envelope: device KG per pair vs the reference walk + expectation on the *same* (device) lines,
                stated tolerance (1e-6 |KG| + 64 eps max|a|) -- isolates the envelope kernel;
      kg      : device KG vs oracle KG per candidate at the stated tolerance alone; the line gap's
                Lipschitz bound (kg_line_floor) is reported as a diagnostic only (``kg_ratio``).
    """
    from dkg_amd import DiscreteKnowledgeGradient
    from oracle.discretekg import kg_pairs_from_lines, lines_batched

    om = to_oracle(state)
    acq = DiscreteKnowledgeGradient(state, D, W, target_output_ix=target, device=dev)
    Xd = X.to(dev)
    plan = acq._plan_for(X.shape[0])
    kg, pairs, _ = plan.forward_stats(Xd)
    a_dev, b_dev = plan.lines(Xd)
    a_dev, b_dev, kg, pairs = a_dev.cpu(), b_dev.cpu(), kg.cpu(), pairs.cpu()
    a_ref, b_ref = lines_batched(om, X, D, W, target)
    pairs_same_lines = kg_pairs_from_lines(a_dev, b_dev)
    pairs_ref = kg_pairs_from_lines(a_ref, b_ref)
    kg_ref = pairs_ref.mean(-1)
    amax_pair = a_ref.abs().amax(-1)                       # [B, S]
    amax = amax_pair.amax(-1)                              # [B]
    da, db = line_gap(a_dev, b_dev, a_ref, b_ref)
    tol_env = stated_tol(pairs_same_lines, a_dev.abs().amax(-1))
    tol_kg = stated_tol(kg_ref, amax)
    err_kg = (kg - kg_ref).abs()
    return {
        "B": X.shape[0], "S": W.shape[0], "lines": a_dev.shape[-1],
        "line_rel_a": float(da.max() / a_ref.abs().max().clamp_min(1e-300)),
        "line_rel_b": float(db.max() / b_ref.abs().max().clamp_min(1e-300)),
        "envelope_ratio": float(((pairs - pairs_same_lines).abs() / tol_env).max()),
        # the asserted ratio (stated tolerance alone), and the same error against the stated tolerance plus
        # the line gap's Lipschitz bound (diagnostic: how much of the tolerance the line gap alone could use)
        "kg_ratio_stated_only": float((err_kg / tol_kg).max()),
        "kg_ratio": float((err_kg / (tol_kg + kg_line_floor(da, db))).max()),
        "kg_max_abs_err": float(err_kg.max()),
        "kg_ref_max": float(kg_ref.abs().max()),
        "line_floor_max": float(kg_line_floor(da, db).max()),
        "stated_floor_max": float((64.0 * EPS * amax).max()),
        "kg_zero_frac": float((kg_ref == 0).double().mean()),
        "_tensors": (kg, kg_ref, tol_kg, pairs, pairs_same_lines, tol_env),
    }


def check_parity_case(res):
    """The asserts on a parity_case result (tests)."""
    assert res["line_rel_a"] <= LINE_RTOL and res["line_rel_b"] <= LINE_RTOL, (
        f"device lines vs oracle: rel {res['line_rel_a']:.3e} / {res['line_rel_b']:.3e} > {LINE_RTOL}")
    kg, kg_ref, tol_kg, pairs, pairs_same, tol_env = res["_tensors"]
    assert_within(pairs, pairs_same, tol_env, "envelope on identical lines")
    assert_within(kg, kg_ref, tol_kg, "end-to-end KG (stated tolerance)")
    print(f"parity: KG err/stated tol {res['kg_ratio_stated_only']:.3g}, line-gap floor max "
          f"{res['line_floor_max']:.3g} (diagnostic, not asserted)")


FAMILIES = {"M12": ("matern", 0.5), "M32": ("matern", 1.5), "M52": ("matern", 2.5), "RBF": ("rbf", None)}
ALL_FAMILIES = ("M52", "M32", "M12", "RBF")


def grad_case(m, d, ns, families, N, S, B, seed, lengthscale=None, noise=None, grid=False, mean_shift=0.0):
    """A seeded value+gradient problem from plain tensors (no device, no global RNG): the same inputs on the
    CPU oracle and on the GPU.  -> (ModelListGPState, D [N, d], W [S, m], X [B, d]).

    Output i: train_x = rand(n_i, d); y = sin(3 sum(x) / sqrt(d) + i) + 0.1 randn; one lengthscale per
    dimension (0.5 + 0.5 rand(d)) sqrt(d / 2), all different (a scalar ``lengthscale`` overrides it);
    outputscale 1 + 0.5 i; noise 1e-2 (1 + i) (a scalar ``noise`` overrides it); mean_constant 0.1 i - 0.2
    (+ ``mean_shift``);
    y_mean 0.3 i; y_std 1 + 0.25 i; the kernel family cycles over ``families`` (keys of FAMILIES).
    D = rand(N, d), or linspace(0, 1, N) with ``grid`` (d = 1); W = rand(S, m) + 0.05 with rows summing to 1;
    X = rand(B, d).  ``ns``: one n per output (cycled when shorter than m)."""
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    g = torch.Generator().manual_seed(int(seed))
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.double)  # noqa: E731
    models = []
    for i in range(m):
        n = ns[i % len(ns)]
        x = rand(n, d)
        y = torch.sin(3.0 * x.sum(-1) / math.sqrt(d) + i) + 0.1 * torch.randn(n, generator=g, dtype=torch.double)
        ls = (0.5 + 0.5 * rand(d)) * math.sqrt(d / 2.0)
        if lengthscale is not None:
            ls = torch.full((d,), float(lengthscale), dtype=torch.double)
        kind, nu = FAMILIES[families[i % len(families)]]
        models.append(SingleTaskGPState(x, y, ls, 1.0 + 0.5 * i, 1e-2 * (1 + i) if noise is None else float(noise),
                                        0.1 * i - 0.2 + mean_shift, kind, 2.5 if nu is None else nu, 0.3 * i, 1.0 + 0.25 * i))
    if grid:
        assert d == 1
        D = torch.linspace(0.0, 1.0, N, dtype=torch.double).reshape(N, 1)
    else:
        D = rand(N, d)
    W = rand(S, m) + 0.05
    W = W / W.sum(-1, keepdim=True)
    X = rand(B, d)
    return ModelListGPState(*models), D, W, X


def _row(id, m, d, ns, fam, N, S, B, targets, slots, split=1, stream=0, seed=0, **kw):
    return dict(id=id, m=m, d=d, ns=ns, fam=fam, N=N, S=S, B=B, targets=targets, slots=slots, split=split,
                stream=stream, seed=seed, kw=kw)


# The value+gradient case matrix (tests/test_gpu_grad_matrix.py on the device, tests/test_grad_matrix_oracle.py
# on the reference alone).  slots / stream / split: the envelope instantiation the row is there for
# (ForwardPlan.envelope_geometry): 2 / 8 / 17 / 33 register slots by N + 1 <= 128 / 512 / 1088 / 2112, streaming
# above that or when the gradient envelope's LDS exceeds 160 KiB; split = ceil(S / 8) workgroups per candidate.
GRAD_MATRIX = [
    # each kernel family alone, one lengthscale per dimension
    *[_row(f"family-{f}", 2, 3, (40, 40), (f,), 200, 8, 19, (None, 1), 8, seed=sd)
      for f, sd in zip(ALL_FAMILIES, (1, 12, 13, 14))],
    # output buckets M = 1, 3, 4, 8 (m = 5 pads the M = 8 records with zero components)
    _row("M1", 1, 2, (37,), ("M52",), 100, 1, 19, (None,), 2, seed=3),
    _row("M3-mixed", 3, 3, (37, 50, 23), ALL_FAMILIES, 150, 8, 19, (None, 2), 8, seed=22),
    _row("M4", 4, 4, (33, 48, 17, 64), ALL_FAMILIES, 150, 8, 19, (None, 0), 8, seed=5),
    _row("M8-padded-m5", 5, 2, (20, 31, 16, 45, 27), ALL_FAMILIES, 120, 8, 19, (None, 4), 2, seed=24),
    _row("M8-full", 8, 2, (20, 31, 16, 45, 27, 38, 18, 52), ALL_FAMILIES, 120, 8, 19, (None, 7), 2, seed=25),
    # dimension buckets DM = 2, 4, 8, 16 and their edges
    _row("d1", 2, 1, (25, 25), ("M52", "M32"), 60, 8, 19, (None, 0), 2, seed=31),
    *[_row(f"d{d}", 2, d, (64, 64), ("M52", "M32"), 200, 8, 19, (None, 0), 8, seed=sd)
      for d, sd in ((4, 3), (5, 4), (8, 8), (9, 40), (16, 47))],
    # more than two workgroups per candidate: ordered last-arriver sums
    _row("S24", 2, 3, (40, 40), ("M52", "M32"), 200, 24, 19, (None, 1), 8, split=3, seed=51),
    _row("S40-m3", 3, 3, (40, 40, 40), ("M52", "M32", "M12"), 200, 40, 19, (None, 1), 8, split=5, seed=52),
    # envelope instantiations
    _row("slots2-B1", 2, 2, (16, 17), ("M52", "RBF"), 9, 3, 1, (None,), 2, seed=2),
    _row("slots33", 2, 3, (40, 40), ("M52", "M32"), 1100, 8, 19, (None,), 33, seed=62),
    _row("stream-by-N", 2, 3, (40, 40), ("M52", "M32"), 2200, 8, 19, (None, 1), 0, stream=1, seed=63),
    # the gradient envelope's LDS (M d stage_len(n_pad) doubles of J rows) over 160 KiB at a small N: the forward
    # plan of the same model is staged (8 slots), the gradient plan streams
    _row("stream-by-LDS", 5, 6, (16, 20, 31, 25, 18), ALL_FAMILIES, 130, 8, 19, (None,), 0, stream=1, seed=64),
    _row("stream-by-LDS-m3", 3, 12, (160, 60, 90), ALL_FAMILIES, 130, 8, 19, (None, 0), 0, stream=1, seed=65),
    # n_pad > 256: the flush's second body
    _row("np272", 2, 3, (260, 40), ("M52", "RBF"), 150, 8, 19, (None, 0), 8, seed=32),
    # long envelopes (more lines than the flush queue's 128, more survivors than the hull's 125)
    _row("long-M12-m1", 1, 1, (6,), ("M12",), 1000, 3, 9, (None,), 17, seed=81, lengthscale=1.0, noise=0.1,
         grid=True, mean_shift=1.2),
    _row("long-M12-m2", 2, 1, (6, 6), ("M12",), 1000, 3, 9, (None,), 17, seed=3, lengthscale=1.0, noise=0.1,
         grid=True),
    _row("long-M32-m1", 1, 1, (12,), ("M32",), 1000, 3, 9, (None,), 17, seed=83, lengthscale=0.3, noise=1e-2,
         grid=True),
    _row("long-M32-m2", 2, 1, (12, 12), ("M32",), 1000, 3, 9, (None,), 17, seed=84, lengthscale=0.3, noise=1e-2,
         grid=True),
]
GRAD_ROWS = {r["id"]: r for r in GRAD_MATRIX}
GRAD_CASES = [(r["id"], t) for r in GRAD_MATRIX for t in r["targets"]]


def grad_row_problem(row, B=None):
    """grad_case of a GRAD_MATRIX row (``B`` overrides the row's candidate count)."""
    return grad_case(row["m"], row["d"], row["ns"], row["fam"], row["N"], row["S"], row["B"] if B is None else B,
                     row["seed"], **row["kw"])


# The forward case matrix (tests/test_gpu_forward_matrix.py on the device, tests/test_forward_matrix_oracle.py on
# the reference alone): the production forward (no kg_pairs: env_flat, the plan's top hint, env_top + env_span)
# in every output bucket M = 1, 2, 3, 4, 8 (m = 5 padded, and m = 8) times every envelope instantiation of
# launch_env_bucket<M, false>: 2 / 8 / 17 / 33 register slots and the streaming kernel.  N only lands the row in
# its bucket; n <= 64 per output, all different; d cycles over 2, 3, 4; the kernel families cycle over
# ALL_FAMILIES from another start in every column, so the M = 1 rows do not all run Matern-5/2; S = 8, B = 19,
# targets (None, m - 1).  Seeds are chosen on the oracle alone (test_forward_matrix_oracle.py states the
# conditions).  GRAD_MATRIX rows are reused where their shape is the cell's (M3-mixed, M4, M8-padded-m5, M8-full).
#
# The M = 8 bucket has no 33-slot forward: two staged record arrays of 64 * 33 * 8 doubles are 264 KiB, over the
# envelope's 160 KiB of LDS at any N, so every M = 8 plan with N + 1 > 1088 streams.  The cell is kept as the rows
# "M8p-N1100" / "M8f-N1100" (the N of the other buckets' 33-slot rows), which assert the streaming kernel there.
FORWARD_NS = {"M1": (37,), "M2": (40, 33), "M3": (37, 50, 23), "M4": (33, 48, 17, 64),
              "M8p": (20, 31, 16, 45, 27), "M8f": (20, 31, 16, 45, 27, 38, 18, 52)}
FORWARD_GEOMETRIES = (("slots2", 100, 2, 0), ("slots8", 200, 8, 0), ("slots17", 600, 17, 0),
                      ("slots33", 1100, 33, 0), ("stream", 2200, 0, 1))
FORWARD_REUSED = {("M3", "slots8"): "M3-mixed", ("M4", "slots8"): "M4", ("M8p", "slots2"): "M8-padded-m5",
                  ("M8f", "slots2"): "M8-full"}
# (seed, grad_case overrides) picked on the oracle so that every bucket has a staged row with at least 8 flat pairs
# (env_flat) next to at least 8 walked pairs with KG > 0 (test_forward_matrix_oracle.py); elsewhere the seed is
# 300 + 10 * bucket + column.  noise = 1e-3 for every output (the default is 1e-2 (1 + i)) shrinks the candidate's
# posterior deviation, which is line 0's slope: what a pair needs to be flat.  With target None that takes every
# output's deviation small at once: 8 such pairs at M = 1 (one candidate, all flat) and M = 2, at most 2 in the
# larger buckets over the few hundred seeds tried per row, whose flat pairs are the target m - 1 ones.
FORWARD_PICKS = {"M1-slots2": (49, {}), "M2-slots17": (8, dict(noise=1e-3)), "M3-slots17": (13, dict(noise=1e-3)),
                 "M4-slots2": (3, dict(noise=1e-3)), "M8p-slots8": (120, {}), "M8f-slots8": (23, dict(noise=1e-3))}


def _forward_matrix():
    rows = []
    for bi, (mk, ns) in enumerate(FORWARD_NS.items()):
        m = len(ns)
        for gi, (gk, N, slots, stream) in enumerate(FORWARD_GEOMETRIES):
            reused = FORWARD_REUSED.get((mk, gk))
            if reused is not None:
                row = dict(GRAD_ROWS[reused], targets=(None, m - 1), cell=(mk, gk))
            else:
                rid = f"{mk}-{gk}"
                if m > 4 and gk == "slots33":  # no 33-slot kernel in the M = 8 bucket: streams by its LDS
                    rid, slots, stream = f"{mk}-N1100", 0, 1
                fam = ALL_FAMILIES[gi % 4:] + ALL_FAMILIES[:gi % 4]
                seed, kw = FORWARD_PICKS.get(rid, (300 + 10 * bi + gi, {}))
                row = _row(rid, m, 2 + (bi + gi) % 3, ns, fam, N, 8, 19, (None, m - 1), slots, stream=stream,
                           seed=seed, **kw)
                row["cell"] = (mk, gk)
            rows.append(row)
    # three and five workgroups per candidate (S = 24, 40) in the M = 3 and M = 4 buckets
    rows.append(dict(_row("M3-S24", 3, 3, FORWARD_NS["M3"], ALL_FAMILIES, 200, 24, 19, (None, 2), 8, split=3,
                          seed=371), cell=("M3", "split3")))
    rows.append(dict(_row("M4-S40", 4, 2, FORWARD_NS["M4"], ALL_FAMILIES, 600, 40, 19, (None, 3), 17, split=5,
                          seed=372), cell=("M4", "split5")))
    return rows


FORWARD_MATRIX = _forward_matrix()
FORWARD_ROWS = {r["id"]: r for r in FORWARD_MATRIX}
FORWARD_CASES = [(r["id"], t) for r in FORWARD_MATRIX for t in r["targets"]]

# streaming forwards over lists longer than LIST_CAP_STREAM = 512 (d = 1 grids in the long-M12 style): M = 1 takes
# the older streaming path (env_extremes_stream / refine_stream / walk_stream), M = 2 the staged chain and then
# its overflow.  N is the smallest tried at which some pair's envelope exceeds 512 lines on the oracle.
FORWARD_LONG = [
    _row("long-stream-m1", 1, 1, (6,), ("M12",), 2600, 3, 9, (None,), 0, stream=1, seed=81, lengthscale=1.0,
         noise=0.1, grid=True, mean_shift=1.2),
    _row("long-stream-m2", 2, 1, (6, 6), ("M12",), 3000, 3, 9, (None,), 0, stream=1, seed=3, lengthscale=1.0,
         noise=0.1, grid=True),
]
FORWARD_LONG_ROWS = {r["id"]: r for r in FORWARD_LONG}

HINT_STATES = ("line0", "grid-unique", "grid-tied", "equal")


def forward_classes(a, b, pairs=None):
    """Which branches of the production forward a set of oracle lines [B, S, L] (line 0: the candidate) asks for,
    per (candidate, scalarisation) pair.  A classifier of inputs, not a tolerance.  -> dict of [B, S] tensors:

      state   : index into HINT_STATES, the plan's top hint (dkg_device.h envelope_body): with a0 line 0's
                intercept, A1 the largest intercept of lines k >= 1 and c1 how many of them attain it:
                a0 > A1 (line 0 is T), a0 < A1 with c1 == 1 (that grid line is T), a0 < A1 with c1 > 1 (tied: no
                hint, env_top finds T) and a0 == A1 (no hint);
      flat    : env_flat's predicate restated: with T = (max a, ties: min b), every line that is not an exact
                copy of T has fma(48, |b - b_T|, a - a_T) <= 2^-40 (a - a_T) (the sign as the kernel has it:
                a - a_T <= 0), so the pair's KG is exactly 0 and the kernel does not walk it;
      kg_zero : the reference KG of the pair is exactly 0.0 (``pairs``: the oracle's kg_pairs_from_lines of the
                same lines when the caller has them already)."""
    from oracle.discretekg import kg_pairs_from_lines

    a0 = a[..., 0]
    A1 = a[..., 1:].amax(-1)
    c1 = (a[..., 1:] == A1[..., None]).sum(-1)
    state = torch.where(a0 > A1, 0, torch.where(a0 == A1, 3, torch.where(c1 == 1, 1, 2)))
    aT = a.amax(-1, keepdim=True)
    bT = torch.where(a == aT, b, torch.inf).amin(-1, keepdim=True)
    da = a - aT
    # the kernel's two fmas written as products and sums: two more roundings of 2^-53 (|da| + 48 |b - bT|), which
    # can move only a pair within 2^-51 |da| of a boundary that itself stands 2^-40 |da| inside the true one
    v = 48.0 * (b - bT).abs() + da
    worst = torch.where((a == aT) & (b == bT), -torch.inf, v - 2.0 ** -40 * da).amax(-1)
    flat = worst <= 0.0
    if pairs is None:
        pairs = kg_pairs_from_lines(a, b)
    return {"state": state, "flat": flat, "kg_zero": pairs == 0.0}


def forward_row_problem(row, B=None):
    """grad_case of a FORWARD_MATRIX / FORWARD_LONG row."""
    return grad_row_problem(row, B)


# Inputs for the states of the plan's top hint no matrix row reaches in numbers (every row is almost all
# "grid-unique"): per output bucket and slot count, a grad_case base (S = 8, B = 19; N lands the slot bucket and is
# small enough for line 0 to beat every grid intercept now and then: the chance falls with N, so the M = 8
# bucket's 17-slot case takes the smallest N of that bucket) and three edits of it (hint_case).
HINT_NS = {k: FORWARD_NS[k] for k in ("M1", "M3", "M4", "M8p")}
HINT_N = {2: 40, 8: 300, 17: 700}
HINT_KINDS = ("line0", "tied", "equal", "equal-tied")
HINT_POOL = 2000
# seeds (the default is 500 + 10 * bucket + slots) moved until the pool holds at least 8 pairs with a0 > A1
HINT_SEEDS = {("M1", 8): 1, ("M1", 17): 3, ("M4", 17): 1}


def _top_rows(om, X, D, W):
    """Per scalarisation, the row of D whose line has the largest intercept (the oracle's; target-independent)."""
    from oracle.discretekg import lines_batched

    return lines_batched(om, X[:1], D, W, None)[0][0, :, 1:].argmax(-1)


def hint_case(mk, slots, kind):
    """-> (ModelListGPState, D, W, X [19, d]) whose oracle lines reach a state of the top hint:

      line0      : the 10 candidates of a pool of HINT_POOL uniform ones with the most scalarisations in which
                   line 0's intercept exceeds every grid line's (a0 > A1), and the 9 with the fewest;
      tied       : D with the argmax-intercept rows of scalarisations 0..3 appended again: their top grid
                   intercept is attained twice (c1 = 2), so the plan gives no hint there;
      equal      : candidates 0 and 1 placed on the argmax rows of scalarisations 0 and 1: line 0 is an exact copy
                   of the top grid line (a0 == A1);
      equal-tied : both edits."""
    from oracle.discretekg import lines_batched

    m = len(HINT_NS[mk])
    bi = list(FORWARD_NS).index(mk)
    N = 512 if (mk, slots) == ("M8p", 17) else HINT_N[slots]
    args = (m, 2 + (bi + slots) % 3, HINT_NS[mk], ALL_FAMILIES, N, 8)
    seed = HINT_SEEDS.get((mk, slots), 500 + 10 * bi + slots)
    state, D, W, X = grad_case(*args, 19, seed)
    om = to_oracle(state)
    if kind == "line0":
        pool = grad_case(*args, HINT_POOL, seed)[3]
        a0 = lines_batched(om, pool, D[:1], W, None)[0][..., 0]                   # [pool, S]
        A1 = lines_batched(om, pool[:1], D, W, None)[0][0, :, 1:].amax(-1)        # [S]
        order = torch.sort((a0 > A1).sum(-1), descending=True, stable=True).indices
        return state, D, W, torch.cat([pool[order[:10]], pool[order[-9:]]])
    top = _top_rows(om, X, D, W)
    if kind in ("equal", "equal-tied"):
        X = X.clone()
        X[0], X[1] = D[top[0]], D[top[1]]
    if kind in ("tied", "equal-tied"):
        D = torch.cat([D, D[torch.unique(top[:4])]])
    return state, D, W, X


def assert_envelopes_are_reference_walk(a, b, hull):
    """On lines a, b [B, S, L] a plan built (device tensors, exported bit for bit by dkg_plan_lines): the device
    walk (calculate_epigraph_indices_batched) returns the oracle walk's indices and intersections exactly, and the
    forward's envelope sizes ``hull`` [B, S] (dkg_plan_hull_sizes) equal the walk's -- every (candidate,
    scalarisation) pair.  -> the envelope sizes, sorted."""
    from dkg_amd import calculate_epigraph_indices_batched
    from oracle.discretekg import calculate_epigraph_indices as ref_epigraph

    B, S, L = a.shape
    idx, xs, cnt = calculate_epigraph_indices_batched(a, b)
    ac, bc, idx, xs, cnt, hull = a.cpu(), b.cpu(), idx.cpu(), xs.cpu(), cnt.cpu(), hull.cpu()
    sizes = []
    for i in range(B):
        for j in range(S):
            ri, rx = ref_epigraph(ac[i, j], bc[i, j])
            m = len(ri)
            assert int(cnt[i, j]) == m and int(hull[i, j]) == m, (i, j, int(cnt[i, j]), int(hull[i, j]), m)
            assert torch.equal(idx[i, j, :m], ri), (i, j)
            assert torch.equal(xs[i, j, : m - 1], rx), (i, j)
            sizes.append(m)
    return sorted(sizes)


def oracle_value_and_grad(om, X, D, W, target):
    """KG [B] and dKG/dX [B, d] of the batched oracle by torch.autograd."""
    from oracle.discretekg import discrete_kg_batched

    Xr = X.clone().requires_grad_(True)
    kg, _ = discrete_kg_batched(om, Xr, D, W, target)
    (g,) = torch.autograd.grad(kg.sum(), Xr)
    return kg.detach(), g


def load_golden(name: str):
    """tests/golden/<name>.npz -> (state, oracle ModelList, D, W, X, arrays dict)."""
    import os

    import numpy as np

    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{name}.npz")
    z = dict(np.load(path))
    t = {k: torch.from_numpy(v) for k, v in z.items()}
    state = ModelListGPState(*[
        SingleTaskGPState(t["train_x"], t["train_y"][:, i], t["lengthscale"][i], float(t["outputscale"][i]),
                          float(t["noise"][i]), float(t["mean_constant"][i]))
        for i in range(t["train_y"].shape[1])])
    return state, to_oracle(state), t["D"], t["W"], t["X"], t
