"""The cases of the hypervolume knowledge gradient tests, built on the CPU from seeds (no device, no global RNG),
with their reference values (tests/hvkg_oracle.py on oracle.gp) computed once and shared.

A case: a fitted model (helpers.grad_case; Standardize taken off where ``std`` is False), base samples
``z [Nf, m]`` (standard normals), a mask, B one-shot points ``X_full [B, 1 + Nf Np, d]`` (uniform), a reference
point and the two scalars.  The reference point is taken from the oracle's own fantasised means: ``refq = 0`` puts it
a tenth of each objective's range below the smallest mean (every point counts), ``refq > 0`` at that quantile of
each objective (some points fall below ref in one objective or in all, so the kernels' validity test is exercised).

Conditions on the inputs (asserted here, on the reference alone): every noise is at least 1e-4, and for the
gradient assertions the kink condition holds: within every fantasy the coordinates differ pairwise, and from ref, by
at least 1e-6 of that objective's range.  Nearer a kink two correct implementations may take different branches.
"""

from __future__ import annotations

import functools

import torch

import hvkg_oracle
from helpers import grad_case

KINK_MIN = 1e-6
NOISE_MIN = 1e-4

# The shapes at which the kernels' loops repeat or branch (csrc/dkg_hvkg.hip).  The triangular products give wave w
# the row tiles w, w + 4, ... of the pad16(n) / 16 and the 8-column words w, w + 4, ...; the fantasy stage takes 16
# points per workgroup, 4 per wave, lanes over the training rows in rounds of 64; the hypervolume stage holds one
# fantasy's points in one wave; the finish stage strides 256 threads over the fantasy points and the training rows.
CASES = {
    # one tile, one word; one fantasy point; d = 1 in DM = 2; Matern-1/2 (the joint rows stay within cdist's exact path)
    "n5-d1-m2-f1p1": dict(m=2, d=1, ns=(5, 7), fam=("M12", "M52"), std=False, mask=(0,), Nf=1, Np=1, B=17, seed=41,
                          refq=0.0, current=None, costs=None),
    # two tiles; mask {1}: output 0 takes the unobserved path; current and cost set
    "n17-d2-m2-f2p2": dict(m=2, d=2, ns=(17, 13), fam=("M32", "RBF"), std=True, mask=(1,), Nf=2, Np=2, B=5, seed=42,
                           refq=0.0, current=0.3, costs=(1.5, 2.5)),
    # 9 tiles (3 per wave, wave 0 alone on the last), three training-row rounds; m = 3 slabs; d = 6 in DM = 8; all
    # outputs observed; ref at the 0.2 quantile
    "n130-d6-m3-f3p4": dict(m=3, d=6, ns=(130, 61, 17), fam=("M52", "RBF", "M32"), std=True, mask=(0, 1, 2), Nf=3, Np=4,
                            B=5, seed=43, refq=0.2, current=0.1, costs=(1.0, 2.0, 4.0)),
    # 253 + 3 = 256 rows: 16 tiles with no padded row; 72 fantasy points: 5 workgroups of the fantasy stage, more
    # than one wave of points; B = 17 restarts
    "n256-d2-m2-f9p8": dict(m=2, d=2, ns=(256, 139), fam=("RBF", "M32"), std=True, mask=(0, 1), Nf=9, Np=8, B=17,
                            seed=44, refq=0.1, current=None, costs=None),
    # the reference preset's shape: 321 rows (the finish stage's second stride over the fantasy points)
    "n64-d2-m2-f32p10": dict(m=2, d=2, ns=(64, 64), fam=("M52",), std=True, mask=(0,), Nf=32, Np=10, B=5, seed=45,
                             refq=0.05, current=0.2, costs=(1.0, 3.0)),
    # the limits: 64 fantasies of 32 points, 2049 rows; d = 16 fills DM = 16; mask {2}; all four families over m = 3
    "n33-d16-m3-f64p32": dict(m=3, d=16, ns=(33, 21, 40), fam=("M12", "RBF", "M52"), std=False, mask=(2,), Nf=64,
                              Np=32, B=1, seed=50, refq=0.3, current=None, costs=None),
    # n = 1024: every tile and word of every wave, 16 training-row rounds, the largest LDS requests
    "n1024-d2-m2-f1p2": dict(m=2, d=2, ns=(1024, 1000), fam=("M32", "M52"), std=True, mask=(0, 1), Nf=1, Np=2, B=1,
                             seed=47, refq=0.0, current=None, costs=None),
}


def mask_bits(mask) -> int:
    return sum(1 << i for i in mask)


def case_cost(c) -> float:
    return 1.0 if c["costs"] is None else float(sum(c["costs"][i] for i in c["mask"]))


def build_state(c):
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    state, _, _, _ = grad_case(c["m"], c["d"], c["ns"], c["fam"], 4, 2, 1, c["seed"])
    if not c["std"]:
        state = ModelListGPState(*[SingleTaskGPState(o.train_x, o.train_y, o.lengthscale, o.outputscale, o.noise,
                                                     o.mean_constant, o.kernel, o.nu, 0.0, 1.0) for o in state.models])
    assert all(o.noise >= NOISE_MIN for o in state.models)
    return state


@functools.lru_cache(maxsize=None)
def problem(cid: str):
    """-> (state, z [Nf, m], X_full [B, 1 + Nf Np, d], ref [m])."""
    c = CASES[cid]
    state = build_state(c)
    g = torch.Generator().manual_seed(2000 + c["seed"])
    z = torch.randn(c["Nf"], c["m"], generator=g, dtype=torch.double)
    X = torch.rand(c["B"], 1 + c["Nf"] * c["Np"], c["d"], generator=g, dtype=torch.double)
    with torch.no_grad():
        Y = hvkg_oracle.fantasy_means(hvkg_oracle.models_of(state), X, z, mask_bits(c["mask"]), c["Nf"], c["Np"])
    flat = Y.reshape(-1, c["m"])
    if c["refq"] > 0:
        ref = torch.quantile(flat, c["refq"], dim=0)
    else:
        ref = flat.min(0).values - 0.1 * (flat.max(0).values - flat.min(0).values + 1e-3)
    return state, z, X, ref


@functools.lru_cache(maxsize=None)
def reference(cid: str, reverse: bool = False):
    """{"Y": [B, Nf, Np, m], "acq": [B], "scale": [B] (mean_f HV_f / cost), "grad": [B, rows, d], "kink": float}."""
    c = CASES[cid]
    state, z, X, ref = problem(cid)
    models = hvkg_oracle.models_of(state, reverse=reverse)
    Xr = X.clone().requires_grad_(True)
    Y = hvkg_oracle.fantasy_means(models, Xr, z, mask_bits(c["mask"]), c["Nf"], c["Np"])
    acq, scale = hvkg_oracle.acq_from_means(Y, ref, 0.0 if c["current"] is None else c["current"], case_cost(c))
    (grad,) = torch.autograd.grad(acq.sum(), Xr)
    kink = hvkg_oracle.kink_margin(Y, ref)
    assert kink >= KINK_MIN, f"{cid}: kink margin {kink:.3g} < {KINK_MIN}"
    return {"Y": Y.detach(), "acq": acq.detach(), "scale": scale, "grad": grad, "kink": kink}


def spreads(cid: str):
    """(largest |acq - acq_reversed|, largest |grad - grad_reversed|): the reference side's rounding floor."""
    a, b = reference(cid), reference(cid, True)
    return float((a["acq"] - b["acq"]).abs().max()), float((a["grad"] - b["grad"]).abs().max())


def bounds(cid: str):
    """The asserted bounds: value ``1e-6 mean_f HV_f / cost + 4 spread_v`` per restart, gradient
    ``1e-6 max_j |g_j| + 4 spread_g`` per restart."""
    r = reference(cid)
    sv, sg = spreads(cid)
    B = r["acq"].shape[0]
    return 1e-6 * r["scale"] + 4.0 * sv, 1e-6 * r["grad"].reshape(B, -1).abs().max(dim=1).values + 4.0 * sg


# ---- the optimisation tests' problem ---------------------------------------------------------------------------
# The SMOKE preset's sizes on the reference's test model.  Every point an optimisation evaluates is recorded
# (Recorder) and replayed on the restatement (replay): the visited points are compared, not two trajectories, which
# a non-smooth objective may separate.  Evaluations that fail the kink condition are skipped; tests/test_hvkg_host.py
# runs the restatement-driven optimisation of this problem on the CPU and asserts that at most one in ten does
# (the seed below was chosen so).
OPT = dict(num_pareto=2, num_fantasies=2, num_restarts=2, raw_samples=4, curr_opt_num_restarts=2,
           curr_opt_raw_samples=8, batch_limit=2, max_iter=20, seed=3)
OPT_COSTS = (1.0, 2.0)
SKIP_CAP = 0.1


@functools.lru_cache(maxsize=None)
def opt_problem():
    """-> (state, ref [m], z [Nf, m], ranges [m]: each objective's range of the posterior mean over a Sobol pool)."""
    from dkg_amd.utils import sobol_draw
    from helpers import to_state
    from oracle.fit import make_reference_test_model

    state = to_state(make_reference_test_model(use_noise=True))
    assert all(o.noise >= NOISE_MIN for o in state.models)
    pool = sobol_draw(2, 64, 17, torch.double)
    with torch.no_grad():
        mean = hvkg_oracle.posterior_means(hvkg_oracle.models_of(state), pool[None])[0, 0]     # [64, m]
    ranges = mean.max(0).values - mean.min(0).values
    ref = mean.min(0).values - 0.1 * ranges
    z = torch.randn(OPT["num_fantasies"], 2, generator=torch.Generator().manual_seed(23), dtype=torch.double)
    return state, ref, z, ranges


class Recorder:
    """Wraps an acquisition and records every evaluation: (mask bits or None, X, values, gradient or None, whether
    it was a value-only call)."""

    def __init__(self, inner, records, tag):
        self.inner, self.records, self.tag = inner, records, tag
        if hasattr(inner, "value_and_grad_host"):
            self.value_and_grad_host = self._value_and_grad_host

    @property
    def X_evaluation_mask(self):
        return self.inner.X_evaluation_mask

    @X_evaluation_mask.setter
    def X_evaluation_mask(self, mask):
        self.inner.X_evaluation_mask = mask

    def _bits(self):
        mask = getattr(self.inner, "X_evaluation_mask", None)
        return None if mask is None else sum(1 << i for i, f in enumerate(mask.reshape(-1).tolist()) if f)

    def extract_candidates(self, X):
        return self.inner.extract_candidates(X)

    def _value_and_grad_host(self, X):
        val, grad = self.inner.value_and_grad_host(X)
        self.records.append(dict(tag=self.tag, bits=self._bits(), X=X.detach().clone(), val=val.clone(),
                                 grad=grad.clone(), value_only=False))
        return val, grad

    def __call__(self, X):
        val = self.inner(X)
        self.records.append(dict(tag=self.tag, bits=self._bits(), X=X.detach().clone(), val=val.detach().clone(),
                                 grad=None, value_only=True))
        return val


def replay(records, costs=None, current=None, check=True):
    """Re-evaluates every recorded restart on the restatement.  -> (evaluations, skipped for the kink condition,
    worst value err / bound, worst gradient err / bound); with ``check`` the two bounds are asserted."""
    state, ref, z, ranges = opt_problem()
    fwd, rev = hvkg_oracle.models_of(state), hvkg_oracle.models_of(state, reverse=True)
    total = skipped = 0
    worst_v = worst_g = 0.0
    for rec in records:
        X = rec["X"].reshape((-1,) + tuple(rec["X"].shape[-2:])).double()
        for b in range(X.shape[0]):
            total += 1
            out = []
            for models in (fwd, rev):
                Xr = X[b:b + 1].clone().requires_grad_(True)
                if rec["tag"] == "value_function":
                    Y = hvkg_oracle.posterior_means(models, Xr)
                    acq, scale = hvkg_oracle.acq_from_means(Y, ref)
                else:
                    bits = 3 if rec["bits"] is None else rec["bits"]
                    cost = 1.0 if costs is None else sum(c for i, c in enumerate(costs) if (bits >> i) & 1)
                    Y = hvkg_oracle.fantasy_means(models, Xr, z, bits, OPT["num_fantasies"], OPT["num_pareto"])
                    acq, scale = hvkg_oracle.acq_from_means(Y, ref, 0.0 if current is None else float(current), cost)
                (g,) = torch.autograd.grad(acq.sum(), Xr)
                out.append((acq.detach()[0], g[0], scale[0], Y))
            (a, g, scale, Y), (a2, g2, _, _) = out
            if hvkg_oracle.kink_margin(Y, ref, ranges) < KINK_MIN:
                skipped += 1
                continue
            if not check:
                continue
            vtol = 1e-6 * float(scale) + 4.0 * abs(float(a - a2))
            verr = abs(float(rec["val"].reshape(-1)[b]) - float(a))
            worst_v = max(worst_v, verr / max(vtol, 1e-300))
            assert verr <= vtol, (rec["tag"], rec["bits"], b, verr, vtol)
            if rec["grad"] is not None:
                gtol = 1e-6 * float(g.abs().max()) + 4.0 * float((g - g2).abs().max())
                gerr = float((rec["grad"].reshape(X.shape)[b] - g).abs().max())
                worst_g = max(worst_g, gerr / max(gtol, 1e-300))
                assert gerr <= gtol, (rec["tag"], rec["bits"], b, gerr, gtol)
    return total, skipped, worst_v, worst_g
