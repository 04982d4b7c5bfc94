"""The committed cases of the joint entropy search tests, built on the CPU from seeds (no device, no global
RNG), with their reference values (tests/jes_oracle.py on oracle.gp) computed once and shared.

A case: a fitted model (helpers.grad_case), P Pareto samples (ps_p: k_p points spread over the non-dominated
ones, in the first two objectives, of the model's posterior mean on a pool of 128 uniform points; pf_p the mean
there plus 0.1 y_std |noise|: a front that dominates most of the posterior, as a sampled one does), boxes and
candidates.  Boxes: for the first two objectives
the staircase of ``compute_sample_box_decomposition``; further objectives are bounded by (-1e10, max_p pf + 2
y_std]; the first box of sample 0 is then cut along its last objective until the sample has J boxes (a finer
partition of the same region), so the samples differ in their box counts and the others are padded with [0, 0]
boxes.  Candidates: uniform, with candidate 0 on a Pareto-set point of sample 0 and candidate 1 on a training
point of output 0.

Condition on the inputs (asserted here, on the reference alone): every (candidate, sample) has
W = sum_j W_j >= 1e-3; the seeds below were moved until it held.

Two sets: CASES (families, noise levels, Standardize on and off; the reference-side spreads that set the bounds
of tests/test_gpu_jes.py are taken over these alone) and SHAPE_CASES (the shapes at which the kernels' loops
repeat and their limits; see the comment there).  ``problem`` and ``reference`` take an id of either.
"""

from __future__ import annotations

import functools

import torch

import jes_oracle
from helpers import ALL_FAMILIES, grad_case, to_oracle

W_MIN = 1e-3
NEG = -1e10
POOL = 128

# id -> m, d, ns, families, noise, standardize, P, k_p, J, B, seed
CASES = {
    "m1-d1-P1-J1": dict(m=1, d=1, ns=(13,), fam=("M52",), noise=1e-2, std=True, ks=(1,), J=1, B=17, seed=11),
    "m2-d2-P3-J6-noise1e-8": dict(m=2, d=2, ns=(13, 21), fam=("M12", "M32"), noise=1e-8, std=False, ks=(1, 3, 5), J=6,
                                  B=40, seed=15),
    "m3-d6-P3-J70": dict(m=3, d=6, ns=(37, 50, 23), fam=("M52", "RBF", "M32"), noise=1e-2, std=True, ks=(3, 5, 1),
                         J=70, B=17, seed=16),
    "m8-d2-P1-J6": dict(m=8, d=2, ns=(20, 31, 17, 45, 27, 38, 18, 52), fam=ALL_FAMILIES, noise=1e-2, std=True,
                        ks=(3,), J=6, B=17, seed=14),
}
# the optimisation tests' problem (not among the cases the spreads are taken over)
OPT_CASE = "m2-d2-opt"
EXTRA_CASES = {OPT_CASE: dict(m=2, d=2, ns=(13, 21), fam=("M52", "M32"), noise=1e-2, std=True, ks=(1, 3, 5), J=5, B=4,
                              seed=15)}
# The shapes at which the kernels' loops repeat (csrc/dkg_jes.hip), kept apart from CASES: the recorded spreads
# are taken over CASES alone, and test_jes_host.py asserts that none of these exceeds them.  The moments stage
# gives wave w the column tiles 8 s + (s odd ? 7 - w : w) of Q, T = pad16(n) / 16 of them; the entropy stage
# gives wave w the states w, w + 4, ... of the P + 1 and walks the boxes in rounds of 64.  All with noise 1e-2
# and Standardize; Matern-1/2 outputs keep n + max(ks) + 1 <= 25 (the oracle's exact-cdist rule), so the large-n
# outputs are of the other families.  ``overlap``: every sample's boxes stated twice, so that sum_j W_j doubles
# and the clamp W = min(sum_j W_j, 1) binds for most (candidate, sample) pairs and not for the others.
SHAPE_CASES = {
    # state 0 has T = 8, the conditioned states T = 9 (tile 8 is wave 7's alone, at s = 1); P = 4: wave 0 takes
    # two states; d = 3 in DM = 4; B = 16: no clamped candidate row
    "n127-P4-d3": dict(m=1, d=3, ns=(127,), fam=("M52",), noise=1e-2, std=True, ks=(3, 3, 3, 3), J=1, B=16, seed=31),
    # 253 + (1, 2, 3 | 4, 5) rows: T = 16 | 17 (tile 16 is wave 0's alone, at s = 2); 139 + 5 = 144 rows exactly
    # (T = 9 with no padded row); 8 states: two full rounds; d = 4 fills DM = 4
    "n253-P7-d4": dict(m=2, d=4, ns=(253, 139), fam=("RBF", "M32"), noise=1e-2, std=True, ks=(3, 5, 1, 4, 2, 5, 3),
                       J=6, B=17, seed=33),
    # 1019 + 5 = 1024 rows: every s on every wave, 32 rounds of the slab fill, the largest LDS request
    "n1019-k5": dict(m=1, d=2, ns=(1019,), fam=("M32",), noise=1e-2, std=True, ks=(5,), J=1, B=5, seed=31),
    # M = 8 with three padded outputs; d = 9 in DM = 16; J = 64: one full round, no clamped lane
    "m5-d9-J64": dict(m=5, d=9, ns=(20, 31, 17, 45, 27), fam=ALL_FAMILIES, noise=1e-2, std=True, ks=(3, 5, 1, 2),
                      J=64, B=16, seed=31),
    # M = 8 with one padded output; d = 8 fills DM = 8; J = 65: a second round of one lane
    "m7-d8-J65": dict(m=7, d=8, ns=(20, 31, 17, 45, 27, 38, 18), fam=("RBF", "M32", "M12", "M52"), noise=1e-2,
                      std=True, ks=(3,), J=65, B=5, seed=31),
    # M = 4 exactly; d = 16 fills DM = 16 (17 slab passes); 10 states: three rounds; J = 129: three box rounds
    "m4-d16-P9-J129": dict(m=4, d=16, ns=(33, 48, 17, 61), fam=ALL_FAMILIES, noise=1e-2, std=True,
                           ks=(3, 5, 1, 2, 4, 3, 5, 2, 4), J=129, B=5, seed=31),
    # DKG_JES_MAX_SAMPLES: 65 states
    "m1-P64": dict(m=1, d=1, ns=(13,), fam=("M52",), noise=1e-2, std=True, ks=(1, 2, 3, 4) * 16, J=1, B=2, seed=31),
    # DKG_JES_MAX_BOXES: 64 box rounds
    "m2-J4096": dict(m=2, d=1, ns=(13, 21), fam=("M52", "M32"), noise=1e-2, std=True, ks=(3,), J=4096, B=2, seed=31),
    # sum_j W_j on both sides of 1 (J = 6 stated twice: 12 boxes)
    "m2-overlap": dict(m=2, d=2, ns=(13, 21), fam=("M52", "M32"), noise=1e-2, std=True, ks=(1, 3, 5), J=6, B=17,
                       seed=33, overlap=True),
}
ESTIMATORS = ("LB", "LB2")


def case(cid: str) -> dict:
    for cases in (CASES, SHAPE_CASES, EXTRA_CASES):
        if cid in cases:
            return cases[cid]
    raise KeyError(cid)


def targets_of(m: int):
    return sorted({None, 0, m - 1}, key=lambda t: -1 if t is None else t)


def make_bounds(fronts, y_std, J: int) -> torch.Tensor:
    from dkg_amd.jes import compute_sample_box_decomposition

    m = fronts[0].shape[1]
    base = compute_sample_box_decomposition([pf[:, :2] for pf in fronts])      # [P, 2, J0, min(m, 2)]
    P, _, J0, m2 = base.shape
    per = []
    for p in range(P):
        k = int((base[p, 1, :, 0] != base[p, 0, :, 0]).sum())                  # boxes that are not padding
        b = torch.empty(2, k, m, dtype=torch.double)
        b[:, :, :m2] = base[p, :, :k]
        for i in range(m2, m):
            b[0, :, i] = NEG
            b[1, :, i] = max(float(pf[:, i].max()) for pf in fronts) + 2.0 * y_std[i]
        if p == 0 and k < J:                                                    # cut box 0 along objective m - 1
            extra = J - k
            i, hi = m - 1, float(b[1, 0, m - 1])
            cuts = [hi - 2.0 * y_std[i] * t / extra for t in range(extra + 1)]  # hi = cuts[0] > ... > cuts[extra]
            pieces = b[:, :1].repeat(1, extra + 1, 1)
            for t in range(extra):
                pieces[1, t, i], pieces[0, t, i] = cuts[t], cuts[t + 1]
            pieces[1, extra, i] = cuts[extra]
            b = torch.cat([pieces, b[:, 1:]], dim=1)
        per.append(b)
    Jmax = max(b.shape[1] for b in per)
    out = torch.zeros(P, 2, Jmax, m, dtype=torch.double)
    for p, b in enumerate(per):
        out[p, :, : b.shape[1]] = b
    return out


@functools.lru_cache(maxsize=None)
def problem(cid: str):
    """-> (state, pareto_sets, pareto_fronts, bounds [P, 2, J, m], X [B, d])."""
    from dkg_amd.model import ModelListGPState, SingleTaskGPState

    c = case(cid)
    state, _, _, X = grad_case(c["m"], c["d"], c["ns"], c["fam"], 4, 2, c["B"], c["seed"], noise=c["noise"])
    if not c["std"]:
        state = ModelListGPState(*[SingleTaskGPState(o.train_x, o.train_y, o.lengthscale, o.outputscale, o.noise,
                                                     o.mean_constant, o.kernel, o.nu, 0.0, 1.0) for o in state.models])
    om = to_oracle(state)
    g = torch.Generator().manual_seed(1000 + c["seed"])
    sets, fronts = [], []
    for k in c["ks"]:
        pool = torch.rand(POOL, c["d"], generator=g, dtype=torch.double)
        mean = torch.stack([torch.cat([o.posterior(pool[r:r + 8])[0] for r in range(0, POOL, 8)])
                            for o in om.models], dim=1)                         # [POOL, m]
        m2 = mean[:, :2]
        dominated = ((m2[None] >= m2[:, None]).all(-1) & (m2[None] > m2[:, None]).any(-1)).any(1)
        nd = torch.nonzero(~dominated).reshape(-1)
        nd = nd[torch.argsort(m2[nd, 0])]
        pick = nd[torch.linspace(0, len(nd) - 1, min(k, len(nd))).round().long()]
        if len(pick) < k:                                                       # a short front: any other points
            rest = torch.tensor([r for r in range(POOL) if r not in set(pick.tolist())])[: k - len(pick)]
            pick = torch.cat([pick, rest])
        ps = pool[pick]
        ys = torch.tensor([o.y_std for o in om.models], dtype=torch.double)
        pf = mean[pick] + 0.1 * ys * torch.randn(k, len(ys), generator=g, dtype=torch.double).abs()
        sets.append(ps)
        fronts.append(pf)
    bounds = make_bounds(fronts, [o.y_std for o in state.models], c["J"])
    assert bounds.shape[2] == max(c["J"], 1), (cid, bounds.shape)
    if c.get("overlap"):
        bounds = torch.cat([bounds, bounds], dim=2)
    X = X.clone()
    X[0] = sets[0][0]
    if X.shape[0] > 1:
        X[1] = state.models[0].train_x[3]
    return state, sets, fronts, bounds, X


@functools.lru_cache(maxsize=None)
def reference(cid: str, reverse: bool = False):
    """The restatement on the oracle's moments: {"moments": (mu, v, tau) [S, m, B], (est, target): (acq [B],
    dacq/dX [B, d])} for every estimator and target of the case.  ``reverse``: every output's training rows
    in reversed order (the same function, another summation order: the reference side's rounding floor)."""
    state, sets, fronts, bounds, X = problem(cid)
    models = jes_oracle.augmented_models(state, sets, fronts, reverse=reverse)
    Xr = X.clone().requires_grad_(True)
    mu, v, tau = jes_oracle.moments(models, Xr)
    out = {"moments": (mu.detach(), v.detach(), tau.detach())}
    for est in ESTIMATORS:
        for t in targets_of(len(state.models)):
            acq, W = jes_oracle.acq_from_moments(bounds, mu, v, tau, t, est == "LB2", return_w=True)
            w_min = float(W.detach().min())
            assert w_min >= W_MIN, f"{cid}: reference-side W = {w_min:.3g} < {W_MIN}"
            (g,) = torch.autograd.grad(acq.sum(), Xr, retain_graph=True)
            out[(est, t)] = (acq.detach(), g)
    return out


def spreads(cid: str):
    """(largest |acq - acq_reversed|, largest |dacq - dacq_reversed|) over the case's estimators and targets."""
    a, b = reference(cid), reference(cid, True)
    keys = [k for k in a if k != "moments"]
    return (max(float((a[k][0] - b[k][0]).abs().max()) for k in keys),
            max(float((a[k][1] - b[k][1]).abs().max()) for k in keys))
