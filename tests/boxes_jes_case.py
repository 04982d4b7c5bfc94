"""The three-objective joint entropy search case of ``test_gpu_boxes.py``, built on the CPU from a seed as
``jes_cases.problem`` builds its cases: n = 17, d = 2, three Pareto samples of 1, 4 and 10 points (spread over the
non-dominated points, in all three objectives, of the posterior mean on a pool of 128 uniform points, lifted by
y_std (0.5 + 0.1 |noise|): a front that dominates most of the posterior, as a sampled one does), B = 17 candidates with candidate 0 on a Pareto-set point and candidate 1 on a training point.
The boxes are the restatement's (``boxes_ref.py``) over -1e10, and a slab partition of the same region.

Conditions on the inputs, asserted here on the reference alone: every (candidate, sample) has W >= 1e-3 under both
partitions, and the oracle's own values under the two partitions differ by at most a quarter of the asserted value
bound.  The lift was raised (0.1 left W at 6e-13 at the one-point sample) until the first held."""

from __future__ import annotations

import functools

import numpy as np
import torch

import boxes_ref as br
import jes_cases
import jes_oracle
from helpers import grad_case, to_oracle

SEED = 16
LIFT = 0.5  # of y_std, added to the picked means
KS = (1, 4, 10)
NEG = -1e10
# DESIGN.md 8d's asserted bounds (tests/test_gpu_jes.py)
SPREAD_VALUE, SPREAD_GRAD, RTOL = 1.1e-8, 1.8e-6, 1e-6


def bounds_of(fronts, fn=br.boxes) -> torch.Tensor:
    ref = np.full(3, NEG)
    per = [fn(pf.numpy(), ref) for pf in fronts]
    J = max(lo.shape[0] for lo, _ in per)
    out = torch.zeros(len(per), 2, J, 3, dtype=torch.double)
    for p, (lo, hi) in enumerate(per):
        out[p, 0, : lo.shape[0]], out[p, 1, : hi.shape[0]] = torch.from_numpy(lo), torch.from_numpy(hi)
    return out


@functools.lru_cache(maxsize=None)
def problem(seed: int = SEED):
    """-> (state, pareto_sets, pareto_fronts, X [17, 2])."""
    state, _, _, X = grad_case(3, 2, (17,), ("M52", "RBF", "M32"), 4, 2, 17, seed, noise=1e-2)
    om = to_oracle(state)
    g = torch.Generator().manual_seed(1000 + seed)
    ys = torch.tensor([o.y_std for o in om.models], dtype=torch.double)
    sets, fronts = [], []
    for k in KS:
        pool = torch.rand(jes_cases.POOL, 2, generator=g, dtype=torch.double)
        mean = torch.stack([torch.cat([o.posterior(pool[r:r + 8])[0] for r in range(0, jes_cases.POOL, 8)])
                            for o in om.models], dim=1)
        dominated = ((mean[None] >= mean[:, None]).all(-1) & (mean[None] > mean[:, None]).any(-1)).any(1)
        nd = torch.nonzero(~dominated).reshape(-1)
        nd = nd[torch.argsort(mean[nd, 0])]
        assert len(nd) >= k, (len(nd), k)
        pick = nd[torch.linspace(0, len(nd) - 1, k).round().long()]
        sets.append(pool[pick])
        fronts.append(mean[pick] + ys * (LIFT + 0.1 * torch.randn(k, 3, generator=g, dtype=torch.double).abs()))
    X = X.clone()
    X[0] = sets[0][0]
    X[1] = state.models[0].train_x[3]
    return state, sets, fronts, X


def value_tol(ref):
    return RTOL * ref.abs() + 4 * SPREAD_VALUE


@functools.lru_cache(maxsize=None)
def reference(seed: int = SEED):
    """{(est, target): (acq [B], dacq/dX [B, d], acq on the slab partition [B])} with the conditions asserted."""
    state, sets, fronts, X = problem(seed)
    bounds, slabs = bounds_of(fronts), bounds_of(fronts, br.slab_boxes)
    assert slabs.shape[2] > bounds.shape[2]
    models = jes_oracle.augmented_models(state, sets, fronts)
    Xr = X.clone().requires_grad_(True)
    mu, v, tau = jes_oracle.moments(models, Xr)
    out = {}
    for est in jes_cases.ESTIMATORS:
        for t in (None, 0, 2):
            acq, W = jes_oracle.acq_from_moments(bounds, mu, v, tau, t, est == "LB2", return_w=True)
            acq_s, W_s = jes_oracle.acq_from_moments(slabs, mu, v, tau, t, est == "LB2", return_w=True)
            w_min = min(float(W.detach().min()), float(W_s.detach().min()))
            assert w_min >= jes_cases.W_MIN, f"reference-side W = {w_min:.3g} < {jes_cases.W_MIN}"
            spread = (acq - acq_s).detach().abs()
            assert bool((spread <= 0.25 * value_tol(acq.detach())).all()), (est, t, float(spread.max()))
            (g,) = torch.autograd.grad(acq.sum(), Xr, retain_graph=True)
            out[(est, t)] = (acq.detach(), g, acq_s.detach())
    return out
