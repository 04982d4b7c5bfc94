"""ORACLE (test infrastructure only) -- the lower-bound joint entropy search (JES-LB / LB2, Tu et al. 2022)
restated in fp64 torch, differentiable.

The reference is ``qLowerBoundMultiObjectiveJointEntropySearch`` (``modules/acquisition/
joint_entropy_search.py``): ``_compute_posterior_statistics`` (:378-470) takes the moments of a candidate
from the model and from every model conditioned on a sampled Pareto set (``condition_on_observations`` with
observation noise, :365-376), ``_compute_entropy_upper_bound`` (:596-732) bounds the entropy over the box
decomposition.  The entropy step below is written from the formulas of DESIGN.md 8d and is pinned to the
reference's own function by ``tests/golden/jes_entropy.npz``; the moments come from ``oracle.gp.OutputGP
.posterior`` on the augmented training data (BoTorch's conditioning cannot run here: DESIGN.md 8d).

Shapes: P samples, S = P + 1 states (state 0 the model), m outputs, B candidates, J boxes.
"""

from __future__ import annotations

import math

import torch

from oracle.gp import OutputGP

EPS = 2.0 ** -52
HALF_LOG_2PIE = 0.5 * (1.0 + math.log(2.0 * math.pi))
# candidates per OutputGP.posterior call: 1 keeps torch.cdist on its exact path for the small Matern-1/2
# outputs of the test cases (n + k_p + 1 <= 25 rows; above 25 rows it forms r^2 by a matrix product, whose
# rounding at r = 0 is ~1e-8 in r: the prior variance s kappa(0) of Matern-1/2 then moves by 1e-8 s)
CHUNK = 1


def augmented_models(state, pareto_sets, pareto_fronts, reverse: bool = False):
    """[S][m] OutputGP: state 0 the model's outputs, state p + 1 output i with the rows
    (ps_p, (pf_p[:, i] - y_mean_i) / y_std_i) appended; hyperparameters unchanged.  ``reverse``: every
    output's training rows in reversed order (the same function, another summation order)."""
    out = []
    for s in range(len(pareto_sets) + 1):
        row = []
        for i, o in enumerate(state.models):
            x, y = o.train_x, o.train_y
            if s > 0:
                ps = torch.as_tensor(pareto_sets[s - 1], dtype=torch.double)
                pf = torch.as_tensor(pareto_fronts[s - 1], dtype=torch.double)
                x = torch.cat([x, ps])
                y = torch.cat([y, (pf[:, i] - o.y_mean) / o.y_std])
            if reverse:
                x, y = x.flip(0), y.flip(0)
            row.append(OutputGP(x, y, o.lengthscale, o.outputscale, o.noise, o.mean_constant, o.kernel, o.nu,
                                o.y_mean, o.y_std))
        out.append(row)
    return out


def moments(models, X: torch.Tensor, chunk: int = CHUNK):
    """(mu, v, tau), each [S, m, B], untransformed space: mu the posterior mean, v = max(var, eps) without
    observation noise, tau = max(max(var + noise, eps) - v, eps) (joint_entropy_search.py:428-461).  State 0:
    v holds var + noise unclamped (the initial entropy's argument, :406-423) and tau 0."""
    S, m, B = len(models), len(models[0]), X.shape[0]
    mu, v, tau = [], [], []
    for s in range(S):
        for i in range(m):
            gp = models[s][i]
            ms, vs, ns = [], [], []
            for b0 in range(0, B, chunk):
                xb = X[b0:b0 + chunk]
                mean, cov = gp.posterior(xb)
                var = cov.diagonal()
                ms.append(mean)
                vs.append(var)
                ns.append(var + gp.noise * gp.y_std ** 2)
            mean, var, varn = torch.cat(ms), torch.cat(vs), torch.cat(ns)
            mu.append(mean)
            if s == 0:
                v.append(varn)
                tau.append(torch.zeros_like(varn))
            else:
                vc = var.clamp_min(EPS)
                v.append(vc)
                tau.append((varn.clamp_min(EPS) - vc).clamp_min(EPS))
    shape = (S, m, B)
    return torch.stack(mu).reshape(shape), torch.stack(v).reshape(shape), torch.stack(tau).reshape(shape)


def _phi(g):
    return torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def _Phi(g):
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))


def entropy_bound(bounds, mu, v, tau, target=None, only_diagonal=False):
    """H_p [B, P] and W = sum_j W_j [B, P] (before the clamp at 1) of DESIGN.md 8d.
    bounds [P, 2, J, m]; mu, v, tau [B, P, m]."""
    m = mu.shape[-1]
    sd = v.sqrt()
    gl = (bounds[None, :, 0] - mu[:, :, None]) / sd[:, :, None]          # [B, P, J, m]
    gu = (bounds[None, :, 1] - mu[:, :, None]) / sd[:, :, None]
    pl, pu = _phi(gl), _phi(gu)
    Wji = (_Phi(gu) - _Phi(gl)).clamp_min(EPS)
    Vji = gu * pu - gl * pl
    Gji = pu - pl
    Wj = torch.exp(torch.log(Wji).sum(-1))                               # [B, P, J]
    Wsum = Wj.sum(-1)                                                    # [B, P]
    W = Wsum.clamp_max(1.0)
    om = Wj / W[..., None]
    s = sd[:, :, None] * (Gji / Wji)                                     # s_ji
    a = (om[..., None] * s).sum(-2)                                      # sum_j omega_j s_ji  [B, P, m]
    mom1 = mu - a
    D = (om[..., None] * v[:, :, None] * Vji / Wji).sum(-2)
    if only_diagonal:
        var = (v + tau - D - 2.0 * mu * a + mu * mu - mom1 * mom1).clamp_min(EPS)
        if target is None:
            return m * HALF_LOG_2PIE + 0.5 * torch.log(var).sum(-1), Wsum
        return HALF_LOG_2PIE + 0.5 * torch.log(var[..., target]), Wsum
    Sik = (om[..., None, None] * s[..., :, None] * s[..., None, :]).sum(-3)   # [B, P, m, m]
    cov = (mu[..., :, None] * mu[..., None, :] - (mu[..., :, None] * a[..., None, :] + mu[..., None, :] * a[..., :, None])
           + Sik + torch.diag_embed(v + tau - D - Sik.diagonal(dim1=-2, dim2=-1))
           - mom1[..., :, None] * mom1[..., None, :])
    if target is None:
        return m * HALF_LOG_2PIE + 0.5 * torch.logdet(cov + 1e-6 * torch.eye(m, dtype=cov.dtype)), Wsum
    return HALF_LOG_2PIE + 0.5 * torch.log(cov[..., target, target]), Wsum


def acq_from_moments(bounds, mu, v, tau, target=None, only_diagonal=False, return_w=False):
    """acq [B] = H_0 - mean_p H_p from moments [S, m, B] (``moments``)."""
    m = mu.shape[1]
    v0 = v[0].T                                                          # [B, m]: var0 + noise
    if target is None:
        H0 = m * HALF_LOG_2PIE + 0.5 * torch.log(v0).sum(-1)
    else:
        H0 = HALF_LOG_2PIE + 0.5 * torch.log(v0[:, target])
    perm = lambda t: t[1:].permute(2, 0, 1)  # noqa: E731  [B, P, m]
    H, Wsum = entropy_bound(bounds, perm(mu), perm(v), perm(tau), target, only_diagonal)
    acq = H0 - H.mean(-1)
    return (acq, Wsum) if return_w else acq


def jes_value(models, bounds, X, target=None, only_diagonal=False, return_w=False):
    return acq_from_moments(bounds, *moments(models, X), target, only_diagonal, return_w)


def value_and_grad(models, bounds, X, target=None, only_diagonal=False):
    """acq [B] and dacq/dX [B, d] by autograd (a candidate's value depends on its own row only)."""
    Xr = X.clone().requires_grad_(True)
    acq = jes_value(models, bounds, Xr, target, only_diagonal)
    (g,) = torch.autograd.grad(acq.sum(), Xr)
    return acq.detach(), g


class OracleJES:
    """The restatement behind the acquisition interface (``forward(X[*batch, 1, d]) -> [*batch]``,
    differentiable): what the optimisation tests run ``optimize_acqf`` and ``JesOptimisationSpec`` on."""

    def __init__(self, state, pareto_sets, pareto_fronts, hypercell_bounds, estimation_type="LB",
                 target_output_ix=None):
        self.models = augmented_models(state, pareto_sets, pareto_fronts)
        self.bounds = hypercell_bounds.to(torch.double)
        self.only_diagonal = estimation_type == "LB2"
        m = len(state.models)
        self.target = None if target_output_ix is None else int(target_output_ix) % m

    def __call__(self, X):
        batch, d = X.shape[:-2], X.shape[-1]
        return jes_value(self.models, self.bounds, X.reshape(-1, d).double(), self.target,
                         self.only_diagonal).reshape(batch).to(X.dtype)
