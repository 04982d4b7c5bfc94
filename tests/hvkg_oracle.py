"""ORACLE (test infrastructure only): the hypervolume knowledge gradient as a differentiable fp64 torch
restatement on ``oracle.gp.OutputGP``.

* The moments come from ``OutputGP.posterior`` on the joint rows ``[x; x'_1 .. x'_R]`` of one restart: the means of
  the fantasy rows, ``Cov(x, x'_r)`` and ``Var(x)`` (as the KG oracle takes ``Cov(x_0, z_k)``), so
  ``Y_r,i = mean_i(x'_r) + [i in E] z_f,i Cov_i(x, x'_r) / sqrt(Var_i(x) + y_std_i^2 noise_i)`` in the untransformed
  space.
* The hypervolume is a sweep for m = 2 and slabs on the last objective for m = 3, with the device's conventions:
  a point counts when it is strictly above ref in every objective; slab k holds the k + 1 points of largest last
  objective (ties: lowest index first); a sweep visits its points by (y0 descending, y1 descending, slab rank
  ascending) and a point adds ``(y0 - ref0) (y1 - h)`` when y1 exceeds the running maximum h strictly.  Which
  points add is decided on detached values; the terms themselves are differentiable, so autograd gives the
  subgradients the device states: exactly 0 for a point that adds nothing, the lowest index of exact duplicates
  takes the derivative.
* ``reverse=True`` restates every output with its training rows reversed (the same function, another summation
  order: the reference side's rounding floor), as ``jes_oracle.augmented_models`` does.
"""

from __future__ import annotations

import torch

from oracle.gp import OutputGP


def models_of(state, reverse: bool = False):
    out = []
    for o in state.models:
        x, y = o.train_x, o.train_y
        if reverse:
            x, y = x.flip(0), y.flip(0)
        out.append(OutputGP(x, y, o.lengthscale, o.outputscale, o.noise, o.mean_constant, o.kernel, o.nu, o.y_mean,
                            o.y_std))
    return out


def fantasy_means(models, X_full: torch.Tensor, z: torch.Tensor, mask_bits: int, Nf: int, Np: int) -> torch.Tensor:
    """``X_full [B, 1 + Nf Np, d]``, ``z [Nf, m]`` -> ``Y [B, Nf, Np, m]`` (differentiable in X_full)."""
    B = X_full.shape[0]
    m = len(models)
    per_b = []
    for b in range(B):
        cols = []
        for i, gp in enumerate(models):
            mean, cov = gp.posterior(X_full[b])
            y = mean[1:]
            if (mask_bits >> i) & 1:
                sig = torch.sqrt(cov[0, 0] + gp.noise * gp.y_std**2)
                y = y + z[:, i].repeat_interleave(Np) * cov[0, 1:] / sig
            cols.append(y)
        per_b.append(torch.stack(cols, dim=-1).reshape(Nf, Np, m))
    return torch.stack(per_b)


def posterior_means(models, X: torch.Tensor) -> torch.Tensor:
    """The value function's points: ``X [B, q, d] -> Y [B, 1, q, m]``."""
    return torch.stack([torch.stack([gp.posterior(X[b])[0] for gp in models], dim=-1) for b in range(X.shape[0])])[:, None]


def _hv_set(Y: torch.Tensor, ref) -> torch.Tensor:
    Np, m = Y.shape
    Yd = Y.detach().tolist()
    r = [float(v) for v in ref]
    valid = [p for p in range(Np) if all(Yd[p][i] > r[i] for i in range(m))]
    if not valid:
        return Y.sum() * 0.0
    if m == 2:
        rank = {p: k for k, p in enumerate(valid)}
        slabs = [(valid, None)]
    else:
        order3 = sorted(valid, key=lambda p: (-Yd[p][2], p))
        rank = {p: k for k, p in enumerate(order3)}
        slabs = []
        for k in range(len(order3)):
            lower = Y[order3[k + 1], 2] if k + 1 < len(order3) else r[2]
            slabs.append((order3[: k + 1], Y[order3[k], 2] - lower))
    total = Y.sum() * 0.0
    for pts, thick in slabs:
        srt = sorted(pts, key=lambda p: (-Yd[p][0], -Yd[p][1], rank[p]))
        h_val, h = r[1], r[1]
        area = Y.sum() * 0.0
        for p in srt:
            if Yd[p][1] > h_val:
                area = area + (Y[p, 0] - r[0]) * (Y[p, 1] - h)
                h_val, h = Yd[p][1], Y[p, 1]
        total = total + (area if thick is None else thick * area)
    return total


def hypervolume(Y: torch.Tensor, ref) -> torch.Tensor:
    """``Y [..., Np, m]`` (m = 2 or 3) -> the hypervolumes ``[...]`` over ``ref``, differentiable in Y."""
    m = Y.shape[-1]
    assert m in (2, 3)
    flat = Y.reshape((-1,) + tuple(Y.shape[-2:]))
    out = torch.stack([_hv_set(flat[s], ref) for s in range(flat.shape[0])])
    return out.reshape(Y.shape[:-2])


def acq_from_means(Y: torch.Tensor, ref, current: float = 0.0, cost: float = 1.0):
    """``Y [B, Nf, Np, m]`` -> (acq [B], the uncancelled scale mean_f HV_f / cost [B])."""
    hv = hypervolume(Y, ref)                    # [B, Nf]
    mean = hv.mean(dim=-1)
    return (mean - current) / cost, mean.detach() / cost


def acquisition(models, X_full, z, mask_bits, Nf, Np, ref, current=0.0, cost=1.0):
    return acq_from_means(fantasy_means(models, X_full, z, mask_bits, Nf, Np), ref, current, cost)


def value_function(models, X, ref):
    return acq_from_means(posterior_means(models, X), ref)


def kink_margin(Y: torch.Tensor, ref, ranges=None) -> float:
    """The smallest gap, in units of each objective's range (``ranges``; by default the range over
    ``Y [B, Nf, Np, m]`` itself), between two coordinates of one fantasy's points or between a coordinate and ref:
    the kink condition asks for at least 1e-6."""
    Y = Y.detach()
    m = Y.shape[-1]
    worst = float("inf")
    for i in range(m):
        v = Y[..., i]                                             # [B, Nf, Np]
        rng = float(ranges[i]) if ranges is not None else (float(v.max() - v.min()) or 1.0)
        withref = torch.cat([v, torch.full_like(v[..., :1], float(ref[i]))], dim=-1)
        gaps = (withref[..., :, None] - withref[..., None, :]).abs()
        gaps = gaps + torch.eye(withref.shape[-1], dtype=gaps.dtype) * 1e300
        worst = min(worst, float(gaps.min()) / rng)
    return worst


def fantasy_mean_by_refactorising(gp: OutputGP, x: torch.Tensor, xp: torch.Tensor, zf: float) -> torch.Tensor:
    """The posterior mean at ``xp [R, d]`` of ``gp`` with the row ``(x, mu(x) + sigma~(x) z)`` appended and the
    model refactorised (untransformed space): what ``fantasize`` + ``PosteriorMeanModel`` compute."""
    mean, cov = gp.posterior(x.reshape(1, -1))
    mu_model = (mean[0] - gp.y_mean) / gp.y_std
    sig_model = torch.sqrt(cov[0, 0] / gp.y_std**2 + gp.noise)
    y_new = mu_model + sig_model * zf
    big = OutputGP(torch.cat([gp.train_x, x.reshape(1, -1)]), torch.cat([gp.train_y, y_new.reshape(1)]),
                   gp.lengthscale, gp.outputscale, gp.noise, gp.mean_constant, gp.kernel, gp.nu, gp.y_mean, gp.y_std)
    return big.posterior(xp)[0]


class OracleValueFunction:
    """The value function on the CPU: ``forward(X[*batch, q, d]) -> [*batch]`` by the restatement above."""

    def __init__(self, state, ref_point):
        self.models = models_of(state)
        self.ref = [float(v) for v in ref_point]

    def __call__(self, X):
        flat = X.reshape((-1,) + tuple(X.shape[-2:])).double()
        return value_function(self.models, flat, self.ref)[0].reshape(X.shape[:-2])


class OracleHvkg:
    """The one-shot acquisition on the CPU with the surface ``HvkgOptimisationSpec`` uses: ``X_evaluation_mask``
    (``[1, m]`` booleans, None = all), ``extract_candidates``, ``get_augmented_q_batch_size`` and
    ``forward(X_full[*batch, 1 + Nf Np, d]) -> [*batch]``."""

    def __init__(self, state, ref_point, num_fantasies, num_pareto, base_samples, current_value=None,
                 cost_aware_utility=None):
        self.models = models_of(state)
        self.m = len(self.models)
        self.ref = [float(v) for v in ref_point]
        self.Nf, self.Np = int(num_fantasies), int(num_pareto)
        self.z = torch.as_tensor(base_samples, dtype=torch.double)
        self.current = 0.0 if current_value is None else float(current_value)
        self.costs = None if cost_aware_utility is None else [float(c) for c in cost_aware_utility]
        self.X_evaluation_mask = None

    def _bits(self) -> int:
        if self.X_evaluation_mask is None:
            return (1 << self.m) - 1
        return sum(1 << i for i, f in enumerate(self.X_evaluation_mask.reshape(-1).tolist()) if f)

    def cost(self) -> float:
        bits = self._bits()
        return 1.0 if self.costs is None else sum(c for i, c in enumerate(self.costs) if (bits >> i) & 1)

    def get_augmented_q_batch_size(self, q: int) -> int:
        return q + self.Nf * self.Np

    def extract_candidates(self, X_full):
        return X_full[..., : -self.Nf * self.Np, :]

    def evaluate(self, X):
        """(acq [*batch], the value's scale mean_f HV_f / cost [*batch], the fantasised means)."""
        flat = X.reshape((-1,) + tuple(X.shape[-2:])).double()
        Y = fantasy_means(self.models, flat, self.z, self._bits(), self.Nf, self.Np)
        acq, scale = acq_from_means(Y, self.ref, self.current, self.cost())
        return acq.reshape(X.shape[:-2]), scale.reshape(X.shape[:-2]), Y

    def __call__(self, X):
        return self.evaluate(X)[0]
