"""The reference's BO metrics on a sampled Pareto front, as host torch code (they are tiny: a
1024 x npoints x m product and an exact hypervolume of ~100 points).

* ``estimate_best_possible_expected_performance_after_scalarisation`` and
  ``estimate_expected_performance_after_scalarisation``: ``modules/performance_after_scalarisation.py:19-123``;
* ``calculate_reference_point``, ``estimate_hypervolume``, ``estimate_hypervolume_from_posterior_mean``:
  ``modules/pareto/botorch_hypervolume.py:12-95``.  The reference takes the dominated hypervolume from BoTorch's
  ``DominatedPartitioning.compute_hypervolume``, which is exact; BoTorch is absent here, so ``hypervolume`` computes
  the same exact number directly: a sweep for m = 2, slicing over the last objective for m >= 3.  Points that do
  not strictly dominate the reference point contribute nothing, as with ``DominatedPartitioning``.

All objectives are maximised.
"""

from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch
from torch import Tensor

from .errors import BotorchTensorDimensionError
from .utils import sample_simplex

N_SCALARISATIONS = 2**10  # performance_after_scalarisation.py:13


def scalarise_linear(points: Tensor, weights: Tensor) -> Tensor:
    """``modules/scalarisations.py:8-9``."""
    return torch.sum(points * weights, dim=-1)


def _tensor(a, tkwargs=None) -> Tensor:
    kw = {"dtype": torch.double}
    kw.update(tkwargs or {})
    return torch.as_tensor(np.asarray(a) if not isinstance(a, Tensor) else a).to(**kw)


def estimate_best_possible_expected_performance_after_scalarisation(
        pareto_front, scalarise: Callable = scalarise_linear, *, n_scalarisations: int = N_SCALARISATIONS,
        scalarisations_seed: Optional[int] = None, tkwargs=None) -> float:
    """The expectation over qMC scalarisation weights of the best scalarised objective on the sampled front
    (``performance_after_scalarisation.py:19-58``)."""
    front = _tensor(pareto_front, tkwargs)
    W = sample_simplex(front.shape[-1], qmc=True, n=n_scalarisations, seed=scalarisations_seed, dtype=front.dtype)
    scalarised = scalarise(front, W.to(front.device).unsqueeze(-2))
    best, _ = torch.max(scalarised, dim=-1)
    return torch.mean(best).item()


def estimate_expected_performance_after_scalarisation(
        posterior_pareto_set, posterior_pareto_front, problem, scalarise: Callable = scalarise_linear, *,
        n_scalarisations: int = N_SCALARISATIONS, scalarisations_seed: Optional[int] = None,
        tkwargs=None) -> Dict[str, float]:
    """Predicted and actual expected scalarised performance of the recommendations
    (``performance_after_scalarisation.py:61-123``): per weight the front's best point (``torch.max``: the first
    index on ties) is the recommendation; its design is evaluated on the true problem (``problem(x)`` -> [n, m])."""
    pset = _tensor(posterior_pareto_set, tkwargs)
    front = _tensor(posterior_pareto_front, tkwargs)
    W = sample_simplex(problem.num_objectives, qmc=True, n=n_scalarisations, seed=scalarisations_seed,
                       dtype=front.dtype).to(front.device)
    scalarised = scalarise(front, W.unsqueeze(-2))
    predicted, rec = torch.max(scalarised, dim=-1)
    real = torch.as_tensor(problem(pset[rec])).to(front)
    performances = scalarise(real, W)
    return {"predicted_scalarperf": predicted.mean().item(), "actual_scalarperf": performances.mean().item()}


def calculate_reference_point(pareto_front: Tensor, buffer: float = 0.01) -> Tensor:
    """The front's minimum less ``buffer`` of its range per objective (``botorch_hypervolume.py:45-63``)."""
    if not pareto_front.ndim == 2:
        raise BotorchTensorDimensionError(
            f"Expected pareto_front to have 2-dimensions. Got {pareto_front.ndim=}.")
    lo = pareto_front.min(dim=-2).values
    hi = pareto_front.max(dim=-2).values
    return lo - buffer * (hi - lo)


def _hv(P: np.ndarray, ref: np.ndarray) -> float:
    """Exact dominated hypervolume of the rows of P (each strictly above ref) by slicing on the last objective."""
    n, m = P.shape
    if n == 0:
        return 0.0
    if m == 1:
        return float(P[:, 0].max() - ref[0])
    if m == 2:
        P = P[np.lexsort((-P[:, 1], -P[:, 0]))]  # first objective descending
        hv, top = 0.0, ref[1]
        for f0, f1 in P:
            if f1 > top:
                hv += (f0 - ref[0]) * (f1 - top)
                top = f1
        return float(hv)
    P = P[np.argsort(-P[:, -1], kind="stable")]  # last objective descending
    z = P[:, -1]
    hv = 0.0
    for i in range(n):
        below = z[i + 1] if i + 1 < n else ref[-1]
        if z[i] > below:  # the slab (below, z_i]: the points 0..i are the ones reaching it
            hv += (z[i] - below) * _hv(P[:i + 1, :-1], ref[:-1])
    return float(hv)


def hypervolume(points, ref_point, device=None) -> float:
    """The exact hypervolume dominated by ``points`` [n, m] above ``ref_point`` [m]
    (``DominatedPartitioning(ref_point, points).compute_hypervolume()``).  ``device`` (default None: the host
    recursion below): for m <= 3 the sweep of ``dkg_amd.boxes.hypervolume_front`` on that ROCm device, the same
    number to rounding; m > 3 stays on the host."""
    if device is not None and len(ref_point) <= 3:
        from .boxes import hypervolume_front

        return float(hypervolume_front(torch.as_tensor(points).reshape(-1, len(ref_point)), ref_point, device=device))
    P = np.asarray(torch.as_tensor(points).detach().cpu().numpy(), dtype=np.float64).reshape(-1, len(ref_point))
    ref = np.asarray(torch.as_tensor(ref_point).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    return _hv(P[(P > ref).all(-1)], ref)


def estimate_hypervolume(pareto_front: Tensor, ref_point: Tensor, return_upper: bool = True, device=None):
    """Lower and (estimated) upper bounds of the dominated hypervolume from a sample of the front
    (``botorch_hypervolume.py:66-95``): the lower bound is the sample's hypervolume; the upper bound is the box
    between the reference point and the sample's ideal point less the hypervolume of the negated points above
    the negated ideal point.  ``device``: as ``hypervolume``'s."""
    pareto_front = torch.as_tensor(pareto_front)
    ref_point = torch.as_tensor(ref_point).to(pareto_front)
    lower = hypervolume(pareto_front, ref_point, device=device)
    if not return_upper:
        return lower
    ideal, _ = pareto_front.max(dim=0)
    above = (pareto_front > ref_point).all(dim=-1)
    if not above.any():
        upper = 0
    else:
        complement = hypervolume(-pareto_front[above], -ideal, device=device)
        upper = torch.prod(ideal - ref_point).item() - complement
    return lower, upper


def estimate_hypervolume_from_posterior_mean(pareto_set, pareto_front, true_problem, ref_point, *,
                                             tkwargs=None, device=None) -> Dict[str, float]:
    """Bounds of the hypervolume of the model's front and of the true image of its Pareto set
    (``botorch_hypervolume.py:12-42``; same keys).  ``device``: as ``hypervolume``'s, for all four."""
    pset = _tensor(pareto_set, tkwargs)
    front = _tensor(pareto_front, tkwargs)
    image = torch.as_tensor(true_problem(pset)).to(front)
    ref = torch.as_tensor(ref_point).to(front)
    pfront_lo, pfront_hi = estimate_hypervolume(front, ref, device=device)
    pset_lo, pset_hi = estimate_hypervolume(image, ref, device=device)
    return {"pfront_hv_lo": pfront_lo, "pfront_hv_hi": pfront_hi, "pset_hv_lo": pset_lo, "pset_hv_hi": pset_hi}
