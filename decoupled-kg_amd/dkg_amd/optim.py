"""Acquisition optimisation over the device KG.

``DiscreteKgOptimisationSpec`` (reference ``acquisition_optimisation_strategy.py:166-273``)
hands ``DiscreteKnowledgeGradient`` to BoTorch's ``optimize_acqf`` with q = 1.  BoTorch is
pinned to a git revision (botorch@c14808f, ``requirements.txt:16``) and is neither vendored
nor installed here, so this module restates the parts of its published algorithm that path
uses:

* ``gen_batch_initial_conditions``: ``raw_samples`` scrambled-Sobol points in the bounds,
  their acquisition values (no gradient, in chunks of ``init_batch_limit``), and
  ``initialize_q_batch``'s Boltzmann selection of ``num_restarts`` starts (eta = 1, the best
  raw point always kept);
* ``gen_candidates_scipy``: L-BFGS-B (scipy) on ``-sum(acq(X))`` over one chunk of restarts
  with the analytic gradient and box bounds, candidates clamped to the bounds;
* ``optimize_acqf``: restarts in chunks of ``batch_limit``, the best candidate returned.

On the device a chunk's value + gradient is one C call for all of its restarts
(``dkg_plan_forward_grad``), so ``batch_limit = num_restarts`` evaluates every restart in the
same launch; the reference uses ``batch_limit = 1`` because its forward is a Python loop over
candidates (``pipeline/nodes/bo_loop.py:127-129``).  ``batch_limit`` keeps BoTorch's meaning:
restarts in one chunk share one L-BFGS-B problem (the sum of their values).

``JesOptimisationSpec`` (``acquisition_optimisation_strategy.py:447-552``) runs the same ``optimize_acqf`` on
the device joint entropy search (``dkg_amd.jes``), and ``HvkgOptimisationSpec`` (``:276-444``) on the
device hypervolume knowledge gradient (``dkg_amd.hvkg``).
"""

from __future__ import annotations

import logging
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

logger = logging.getLogger(__name__)

# option keys consumed by the initial-condition stage, not passed to L-BFGS-B
# (BoTorch optimize_acqf's INIT_OPTION_KEYS subset that applies here)
INIT_OPTION_KEYS = {"batch_limit", "init_batch_limit", "eta", "seed", "nonnegative", "alpha"}


def draw_sobol_samples(bounds: Tensor, n: int, q: int, seed: Optional[int] = None) -> Tensor:
    """``botorch.utils.sampling.draw_sobol_samples``: n x q x d scrambled Sobol points in ``bounds``."""
    lower, upper = bounds[0], bounds[1]
    d = lower.shape[-1]
    if seed is None:
        seed = int(torch.randint(0, 10**6, (1,)).item())
    from .utils import sobol_draw

    raw = sobol_draw(d * q, n, seed, lower.dtype).to(lower.device).view(n, q, d)
    return lower + (upper - lower) * raw


def initialize_q_batch(X: Tensor, Y: Tensor, n: int, eta: float = 1.0) -> Tensor:
    """``botorch.optim.initializers.initialize_q_batch``: Boltzmann sample of n rows of X by
    ``exp(eta * standardised Y)``, always keeping the best raw point."""
    n_samples = X.shape[0]
    if n > n_samples:
        raise RuntimeError(f"n ({n}) cannot be larger than the number of provided samples ({n_samples})")
    if n == n_samples:
        return X
    Ystd = Y.std(dim=0)
    if bool(torch.any(Ystd == 0)):
        warnings.warn("All acquisition values for raw samples points are the same for at least one batch. "
                      "Choosing initial conditions at random.", RuntimeWarning)
        return X[torch.randperm(n=n_samples, device=X.device)][:n]
    max_idx = int(torch.argmax(Y))
    Z = (Y - Y.mean(dim=0)) / Ystd
    etaZ = eta * Z
    weights = torch.exp(etaZ)
    while bool(torch.isinf(weights).any()):
        etaZ = etaZ * 0.5
        weights = torch.exp(etaZ)
    idcs = torch.multinomial(weights, n)
    if max_idx not in idcs:
        idcs[-1] = max_idx
    return X[idcs]


def _no_grad_values(acq: Callable[[Tensor], Tensor], X: Tensor, chunk: int) -> Tensor:
    with torch.no_grad():
        return torch.cat([acq(X[i:i + chunk]).reshape(-1) for i in range(0, X.shape[0], chunk)])


def gen_batch_initial_conditions(acq_function: Callable[[Tensor], Tensor], bounds: Tensor, q: int,
                                 num_restarts: int, raw_samples: int, options: Optional[Dict] = None) -> Tensor:
    """``botorch.optim.initializers.gen_batch_initial_conditions`` (q-batch Sobol raw samples,
    ``initialize_q_batch``): num_restarts x q x d starting points."""
    options = options or {}
    X_rnd = draw_sobol_samples(bounds, raw_samples, q, seed=options.get("seed"))
    chunk = options.get("init_batch_limit", options.get("batch_limit", raw_samples)) or raw_samples
    Y_rnd = _no_grad_values(acq_function, X_rnd, max(1, int(chunk)))
    return initialize_q_batch(X_rnd, Y_rnd.to(X_rnd), n=num_restarts, eta=options.get("eta", 1.0))


def gen_candidates_scipy(initial_conditions: Tensor, acquisition_function: Callable[[Tensor], Tensor],
                         lower_bounds: Tensor, upper_bounds: Tensor,
                         options: Optional[Dict] = None) -> Tuple[Tensor, Tensor]:
    """``botorch.generation.gen.gen_candidates_scipy`` with L-BFGS-B: minimise -sum acq over the
    flattened restarts (box bounds, analytic gradient); returns (candidates, acq values)."""
    from scipy.optimize import minimize

    options = dict(options or {})
    ic = initial_conditions.clamp(lower_bounds, upper_bounds)
    shapeX = ic.shape
    lb = lower_bounds.expand(shapeX).reshape(-1).cpu().numpy()
    ub = upper_bounds.expand(shapeX).reshape(-1).cpu().numpy()
    bounds = list(zip(lb.tolist(), ub.tolist()))

    fast = getattr(acquisition_function, "value_and_grad_host", None)

    def f_np(x: np.ndarray):
        if fast is not None:
            # the device KG: value and gradient in one round trip (DiscreteKnowledgeGradient.value_and_grad_host)
            kg, g = fast(torch.from_numpy(x).view(shapeX))
            loss = -float(kg.sum())
            if not np.isfinite(loss):
                raise RuntimeError("acquisition function returned a non-finite value inside L-BFGS-B")
            return loss, (-g).reshape(-1).numpy()
        X = torch.from_numpy(x).to(ic).view(shapeX).contiguous().requires_grad_(True)
        loss = -acquisition_function(X).sum()
        if not torch.isfinite(loss):
            raise RuntimeError("acquisition function returned a non-finite value inside L-BFGS-B")
        (grad,) = torch.autograd.grad(loss, X)
        return float(loss.item()), grad.reshape(-1).double().cpu().numpy()

    minimize_opts = {k: v for k, v in options.items() if k not in ("method", "callback", "with_grad")}
    res = minimize(f_np, ic.reshape(-1).double().cpu().numpy(), method="L-BFGS-B", jac=True, bounds=bounds,
                   options=minimize_opts)
    candidates = torch.from_numpy(res.x).to(ic).view(shapeX).clamp(lower_bounds, upper_bounds)
    with torch.no_grad():
        batch_acquisition = acquisition_function(candidates)
    return candidates, batch_acquisition


def optimize_acqf(acq_function: Callable[[Tensor], Tensor], bounds: Tensor, q: int, num_restarts: int,
                  raw_samples: Optional[int] = None, options: Optional[Dict] = None,
                  batch_initial_conditions: Optional[Tensor] = None,
                  return_best_only: bool = True) -> Tuple[Tensor, Tensor]:
    """``botorch.optim.optimize_acqf`` for the no-constraint, non-sequential case the reference uses: q = 1
    (``acquisition_optimisation_strategy.py:217-224, 259-266``) and the joint optimisation of a q-batch
    (``:435-443``; every restart is a ``q x d`` point, and the initialiser and ``gen_candidates_scipy`` take any q)."""
    if q < 1:
        raise ValueError(f"q must be at least 1, got {q}")
    options = dict(options or {})
    if batch_initial_conditions is None:
        if raw_samples is None:
            raise ValueError("Must specify `raw_samples` when `batch_initial_conditions` is None`.")
        batch_initial_conditions = gen_batch_initial_conditions(acq_function, bounds, q, num_restarts, raw_samples,
                                                                options)
    batch_limit = int(options.get("batch_limit", num_restarts) or num_restarts)
    gen_opts = {k: v for k, v in options.items() if k not in INIT_OPTION_KEYS}
    cands: List[Tensor] = []
    vals: List[Tensor] = []
    for start in range(0, batch_initial_conditions.shape[0], batch_limit):
        c, v = gen_candidates_scipy(batch_initial_conditions[start:start + batch_limit], acq_function,
                                    bounds[0], bounds[1], gen_opts)
        cands.append(c)
        vals.append(v.reshape(-1))
    batch_candidates = torch.cat(cands)
    batch_acq_values = torch.cat(vals)
    if return_best_only:
        best = int(torch.argmax(batch_acq_values))
        return batch_candidates[best], batch_acq_values[best]
    return batch_candidates, batch_acq_values


def joint_best_per_cost(kg: Tensor, costs) -> Tuple[Tensor, Tensor]:
    """The decoupled decision at fixed candidates: ``kg [T, *batch]`` (row t: KG observing objective t alone)
    -> ``(max_t max(KG_t, 0) / cost_t [*batch], the winning t [*batch])``.  ``_choose_best_objective``'s rule
    per candidate: negative values clip to 0, ties go to the cheaper objective, then to the lower index."""
    c = [float(x) for x in costs]
    if kg.shape[0] != len(c):
        raise ValueError(f"{kg.shape[0]} targets but {len(c)} costs")
    best = kg[0].clamp_min(0) / c[0]
    win = torch.zeros(kg.shape[1:], dtype=torch.long, device=kg.device)
    wcost = torch.full(kg.shape[1:], c[0], dtype=kg.dtype, device=kg.device)
    for t in range(1, len(c)):
        v = kg[t].clamp_min(0) / c[t]
        take = (v > best) | ((v == best) & (c[t] < wcost))
        best = torch.where(take, v, best)
        win = torch.where(take, torch.full_like(win, t), win)
        wcost = torch.where(take, torch.full_like(wcost, c[t]), wcost)
    return best, win


class JointDecoupledAcquisition:
    """``A(x) = max_t max(KG_t(x), 0) / cost_t`` over the m single-objective targets, as one acquisition for
    ``optimize_acqf`` (``optimize_for_single_objective(joint=True)``).

    ``acqs``: one acquisition with ``forward_targets`` / ``value_and_grad_host_targets`` (the device
    ``DiscreteKnowledgeGradient``: every evaluation is one pass over the shared stages for all targets), or a
    list of m acquisitions, one per objective, whose ``forward``s are combined (an injected acquisition
    without the multi-target entries).  The gradient of A is the winning target's dKG/dx / cost where its KG
    is positive, 0 where the clip holds."""

    def __init__(self, acqs, costs, num_outputs: int):
        self.m = int(num_outputs)
        self.costs = [float(costs[i]) for i in range(self.m)]
        self.targets = list(range(self.m))
        self.acqs = acqs
        self.shared = not isinstance(acqs, (list, tuple))
        if not self.shared and len(acqs) != self.m:
            raise ValueError(f"{len(acqs)} acquisitions for {self.m} objectives")
        if self.shared and hasattr(acqs, "value_and_grad_host_targets"):
            self.value_and_grad_host = self._value_and_grad_host  # gen_candidates_scipy's one-round-trip route

    def per_target(self, X: Tensor) -> Tensor:
        """KG_t(X) for every objective t: ``[m, *batch]``."""
        if self.shared:
            return self.acqs.forward_targets(X, targets=self.targets)
        return torch.stack([a(X) for a in self.acqs])

    def __call__(self, X: Tensor) -> Tensor:
        kg = self.per_target(X)
        _, win = joint_best_per_cost(kg.detach(), self.costs)
        c = torch.tensor(self.costs, dtype=kg.dtype, device=kg.device)
        return kg.gather(0, win.unsqueeze(0)).squeeze(0).clamp_min(0) / c[win]

    def _value_and_grad_host(self, X: Tensor):
        kg, dkg = self.acqs.value_and_grad_host_targets(X, targets=self.targets)  # [m, *batch], [m, *X.shape]
        best, win = joint_best_per_cost(kg, self.costs)
        c = torch.tensor(self.costs, dtype=kg.dtype)
        kw = kg.gather(0, win.unsqueeze(0)).squeeze(0)
        idx = win.reshape((1,) + tuple(win.shape) + (1,) * (dkg.dim() - 1 - win.dim())).expand((1,) + dkg.shape[1:])
        scale = torch.where(kw > 0, 1.0 / c[win], torch.zeros_like(kw))
        g = dkg.gather(0, idx).squeeze(0) * scale.reshape(tuple(scale.shape) + (1,) * (dkg.dim() - 1 - win.dim()))
        return best, g


def _get_standard_bounds(dim: int, dtype=torch.double) -> Tensor:
    """``acquisition_optimisation_strategy.py:555``: the unit cube."""
    return torch.stack([torch.zeros(dim, dtype=dtype), torch.ones(dim, dtype=dtype)])


class DiscreteKgOptimisationSpec:
    """``DiscreteKgOptimisationSpec`` (``acquisition_optimisation_strategy.py:166-273``) on the
    device KG: same constructor, same two entry points, same tie-breaking.

    ``n_discretisation_points_per_axis``: grid points per axis of the discretisation
    (``make_torch_std_grid``); ``num_restarts`` / ``raw_samples`` / ``batch_limit`` /
    ``max_iter``: passed to ``optimize_acqf`` exactly as the reference does (:217-224).

    The gradient plans of the acquisitions it builds follow the module default of
    ``dkg_amd.set_gradient_rows`` (no argument here): under ``"staged"`` a model whose gradient rows do not
    fit in LDS raises ``UnsupportedError``, under ``"auto"`` it is optimised with global rows.
    """

    def __init__(self, n_discretisation_points_per_axis: int, num_restarts: int, raw_samples: int,
                 batch_limit: int, max_iter: int, device=None, seed: Optional[int] = None,
                 acq_factory: Optional[Callable] = None):
        self.n_discretisation_points_per_axis = n_discretisation_points_per_axis
        self.num_restarts = num_restarts
        self.raw_samples = raw_samples
        self.batch_limit = batch_limit
        self.max_iter = max_iter
        self.device = device
        self.seed = seed
        # acq_factory(model, x_discretisation, scalarisation_weights, target_output_ix) -> acquisition:
        # None builds the device DiscreteKnowledgeGradient (tests inject the oracle's KG to compare runs)
        self.acq_factory = acq_factory

    def _options(self) -> Dict:
        opts = {"batch_limit": self.batch_limit, "maxiter": self.max_iter}
        if self.seed is not None:
            opts["seed"] = self.seed
        return opts

    def _acq(self, model, input_dim: int, scalarisation_weights: Tensor, target: Optional[int]):
        from .discretekg import DiscreteKnowledgeGradient
        from .utils import make_torch_std_grid

        disc = make_torch_std_grid(self.n_discretisation_points_per_axis, input_dim, {"dtype": torch.double})
        if self.acq_factory is not None:
            return self.acq_factory(model, disc, scalarisation_weights, target)
        return DiscreteKnowledgeGradient(model, x_discretisation=disc, scalarisation_weights=scalarisation_weights,
                                         target_output_ix=target, device=self.device)

    def optimize_for_single_objective(self, model, costs: Union[Tensor, Sequence], input_dim: int, *,
                                      scalarisation_weights: Tensor, joint: bool = False,
                                      **_unused_kwargs) -> Tuple[Tensor, int, Tensor]:
        """Decoupled KG per objective, best KG per cost (:196-240).

        ``joint=True`` (not the reference's search; opt-in): one ``optimize_acqf`` run on
        ``A(x) = max_t max(KG_t(x), 0) / cost_t`` (``JointDecoupledAcquisition``) instead of one run per
        objective.  In exact arithmetic the maximum of A is the reference's decision -- the best objective's
        best point per cost -- but the local search differs: one set of raw samples and restarts follows the
        upper envelope of the m scaled surfaces, where the reference gives every objective its own restarts.
        On the device KG every evaluation is one pass over the shared cross and covariance stages for all m
        targets (``value_and_grad_host_targets``).  Returns the same triple."""
        from .discretekg import _as_model_state

        standard_bounds = _get_standard_bounds(input_dim)
        m = _as_model_state(model).num_outputs
        if joint:
            # the device KG evaluates every target on one acquisition; an injected acquisition without
            # value_and_grad_host_targets is built once per objective and combined from the m forwards
            acqs = self._acq(model, input_dim, scalarisation_weights, 0)
            if not hasattr(acqs, "value_and_grad_host_targets"):
                acqs = [acqs] + [self._acq(model, input_dim, scalarisation_weights, i) for i in range(1, m)]
            acq_func = JointDecoupledAcquisition(acqs, costs, m)
            candidate_x, _ = optimize_acqf(acq_function=acq_func, bounds=standard_bounds, q=1,
                                           num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                           options=self._options())
            candidate_x = candidate_x.detach()
            with torch.no_grad():
                kg = acq_func.per_target(candidate_x.unsqueeze(0)).reshape(m)
            best_i = int(joint_best_per_cost(kg, acq_func.costs)[1])
            if kg[best_i] < 0:
                logger.warning("Optimal acquisition function value is negative: obj_index=%i, acq_value=%f", best_i,
                               kg[best_i])
            return candidate_x, best_i, (kg[best_i] / acq_func.costs[best_i]).detach()
        candidates = []
        for i in range(m):
            acq_func = self._acq(model, input_dim, scalarisation_weights, i)
            candidate_x, acq_value = optimize_acqf(acq_function=acq_func, bounds=standard_bounds, q=1,
                                                   num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                                   options=self._options())
            if acq_value < 0:
                logger.warning("Optimal acquisition function value is negative: obj_index=%i, acq_value=%f", i,
                               acq_value)
            candidates.append((i, candidate_x.detach(), acq_value.detach()))
        best_i, best_x, best_kg_per_cost = self._choose_best_objective(candidates, costs)
        return best_x, best_i, best_kg_per_cost

    def optimize_for_full_evaluation(self, model, input_dim: int, *, scalarisation_weights: Tensor,
                                     **_unused_kwargs) -> Tuple[Tensor, Tensor]:
        """Coupled (full-evaluation) KG (:242-273)."""
        acq_func = self._acq(model, input_dim, scalarisation_weights, None)
        candidate_x, acq_value = optimize_acqf(acq_function=acq_func, bounds=_get_standard_bounds(input_dim), q=1,
                                               num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                               options=self._options())
        if acq_value < 0:
            logger.warning("Optimal acquisition function value is negative: acq_value=%f", acq_value)
        return candidate_x.detach(), acq_value.detach()

    @staticmethod
    def _choose_best_objective(candidates, costs):
        """:143-163 — clip negative values to 0, maximise value / cost, ties to the cheaper objective."""
        best_i, best_x, best_acq_value = max(candidates, key=lambda x: (max(x[-1], 0) / costs[x[0]], -costs[x[0]]))
        return best_i, best_x, best_acq_value / costs[best_i]


class JesOptimisationSpec:
    """``JesOptimisationSpec`` (``acquisition_optimisation_strategy.py:447-552``) on the device joint entropy
    search: the reference's constructor arguments, its two entry points and its ``_choose_best_objective`` rule
    (JES carries no cost-aware utility, so the decoupled decision is value per cost, :511-513).

    ``pareto_sampler(model, bounds, num_samples, target_num_points) -> (pareto_sets, pareto_fronts)`` is required:
    the reference samples GP paths by random Fourier features, runs NSGA-II on each and prunes the fronts
    (``sample_discrete_pareto_optimal_points``, ``jes_sample_pareto.py``); ``with_device_sampler`` builds a spec whose
    sampler is this library's (``dkg_amd.jes_pareto``).  The sets are
    in the model's input space (the unit cube), the fronts in the untransformed output space; samples may hold
    different numbers of points.  The boxes come from ``compute_sample_box_decomposition`` on the host for one or
    two objectives and from ``dkg_amd.boxes.dominated_boxes`` on the spec's device for three;
    ``hypercell_bounds_fn(pareto_fronts)`` replaces either.
    """

    def __init__(self, estimation_type: str, num_pareto_samples: int, num_pareto_points: int, num_restarts: int,
                 raw_samples: int, batch_limit: int, max_iter: int, pareto_sampler: Callable, device=None,
                 seed: Optional[int] = None, acq_factory: Optional[Callable] = None,
                 hypercell_bounds_fn: Optional[Callable] = None, conditioning: str = "refactorise"):
        if not callable(pareto_sampler):
            raise TypeError("pareto_sampler(model, bounds, num_samples, target_num_points) must be callable")
        self.estimation_type = estimation_type
        self.num_pareto_samples = num_pareto_samples
        self.num_pareto_points = num_pareto_points
        self.num_restarts = num_restarts
        self.raw_samples = raw_samples
        self.batch_limit = batch_limit
        self.max_iter = max_iter
        self.pareto_sampler = pareto_sampler
        self.device = device
        self.seed = seed
        # acq_factory(model, pareto_sets, pareto_fronts, hypercell_bounds, estimation_type, target_output_ix) ->
        # acquisition: None builds the device acquisition (tests inject the CPU restatement to compare runs)
        self.acq_factory = acq_factory
        self.hypercell_bounds_fn = hypercell_bounds_fn
        # how the device acquisition builds its conditioned states ("refactorise" / "append", dkg_amd.jes)
        self.conditioning = conditioning

    @classmethod
    def with_device_sampler(cls, estimation_type: str, num_pareto_samples: int, num_pareto_points: int,
                            num_restarts: int, raw_samples: int, batch_limit: int, max_iter: int, device=None,
                            seed: Optional[int] = None, acq_factory: Optional[Callable] = None,
                            hypercell_bounds_fn: Optional[Callable] = None, conditioning: str = "refactorise",
                            **sampler_kwargs) -> "JesOptimisationSpec":
        """A spec whose Pareto samples come from the device sampler
        (``jes_pareto.sample_discrete_pareto_optimal_points``: random-Fourier-feature paths, NSGA-II and pruning,
        ``jes_sample_pareto.py:48-98``), as the reference's spec does at
        ``acquisition_optimisation_strategy.py:481-489, 526-534``.  ``sampler_kwargs`` go to the sampler
        (``num_rffs``, ``nsga2_pop_size``, ``nsga2_generations``, ``mutation_prob``); ``seed`` seeds both the
        sampler's draws and ``optimize_acqf``'s."""
        from .jes_pareto import sample_discrete_pareto_optimal_points

        def sampler(model, bounds, num_samples, target_num_points):
            return sample_discrete_pareto_optimal_points(model, bounds, num_samples, target_num_points, seed=seed,
                                                         device=device, **sampler_kwargs)

        return cls(estimation_type, num_pareto_samples, num_pareto_points, num_restarts, raw_samples, batch_limit,
                   max_iter, pareto_sampler=sampler, device=device, seed=seed, acq_factory=acq_factory,
                   hypercell_bounds_fn=hypercell_bounds_fn, conditioning=conditioning)

    def _options(self) -> Dict:
        opts = {"batch_limit": self.batch_limit, "maxiter": self.max_iter}
        if self.seed is not None:
            opts["seed"] = self.seed
        return opts

    def _samples(self, model, input_dim: int):
        from .jes import compute_sample_box_decomposition

        pareto_sets, pareto_fronts = self.pareto_sampler(model, _get_standard_bounds(input_dim),
                                                         num_samples=self.num_pareto_samples,
                                                         target_num_points=self.num_pareto_points)
        fn = self.hypercell_bounds_fn
        if fn is None:
            if pareto_fronts[0].shape[-1] >= 3:  # m <= 2 keeps the host function and its bits
                from .boxes import dominated_boxes

                return pareto_sets, pareto_fronts, dominated_boxes(pareto_fronts, device=self.device)
            fn = compute_sample_box_decomposition
        return pareto_sets, pareto_fronts, fn(pareto_fronts)

    def _acq(self, model, samples, target: Optional[int]):
        from .jes import qLowerBoundMultiObjectiveJointEntropySearch

        pareto_sets, pareto_fronts, hypercell_bounds = samples
        if self.acq_factory is not None:
            return self.acq_factory(model, pareto_sets, pareto_fronts, hypercell_bounds, self.estimation_type, target)
        return qLowerBoundMultiObjectiveJointEntropySearch(model, pareto_sets, pareto_fronts, hypercell_bounds,
                                                           estimation_type=self.estimation_type,
                                                           target_output_ix=target, device=self.device,
                                                           conditioning=self.conditioning)

    def optimize_for_single_objective(self, model, costs: Union[Tensor, Sequence], input_dim: int,
                                      **_unused_kwargs) -> Tuple[Tensor, int, Tensor]:
        """One acquisition per objective on the same Pareto samples, best value per cost (:467-515)."""
        from .discretekg import _as_model_state

        samples = self._samples(model, input_dim)
        candidates = []
        for i in range(_as_model_state(model).num_outputs):
            candidate_x, acq_value = optimize_acqf(acq_function=self._acq(model, samples, i),
                                                   bounds=_get_standard_bounds(input_dim), q=1,
                                                   num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                                   options=self._options())
            candidates.append((i, candidate_x.detach(), acq_value.detach()))
        best_i, best_x, best_acqval_per_cost = self._choose_best_objective(candidates, costs)
        return best_x, best_i, best_acqval_per_cost

    def optimize_for_full_evaluation(self, model, input_dim: int, **_unused_kwargs) -> Tuple[Tensor, Tensor]:
        """All outputs observed (:517-552)."""
        samples = self._samples(model, input_dim)
        candidate_x, acq_value = optimize_acqf(acq_function=self._acq(model, samples, None),
                                               bounds=_get_standard_bounds(input_dim), q=1,
                                               num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                               options=self._options())
        return candidate_x.detach(), acq_value.detach()

    _choose_best_objective = staticmethod(DiscreteKgOptimisationSpec._choose_best_objective)


class HvkgOptimisationSpec:
    """``HvkgOptimisationSpec`` (``acquisition_optimisation_strategy.py:276-444``) on the device hypervolume
    knowledge gradient: the reference's constructor arguments, its two entry points with their ``hv_refpoint``
    keyword and their warnings.  The decoupled decision is the argmax of the per-objective values: the cost is
    inside the acquisition (its cost-aware utility), so it is not ``_choose_best_objective`` (:382-386).

    The current optimum is the best value of the value function (``PosteriorMeanHypervolume``) over
    ``q = num_pareto`` points (``_compute_current_optimum``, :428-444).

    One-shot initial conditions are this library's own (BoTorch's ``gen_one_shot_hvkg_initial_conditions`` is
    absent, so parity with it is unpinned): ``raw_samples`` Sobol candidates, each with the current
    optimum's Pareto set repeated over the fantasies as its fantasy rows, evaluated without gradient in chunks,
    ``num_restarts`` of them picked by ``initialize_q_batch``; L-BFGS-B then moves every row of the one-shot
    points inside the unit cube, and the candidate returned is ``extract_candidates`` of the best restart.

    ``acq_factory(kind, model, ref_point, **kwargs)`` (tests inject a CPU restatement): ``kind`` is
    ``"value_function"`` (no kwargs) or ``"hvkg"`` (``num_fantasies``, ``num_pareto``, ``current_value``,
    ``cost_aware_utility``, ``seed``); ``None`` builds the device acquisitions."""

    INIT_CHUNK = 512  # one-shot points per evaluation of the raw-sample screen

    def __init__(self, num_pareto: int, num_fantasies: int, num_restarts: int, raw_samples: int,
                 curr_opt_num_restarts: int, curr_opt_raw_samples: int, batch_limit: int, max_iter: int, device=None,
                 seed: Optional[int] = None, acq_factory: Optional[Callable] = None):
        self.num_pareto = num_pareto
        self.num_fantasies = num_fantasies
        self.num_restarts = num_restarts
        self.raw_samples = raw_samples
        self.curr_opt_num_restarts = curr_opt_num_restarts
        self.curr_opt_raw_samples = curr_opt_raw_samples
        self.batch_limit = batch_limit
        self.max_iter = max_iter
        self.device = device
        self.seed = seed
        self.acq_factory = acq_factory

    def _seeded(self, opts: Dict) -> Dict:
        if self.seed is not None:
            opts["seed"] = self.seed
        return opts

    def _value_function(self, model, ref_point):
        if self.acq_factory is not None:
            return self.acq_factory("value_function", model, ref_point)
        from .hvkg import PosteriorMeanHypervolume

        return PosteriorMeanHypervolume(model, ref_point, device=self.device)

    def _acq(self, model, ref_point, current_value, costs):
        kw = dict(num_fantasies=self.num_fantasies, num_pareto=self.num_pareto, current_value=current_value,
                  cost_aware_utility=costs, seed=self.seed)
        if self.acq_factory is not None:
            return self.acq_factory("hvkg", model, ref_point, **kw)
        from .hvkg import qHypervolumeKnowledgeGradient

        return qHypervolumeKnowledgeGradient(model, ref_point, device=self.device, **kw)

    def _compute_current_optimum(self, model, ref_point, bounds) -> Tuple[Tensor, Tensor]:
        """The hypervolume-maximising set of ``num_pareto`` points under the posterior mean and its hypervolume."""
        pareto_set, current_optimum = optimize_acqf(
            acq_function=self._value_function(model, ref_point), bounds=bounds, q=self.num_pareto,
            num_restarts=self.curr_opt_num_restarts, raw_samples=self.curr_opt_raw_samples,
            options=self._seeded({"batch_limit": self.batch_limit}))
        return pareto_set.detach(), current_optimum.detach()

    def _optimize_one_shot(self, acq_func, bounds: Tensor, pareto_set: Tensor) -> Tuple[Tensor, Tensor]:
        candidates = draw_sobol_samples(bounds, self.raw_samples, 1, seed=self.seed)            # [raw, 1, d]
        fantasy_rows = pareto_set.to(candidates).repeat(self.num_fantasies, 1)                  # [Nf Np, d]
        X_raw = torch.cat([candidates, fantasy_rows.expand(self.raw_samples, -1, -1)], dim=1)
        Y_raw = _no_grad_values(acq_func, X_raw, self.INIT_CHUNK)
        ic = initialize_q_batch(X_raw, Y_raw.to(X_raw), n=self.num_restarts)
        X_full, acq_value = optimize_acqf(acq_function=acq_func, bounds=bounds, q=X_raw.shape[1],
                                          num_restarts=self.num_restarts, batch_initial_conditions=ic,
                                          options={"batch_limit": self.batch_limit, "maxiter": self.max_iter})
        return acq_func.extract_candidates(X_full).detach(), acq_value.detach()

    def optimize_for_single_objective(self, model, costs: Union[Tensor, Sequence], input_dim: int, *,
                                      hv_refpoint: Tensor, **_unused_kwargs) -> Tuple[Tensor, int, Tensor]:
        """One mask per objective on one acquisition, the best value wins (:322-388)."""
        from .discretekg import _as_model_state

        bounds = _get_standard_bounds(input_dim)
        pareto_set, current_opt = self._compute_current_optimum(model, hv_refpoint, bounds)
        m = _as_model_state(model).num_outputs
        acq_func = self._acq(model, hv_refpoint, current_opt, [float(c) for c in torch.as_tensor(costs).reshape(-1)])
        objective_candidates, objective_vals = [], []
        for i in range(m):
            evaluation_mask = torch.zeros(1, m, dtype=torch.bool)
            evaluation_mask[0, i] = 1
            acq_func.X_evaluation_mask = evaluation_mask
            candidate_x, acq_value = self._optimize_one_shot(acq_func, bounds, pareto_set)
            if acq_value <= 0:
                logger.warning("Optimal acquisition function value is not strictly positive "
                               "(after clipping to be at least zero): obj_index=%i, acq_value=%f", i, acq_value)
            objective_candidates.append(candidate_x)
            objective_vals.append(acq_value)
        best_i = int(torch.stack(objective_vals).argmax().item())
        return objective_candidates[best_i], best_i, objective_vals[best_i]

    def optimize_for_full_evaluation(self, model, input_dim: int, *, hv_refpoint: Tensor,
                                     **_unused_kwargs) -> Tuple[Tensor, Tensor]:
        """Every output observed, no cost-aware utility (:390-426)."""
        bounds = _get_standard_bounds(input_dim)
        pareto_set, current_opt = self._compute_current_optimum(model, hv_refpoint, bounds)
        acq_func = self._acq(model, hv_refpoint, current_opt, None)
        candidate_x, acq_value = self._optimize_one_shot(acq_func, bounds, pareto_set)
        if acq_value < 0:
            logger.warning("Optimal acquisition function value is negative: acq_value=%f", acq_value)
        return candidate_x, acq_value
