"""Hypervolume knowledge gradient (HVKG, Daulton et al., ICML 2023) on MI355X -- host mirror.

The surface of BoTorch's ``qHypervolumeKnowledgeGradient`` as the reference's ``HvkgOptimisationSpec`` drives it
(``modules/acquisition_optimisation_strategy.py:276-444``): q = 1, one-shot, the posterior mean as the inner value
function, ``X_evaluation_mask`` for the decoupled runs, ``current_value`` and a cost-aware utility of fixed
per-output costs:

* ``qHypervolumeKnowledgeGradient(model, ref_point, num_fantasies=8, num_pareto=10, X_evaluation_mask=None,
  current_value=None, cost_aware_utility=None, base_samples=None, seed=None, device=None)`` with
  ``forward(X_full[*batch, 1 + num_fantasies * num_pareto, d]) -> [*batch]`` (differentiable),
  ``value_and_grad_host``, ``get_augmented_q_batch_size`` and ``extract_candidates``;
* ``PosteriorMeanHypervolume(model, ref_point, device=None)``: the value function, the hypervolume of the posterior
  mean at q <= 32 points, ``forward(X[*batch, q, d])`` (``_compute_current_optimum`` optimises it, :428-444).

A one-shot point holds the candidate in row 0 and point p of fantasy f in row ``1 + f * num_pareto + p``
(BoTorch's layout).  The fantasy model is never built: the posterior mean after observing
``mu_i(x) + sigma~_i(x) z_f,i`` at the candidate is ``mu_i(x') + z_f,i c_i(x', x) / sigma~_i(x)`` in closed form
(DESIGN.md 8f).  Every evaluation is four HIP kernel launches through the C ABI (``include/dkg.h`` ``dkg_hvkg_*``),
three for the value function.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib, _plan
from .discretekg import _as_model_state, _Base, _fingerprint, _HAVE_BOTORCH, shared_state
from .errors import UnsupportedError
from .gp_state import current_stream_ptr
from .utils import sobol_draw

MIN_PLAN_RESTARTS = 16


def hypervolume_limits(m: int, num_fantasies: int, num_pareto: int) -> None:
    """The limits of ``dkg_hvkg_init`` that do not depend on the batch, raised as ``UnsupportedError``."""
    if m not in (2, 3):
        raise UnsupportedError(
            f"the hypervolume kernels handle 2 or 3 objectives; the model has {m} (m = 1 and m > 3 are not built)")
    if num_fantasies > _lib.DKG_HVKG_MAX_FANTASIES:
        raise UnsupportedError(f"num_fantasies={num_fantasies} > {_lib.DKG_HVKG_MAX_FANTASIES}")
    if num_pareto > _lib.DKG_HVKG_MAX_PARETO:
        raise UnsupportedError(f"num_pareto={num_pareto} > {_lib.DKG_HVKG_MAX_PARETO}")


class HvkgPlan(_plan.Plan):
    """A ``dkg_hvkg_*`` plan (include/dkg.h): the outputs, the reference point, the base samples, the mask and the
    two scalars, with the workspace for up to ``max_B`` restarts.  ``mask = 0`` is the value function."""

    def __init__(self, structs, m: int, d: int, ref_point, num_fantasies: int, num_pareto: int, base_samples,
                 mask: int, current_value: float, cost: float, max_B: int, device):
        lib = _lib.load()
        self.m, self.d = m, d
        self.Nf, self.Np = int(num_fantasies), int(num_pareto)
        self.rows = self.Nf * self.Np + (1 if mask else 0)
        super().__init__(device, lib.dkg_hvkg_plan_bytes(),
                         lib.dkg_hvkg_workspace(m, d, self.Nf, self.Np, int(max_B)), max_B)
        ref = (ctypes.c_double * m)(*[float(v) for v in ref_point])
        z = None
        if mask:
            z = (ctypes.c_double * (self.Nf * m))(*[float(v) for v in base_samples.reshape(-1).tolist()])
        _lib.check(lib.dkg_hvkg_init(structs, m, d, ref, self.Nf, self.Np, z, int(mask), float(current_value),
                                     float(cost), self.max_B, _lib.ptr(self.ws), self.ws.numel(), self.host,
                                     current_stream_ptr(device)), "dkg_hvkg_init")
        self._fwd = lib.dkg_hvkg_forward

    def forward(self, X: Tensor, grad: bool = False, means: bool = False):
        """``X``: device fp64 ``[B, rows, d]``.  -> ``out`` (device; with the gradient ``[B * (1 + rows * d)]``:
        ``out[:B]`` the values, ``out[B:]`` dacq/dX row-major; else ``[B]``) and, with ``means``, the fantasised
        means ``[B, Nf, Np, m]``."""
        B = X.shape[0]
        Y = torch.empty(B, self.Nf, self.Np, self.m, dtype=torch.double, device=self.device) if means else None
        out = self._forward(self._fwd, "dkg_hvkg_forward", X, self.rows * self.d, grad, Y)
        return (out, Y) if means else out


def hypervolume_device(Y: Tensor, ref_point, grad: bool = False):
    """``dkg_hypervolume``: the hypervolume stage alone on device sets ``Y [S, Np, m]`` (fp64) ->
    ``hv [S]`` and, with ``grad``, ``dhv [S, Np, m]``."""
    lib = _lib.load()
    if Y.dim() != 3 or Y.dtype is not torch.double or Y.device.type != "cuda":
        raise ValueError("Expected a device fp64 tensor of shape `S x num_pareto x m`.")
    S, Np, m = Y.shape
    Y = Y.contiguous()
    ref = (ctypes.c_double * m)(*[float(v) for v in torch.as_tensor(ref_point).reshape(-1).tolist()])
    hv = torch.empty(S, dtype=torch.double, device=Y.device)
    dhv = torch.empty(S, Np, m, dtype=torch.double, device=Y.device) if grad else None
    with torch.cuda.device(Y.device):
        _lib.check(lib.dkg_hypervolume(_lib.ptr(Y), S, Np, m, ref, _lib.ptr(hv), _lib.ptr(dhv),
                                       current_stream_ptr(Y.device)), "dkg_hypervolume")
    return (hv, dhv) if grad else hv


class _HypervolumeBase(_Base):
    """What the two acquisitions share: the model read live (``_fingerprint``), its device state shared through
    ``shared_state`` over an empty discretisation, the plan cache and the two evaluation routes."""

    def __init__(self, model, ref_point, device) -> None:
        if _HAVE_BOTORCH:  # pragma: no cover
            super().__init__(model=model)
        else:
            super().__init__()
            self.model = model
        state = _as_model_state(model)
        self._m, self._d = state.num_outputs, state.input_dim
        ref = torch.as_tensor(ref_point).detach().to("cpu", torch.double).reshape(-1)
        if ref.shape[0] != self._m:
            raise ValueError(
                f"The length of the reference point must match the number of outcomes. Got ref_point with "
                f"{ref.shape[0]} elements, but expected {self._m}.")
        self.ref_point = ref
        dev = _plan.hip_device(device, "hypervolume")
        if self._d > _lib.MAX_DIM:
            raise UnsupportedError(f"input dimension {self._d} > {_lib.MAX_DIM}")
        self._device = dev
        self._fp = None
        self._state = None
        self._plans = {}

    def _refresh(self) -> None:
        """Rebuild the device state, and with it the plans, if the model changed since it was read."""
        fp = _fingerprint(self.model)
        if fp != self._fp or self._state is None:
            empty = torch.empty(0, self._d, dtype=torch.double)
            with torch.cuda.device(self._device):
                self._state = shared_state(_as_model_state(self.model), fp, empty, self._device, owner=self.model)
            self._plans = {}
            self._fp = fp

    def _plan_args(self, rows: int):  # -> (key, num_fantasies, num_pareto, base_samples, mask, current, cost)
        raise NotImplementedError

    def _plan_for(self, B: int, rows: int) -> HvkgPlan:
        """The plan, grown in powers of two (at least 16) to hold B restarts."""
        self._refresh()
        if B > _lib.DKG_HVKG_MAX_RESTARTS:
            raise UnsupportedError(f"{B} restarts in one evaluation > {_lib.DKG_HVKG_MAX_RESTARTS}")
        key, Nf, Np, z, mask, current, cost = self._plan_args(rows)
        plan = self._plans.get(key)
        if plan is None or plan.max_B < B:
            cap = _plan.grow(B, MIN_PLAN_RESTARTS, _lib.DKG_HVKG_MAX_RESTARTS)
            with torch.cuda.device(self._device):
                plan = HvkgPlan(self._state.structs, self._m, self._d, self.ref_point.tolist(), Nf, Np, z, mask,
                                current, cost, cap, self._device)
            self._plans[key] = plan
        return plan

    def _check_x(self, X: Tensor) -> None:
        if X.dim() < 2:
            raise ValueError(
                f"{type(self).__name__} requires X to have at least 2 dimensions, but received X with only "
                f"{X.dim()} dimensions.")
        if X.shape[-1] != self._d:
            raise RuntimeError(f"Expected X to have last dimension {self._d} (the model's inputs). Got {X.shape[-1]=}.")
        self._check_rows(X.shape[-2])

    def _check_rows(self, rows: int) -> None:
        raise NotImplementedError

    def forward(self, X: Tensor) -> Tensor:
        self._check_x(X)
        if X.dim() == 2:
            X = X.unsqueeze(0)
        if X.device.type == "cpu":
            return _plan.HostForwardFn.apply(X, self)
        batch = X.shape[:-2]
        Xd = X.reshape((-1,) + tuple(X.shape[-2:])).to(self._device, torch.double)
        return _plan.ForwardFn.apply(Xd, self).to(device=X.device, dtype=X.dtype).reshape(batch)

    def _host_x(self, X: Tensor):
        self._check_x(X)
        if X.dim() == 2:
            X = X.unsqueeze(0)
        return X.detach().to("cpu", torch.double).reshape((-1,) + tuple(X.shape[-2:])), X.shape[:-2], X.shape

    def _values_host(self, X: Tensor) -> Tensor:
        xs, batch, _ = self._host_x(X)
        return self._plan_for(xs.shape[0], xs.shape[1]).forward(xs.to(self._device)).cpu().reshape(batch)

    def value_and_grad_host(self, X: Tensor):
        """acq and dacq/dX for host points X ``[*batch, rows, d]`` as host fp64 tensors of shapes ``batch`` and
        ``[*batch, rows, d]``: what one L-BFGS-B evaluation of ``optimize_acqf`` needs back, in one device round
        trip (one copy in, the launches, one copy of [acq | dacq/dX] out) and no autograd graph.  The same bits as
        ``forward`` + autograd."""
        xs, batch, shape = self._host_x(X)
        B = xs.shape[0]
        out = self._plan_for(B, xs.shape[1]).forward(xs.to(self._device), grad=True).cpu()
        return out[:B].reshape(batch), out[B:].reshape(shape)


class qHypervolumeKnowledgeGradient(_HypervolumeBase):
    """The one-shot hypervolume knowledge gradient, q = 1, with the posterior mean as the inner value function."""

    def __init__(self, model, ref_point, num_fantasies: int = 8, num_pareto: int = 10, sampler=None, objective=None,
                 inner_sampler=None, X_evaluation_mask: Optional[Tensor] = None, X_pending: Optional[Tensor] = None,
                 current_value=None, use_posterior_mean: bool = True, cost_aware_utility: Optional[Sequence] = None,
                 base_samples: Optional[Tensor] = None, seed: Optional[int] = None, device=None) -> None:
        for name, given in (("sampler", sampler), ("objective", objective), ("inner_sampler", inner_sampler),
                            ("X_pending", X_pending)):
            if given is not None:
                raise UnsupportedError(f"{type(self).__name__} on the device does not take `{name}`.")
        if not use_posterior_mean:
            raise UnsupportedError(
                f"{type(self).__name__} on the device uses the posterior mean as its inner value function; "
                "use_posterior_mean=False (the Monte Carlo value function) is not built.")
        if num_fantasies is None or int(num_fantasies) < 1:
            raise ValueError("Must specify `num_fantasies` >= 1.")
        if int(num_pareto) < 1:
            raise ValueError("Must specify `num_pareto` >= 1.")
        if current_value is None and cost_aware_utility is not None:
            raise ValueError("Cost-aware HV-KG requires current_value to be specified.")
        super().__init__(model, ref_point, device)
        self.num_fantasies, self.num_pareto = int(num_fantasies), int(num_pareto)
        hypervolume_limits(self._m, self.num_fantasies, self.num_pareto)
        self.num_pseudo_points = self.num_fantasies * self.num_pareto
        self.current_value = current_value
        self._current = 0.0 if current_value is None else float(torch.as_tensor(current_value).reshape(()))
        self.cost_aware_utility = cost_aware_utility
        self._costs = None
        if cost_aware_utility is not None:
            costs = [float(c) for c in torch.as_tensor(cost_aware_utility).reshape(-1).tolist()]
            if len(costs) != self._m or not all(c > 0 and math.isfinite(c) for c in costs):
                raise ValueError(f"Expected cost_aware_utility to hold {self._m} positive per-output costs. Got {costs}.")
            self._costs = costs
        if base_samples is None:
            base_samples = self._sobol_normal(seed)
        z = torch.as_tensor(base_samples).detach().to("cpu", torch.double)
        if tuple(z.shape) != (self.num_fantasies, self._m):
            raise ValueError(
                f"Expected base_samples of shape `num_fantasies x m` = {self.num_fantasies} x {self._m}. "
                f"Got {tuple(z.shape)}.")
        self.base_samples = z.contiguous()
        self.X_pending = None
        self._mask_bits = (1 << self._m) - 1
        self._mask_tensor = None
        self.X_evaluation_mask = X_evaluation_mask

    def _sobol_normal(self, seed: Optional[int]) -> Tensor:
        """``[num_fantasies, m]`` standard normal draws, one scrambled Sobol engine per output (what BoTorch's
        default ``ListSampler`` of ``SobolQMCNormalSampler``s gives each output), the engines seeded from a
        generator of its own seeded by ``seed``: the global generator is not read."""
        gen = torch.Generator()
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        seeds = torch.randint(0, 2**31 - 1, (self._m,), generator=gen).tolist()
        cols = []
        for s in seeds:
            u = sobol_draw(1, self.num_fantasies, int(s), torch.double)[:, 0]
            u = u.clamp(1e-12, 1.0 - 1e-12)
            cols.append(math.sqrt(2.0) * torch.erfinv(2.0 * u - 1.0))
        return torch.stack(cols, dim=-1)

    # -- X_evaluation_mask: a settable attribute, [1, m] booleans; None = every output is evaluated
    @property
    def X_evaluation_mask(self) -> Optional[Tensor]:
        return self._mask_tensor

    @X_evaluation_mask.setter
    def X_evaluation_mask(self, mask: Optional[Tensor]) -> None:
        if mask is None:
            bits = (1 << self._m) - 1
        else:
            mk = torch.as_tensor(mask)
            if mk.dim() != 2 or tuple(mk.shape) != (1, self._m):
                raise ValueError(
                    f"Expected X_evaluation_mask of shape `1 x {self._m}` (q = 1), but got {tuple(mk.shape)}.")
            flags = mk.detach().to("cpu").bool().reshape(-1).tolist()
            bits = sum(1 << i for i, f in enumerate(flags) if f)
            if bits == 0:
                raise ValueError("X_evaluation_mask must select at least one output.")
        self._mask_tensor = mask
        self._mask_bits = bits  # the plans are kept by mask: setting one back finds its plan again

    @property
    def cost(self) -> float:
        """The cost of evaluating the masked outputs (``InverseCostWeightedUtility`` over ``FixedCostModel``)."""
        if self._costs is None:
            return 1.0
        return sum(c for i, c in enumerate(self._costs) if (self._mask_bits >> i) & 1)

    def get_augmented_q_batch_size(self, q: int) -> int:
        """The rows of a one-shot point for q candidates: ``q + num_fantasies * num_pareto``."""
        return q + self.num_pseudo_points

    def extract_candidates(self, X_full: Tensor) -> Tensor:
        """``X_full[*batch, q + num_fantasies * num_pareto, d] -> [*batch, q, d]``: the candidate rows."""
        return X_full[..., : -self.num_pseudo_points, :]

    def set_X_pending(self, X_pending: Optional[Tensor] = None) -> None:
        if X_pending is not None:
            raise UnsupportedError(f"{type(self).__name__} does not account for X_pending yet.")
        self.X_pending = None

    def _check_rows(self, rows: int) -> None:
        if rows <= self.num_pseudo_points:
            raise ValueError(
                f"n_f*num_pareto ({self.num_pseudo_points}) must be less than the q-batch dimension of X ({rows})")
        if rows != 1 + self.num_pseudo_points:
            raise UnsupportedError(
                f"only q = 1 is supported: expected X of {1 + self.num_pseudo_points} rows "
                f"(1 + num_fantasies * num_pareto), got {rows}.")

    def _plan_args(self, rows: int):
        return (self._mask_bits, self.num_fantasies, self.num_pareto, self.base_samples, self._mask_bits,
                self._current, self.cost)

    def fantasy_means(self, X: Tensor) -> Tensor:
        """Diagnostics: the fantasised posterior means ``Y [B, num_fantasies, num_pareto, m]`` (untransformed
        space) the hypervolume stage read for the one-shot points ``X [B, 1 + Nf Np, d]``."""
        self._check_x(X)
        Xd = X.detach().reshape((-1,) + tuple(X.shape[-2:])).to(self._device, torch.double)
        return self._plan_for(Xd.shape[0], Xd.shape[1]).forward(Xd, means=True)[1]


class PosteriorMeanHypervolume(_HypervolumeBase):
    """The value function: the hypervolume (over ``ref_point``) of the posterior mean at the q points of
    ``X[*batch, q, d]``, q <= 32 (BoTorch's ``_get_hv_value_function(use_posterior_mean=True)``)."""

    def __init__(self, model, ref_point, device=None) -> None:
        super().__init__(model, ref_point, device)
        hypervolume_limits(self._m, 1, 1)

    def _check_rows(self, rows: int) -> None:
        if rows > _lib.DKG_HVKG_MAX_PARETO:
            raise UnsupportedError(f"q={rows} points > {_lib.DKG_HVKG_MAX_PARETO}")

    def _plan_args(self, rows: int):
        return (rows, 1, rows, None, 0, 0.0, 1.0)
