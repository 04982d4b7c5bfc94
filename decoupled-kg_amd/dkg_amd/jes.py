"""Lower-bound joint entropy search (JES-LB / LB2, Tu et al. 2022) on MI355X -- host mirror.

Same surface as the reference's ``decoupledbo.modules.acquisition.joint_entropy_search``
(``joint_entropy_search.py:291-526``) for the estimators the reference's presets run (``"LB"``, ``"LB2"``;
``bo_loop.py:142-159``), with its ``target_output_ix`` for the decoupled setting:

* ``qLowerBoundMultiObjectiveJointEntropySearch(model, pareto_sets, pareto_fronts, hypercell_bounds,
  X_pending=None, estimation_type="LB", num_samples=64, target_output_ix=None)`` with
  ``forward(X[*batch, 1, d]) -> [*batch]`` (differentiable) and ``value_and_grad_host``;
* ``compute_sample_box_decomposition(pareto_fronts)`` (``jes_sample_pareto.py:235-…``) for one and two
  objectives.

The model conditioned on each sampled Pareto set (``condition_on_observations`` with observation noise,
``:365-376``) is built once at construction as a fitted state of its own: the sample's rows appended to every
output's training data, hyperparameters, noise and Standardize statistics unchanged, factorised by the full
preparation (``gp_state.prepare_outputs``, the oracle's jitter policy), or with ``conditioning="append"`` from the
model's own caches by one batched block update (``gp_state.append_observations``).  Every evaluation is then two
HIP kernel launches through the C ABI (``include/dkg.h`` ``dkg_jes_*``).  There is no CPU fallback.
"""

from __future__ import annotations

from typing import List, Optional

import torch
from torch import Tensor

from . import _lib, _plan, gp_state
from .discretekg import _as_model_state, _Base, _HAVE_BOTORCH, t_batch_mode_transform
from .errors import UnsupportedError
from .gp_state import current_stream_ptr
from .model import ModelListGPState, SingleTaskGPState

NEG_INF = -1e10  # the reference point of the box decompositions (BoTorch's compute_sample_box_decomposition)
ESTIMATION_TYPES = ["0", "LB", "LB2", "MC"]
SUPPORTED_ESTIMATION_TYPES = ("LB", "LB2")
# how the conditioned states are built: the full preparation of every state (the default: the oracle's jitter policy
# and the bits every result has had), or one batched block update of state 0's caches (gp_state.append_observations)
CONDITIONING = ("refactorise", "append")


def _nondominated_sorted_2d(pf: Tensor) -> Tensor:
    """The non-dominated points of pf [k, 2] (both maximised), duplicates dropped, by the first objective."""
    pf = torch.unique(pf, dim=0)  # sorted by the first objective, then the second, ascending
    keep = []
    best = -float("inf")
    for r in range(pf.shape[0] - 1, -1, -1):  # from the largest first objective down
        if float(pf[r, 1]) > best:
            keep.append(r)
            best = float(pf[r, 1])
    return pf[sorted(keep)]


def compute_sample_box_decomposition(pareto_fronts: List[Tensor], maximize: bool = True) -> Tensor:
    """The box decomposition of the space dominated by each sampled Pareto front (``jes_sample_pareto.py:235``,
    BoTorch's function of the same name with ``DominatedPartitioning``), for one and two objectives, on the
    host: ``[P, 2, J, m]`` with ``[:, 0]`` the lower and ``[:, 1]`` the upper corners.

    * m = 1: the one box ``[-1e10, max]``.
    * m = 2: the staircase of the non-dominated points sorted by the first objective,
      ``(a_1, b_1), ..., (a_k, b_k)`` with a increasing and b decreasing: box j is
      ``[a_{j-1}, a_j] x [-1e10, b_j]`` (``a_0 = -1e10``).  Dominated and repeated points give no box.
    * Samples with fewer boxes are padded with zero-width boxes ``[0, 0]``, as the reference pads (:243-245).
    * ``maximize=False``: the fronts are negated, decomposed, and the boxes mirrored back.

    m >= 3 raises ``UnsupportedError``: ``dkg_amd.boxes.dominated_boxes`` builds the boxes of three objectives on
    the device (and these, bit for bit, for one and two), or pass your own bounds to the acquisition."""
    if len(pareto_fronts) == 0:
        raise ValueError("Expected at least one Pareto front.")
    if not all(pf.dim() == 2 for pf in pareto_fronts):
        raise ValueError("The Pareto fronts should have a shape of `num_pareto_points_i x num_objectives`.")
    m = pareto_fronts[0].shape[-1]
    if not all(pf.shape[-1] == m and pf.shape[0] >= 1 for pf in pareto_fronts):
        raise ValueError("Expected every Pareto front to hold at least one point of the same number of objectives.")
    if m > 2:
        raise UnsupportedError(
            f"compute_sample_box_decomposition builds the boxes of 1 or 2 objectives; got {m}. "
            "Pass the hypercell bounds of your own partitioning to the acquisition.")
    weight = 1.0 if maximize else -1.0
    per_sample = []
    for pf in pareto_fronts:
        y = weight * pf.detach().to("cpu", torch.double)
        if m == 1:
            lo = torch.full((1, 1), NEG_INF, dtype=torch.double)
            hi = y.max(dim=0, keepdim=True).values
        else:
            nd = _nondominated_sorted_2d(y)
            lo = torch.full_like(nd, NEG_INF)
            lo[1:, 0] = nd[:-1, 0]
            hi = nd.clone()
        per_sample.append((lo, hi))
    J = max(lo.shape[0] for lo, _ in per_sample)
    out = torch.zeros(len(per_sample), 2, J, m, dtype=torch.double)
    for p, (lo, hi) in enumerate(per_sample):
        k = lo.shape[0]
        if maximize:
            out[p, 0, :k], out[p, 1, :k] = lo, hi
        else:
            out[p, 0, :k], out[p, 1, :k] = -hi, -lo
    return out.to(pareto_fronts[0].dtype)


def conditioned_states(state: ModelListGPState, pareto_sets, pareto_fronts) -> List[ModelListGPState]:
    """Per Pareto sample p, the model conditioned on it (``joint_entropy_search.py:365-376``): output i with
    the rows ``(ps_p, (pf_p[:, i] - y_mean_i) / y_std_i)`` appended to its training data (``pareto_sets`` in the
    model's input space, ``pareto_fronts`` in the untransformed output space); the new rows carry the
    likelihood's noise, and hyperparameters, noise and Standardize statistics are the model's."""
    out = []
    for ps, pf in zip(pareto_sets, pareto_fronts):
        ps = ps.detach().to("cpu", torch.double)
        pf = pf.detach().to("cpu", torch.double)
        models = []
        for i, o in enumerate(state.models):
            y_new = (pf[:, i] - o.y_mean) / o.y_std
            models.append(SingleTaskGPState(torch.cat([o.train_x, ps]), torch.cat([o.train_y, y_new]), o.lengthscale,
                                            o.outputscale, o.noise, o.mean_constant, o.kernel, o.nu, o.y_mean,
                                            o.y_std))
        out.append(ModelListGPState(*models))
    return out


class JesPlan(_plan.Plan):
    """A ``dkg_jes_*`` plan (include/dkg.h): the (P + 1) m fitted states, the boxes, the estimator and the
    target, with the workspace for up to ``max_B`` candidates; the state table is uploaded once."""

    def __init__(self, structs, m: int, P: int, d: int, bounds: Tensor, target: int, only_diagonal: bool,
                 max_B: int, device):
        lib = _lib.load()
        self.m, self.P, self.d = m, P, d
        self.J = bounds.shape[2]
        self.bounds = bounds  # device [P, 2, J, m]; read at every evaluation
        super().__init__(device, lib.dkg_jes_plan_bytes(), lib.dkg_jes_workspace(m, P, d, self.J, int(max_B)), max_B)
        _lib.check(lib.dkg_jes_init(structs, m, P, d, _lib.ptr(bounds), self.J, target, int(bool(only_diagonal)),
                                    self.max_B, _lib.ptr(self.ws), self.ws.numel(), self.host,
                                    current_stream_ptr(device)), "dkg_jes_init")
        self._fwd = lib.dkg_jes_forward

    def forward(self, X: Tensor, grad: bool = False, moments: bool = False):
        """``X``: device fp64 ``[B, d]`` or ``[B, 1, d]``.  -> ``out`` (device, ``[B * (1 + d)]`` with the
        gradient, else ``[B]``: ``out[:B]`` the values, ``out[B:]`` dacq/dX row-major) and, with ``moments``, the
        exported moments ``[3, P + 1, m, B]``."""
        B = X.shape[0]
        mom = torch.empty(3, self.P + 1, self.m, B, dtype=torch.double, device=self.device) if moments else None
        out = self._forward(self._fwd, "dkg_jes_forward", X, self.d, grad, mom)
        return (out, mom) if moments else out


class qLowerBoundMultiObjectiveJointEntropySearch(_Base):
    """The lower-bound joint entropy search acquisition (``joint_entropy_search.py:291-526``), q = 1."""

    def __init__(self, model, pareto_sets: List[Tensor], pareto_fronts: List[Tensor], hypercell_bounds: Tensor,
                 X_pending: Optional[Tensor] = None, estimation_type: str = "LB", num_samples: int = 64,
                 target_output_ix: Optional[int] = None, device=None, conditioning: str = "refactorise",
                 **kwargs) -> None:
        if conditioning not in CONDITIONING:
            raise ValueError(f"conditioning must be one of {CONDITIONING}, got {conditioning!r}")
        if _HAVE_BOTORCH:  # pragma: no cover
            super().__init__(model=model)
        else:
            super().__init__()
            self.model = model
        state = _as_model_state(model)
        self.initial_model = model
        # the reference's checks and messages (:99-148)
        if len(pareto_sets) != len(pareto_fronts):
            raise ValueError(
                f"The number of Pareto fronts and Pareto sets should be equal! "
                f"Got {len(pareto_sets)=}, {len(pareto_fronts)=}")
        if not all(ps.ndim == 2 for ps in pareto_sets) or not all(pf.ndim == 2 for pf in pareto_fronts):
            raise ValueError(
                "The Pareto sets and fronts should have shapes of "
                "`num_pareto_points_i x input_dim` and "
                "`num_pareto_points_i x num_objectives`, respectively")
        if not all(ps.shape[0] == pf.shape[0] for ps, pf in zip(pareto_sets, pareto_fronts)):
            raise ValueError(
                "Expected each pair of Pareto set and Pareto front to have the same"
                "number of points.")
        self.pareto_sets = pareto_sets
        self.pareto_fronts = pareto_fronts
        if hypercell_bounds.ndim != 4:
            raise UnsupportedError(
                "The hypercell_bounds should have a shape of "
                "`num_pareto_samples x 2 x num_boxes x num_objectives`.")
        self.hypercell_bounds = hypercell_bounds
        self.num_pareto_samples = hypercell_bounds.shape[0]
        self.target_output_ix = target_output_ix
        self.estimation_type = estimation_type
        self.num_samples = num_samples  # the Monte Carlo estimate's ("MC"); unused by "LB" / "LB2"
        if estimation_type not in ESTIMATION_TYPES:
            raise NotImplementedError(
                "Currently the only supported estimation type are: "
                + ", ".join(f'"{h}"' for h in ESTIMATION_TYPES) + ".")
        if self.target_output_ix is not None and estimation_type not in {"LB", "LB2"}:
            raise UnsupportedError(
                f"Currently only estimation types 'LB' and 'LB2' are supported when "
                f"supplying a . Got {estimation_type!r}.")
        if estimation_type not in SUPPORTED_ESTIMATION_TYPES:
            raise UnsupportedError(
                f"estimation_type {estimation_type!r} is not built on the device; supported: "
                + ", ".join(f'"{h}"' for h in SUPPORTED_ESTIMATION_TYPES) + ".")
        self.set_X_pending(X_pending)
        # beyond the reference's checks: shapes it would fail on later, while broadcasting
        m, d = state.num_outputs, state.input_dim
        P = len(pareto_sets)
        if P < 1:
            raise ValueError("Expected at least one Pareto sample.")
        if hypercell_bounds.shape[0] != P or hypercell_bounds.shape[1] != 2 or hypercell_bounds.shape[3] != m:
            raise ValueError(
                f"Expected hypercell_bounds of shape {P} x 2 x num_boxes x {m}. Got {tuple(hypercell_bounds.shape)}.")
        if not all(ps.shape[1] == d for ps in pareto_sets) or not all(pf.shape[1] == m for pf in pareto_fronts):
            raise ValueError(f"Expected Pareto sets of {d} columns and Pareto fronts of {m} columns.")
        # target_output_ix as discretekg.py reads it: negatives from the end, IndexError at evaluation
        self._target = None
        self._target_error = None
        if target_output_ix is not None:
            t = int(target_output_ix)
            if -m <= t < m:
                self._target = t % m
            else:
                self._target_error = IndexError("list index out of range")
        dev = _plan.hip_device(device, "joint entropy search")
        if m > _lib.MAX_OUTPUTS:
            raise UnsupportedError(f"{m} outputs > {_lib.MAX_OUTPUTS}")
        if d > _lib.MAX_DIM:
            raise UnsupportedError(f"input dimension {d} > {_lib.MAX_DIM}")
        if P > _lib.DKG_JES_MAX_SAMPLES:
            raise UnsupportedError(f"{P} Pareto samples > {_lib.DKG_JES_MAX_SAMPLES}")
        self._device = dev
        self._m, self._d, self._P = m, d, P
        # state 0 the model, state p + 1 the model conditioned on sample p: the full preparation over an empty
        # discretisation, one call per state
        states = [state] + conditioned_states(state, pareto_sets, pareto_fronts)
        empty = torch.empty(0, d, dtype=torch.double, device=dev)
        self.conditioning = conditioning
        self.append_fallbacks = 0  # "append": the conditioned outputs that took the full preparation instead
        with torch.cuda.device(dev):
            if conditioning == "refactorise":
                self._caches = [gp_state.prepare_outputs(s.models, empty) for s in states]
            else:
                self._caches = self._append_caches(states, empty)
        self._structs = (_lib.DkgOutput * ((P + 1) * m))(*[c.struct for cs in self._caches for c in cs])
        self._bounds = hypercell_bounds.detach().to(dev, torch.double).contiguous()
        self._plan = None

    def _append_caches(self, states: List[ModelListGPState], empty: Tensor):
        """``conditioning="append"``: state 0 by the full preparation, the conditioned states from its caches by
        one batched block update over the P m (sample, output) jobs (``gp_state.append_observations``).  A job
        whose base output was factorised with jitter, or whose update is not positive definite, takes the full
        preparation instead (the oracle's jitter policy), and is counted in ``append_fallbacks``."""
        base = gp_state.prepare_outputs(states[0].models, empty)
        m = len(base)
        # (a sample of more than DKG_APPEND_MAX_ROWS points is beyond the block update: the full preparation too)
        jobs = [(p, i) for p in range(1, len(states)) for i in range(m) if base[i].jitter == 0.0
                and 1 <= states[p].models[i].num_train - base[i].train_x.shape[0] <= _lib.DKG_APPEND_MAX_ROWS]
        new = gp_state.append_observations(
            [base[i] for _, i in jobs], empty,
            [states[p].models[i].train_x[base[i].train_x.shape[0]:] for p, i in jobs],
            [states[p].models[i].train_y for p, i in jobs], check=False)
        done = {job: cache for job, cache in zip(jobs, new) if cache is not None}
        caches = [base]
        for p in range(1, len(states)):
            row = []
            for i in range(m):
                if (p, i) not in done:
                    self.append_fallbacks += 1
                    done[(p, i)] = gp_state.prepare_output(states[p].models[i], empty)
                row.append(done[(p, i)])
            caches.append(row)
        return caches

    def set_X_pending(self, X_pending: Optional[Tensor] = None) -> None:
        if X_pending is not None:
            raise UnsupportedError(f"{type(self).__name__} does not account for X_pending yet.")
        self.X_pending = None

    def _plan_for(self, B: int, rows: int = 1) -> JesPlan:
        """The plan, grown (powers of two, at least 16) to hold B candidates (of ``rows`` = 1 point each)."""
        if self._target_error is not None:
            raise self._target_error
        if self._plan is None or self._plan.max_B < B:
            with torch.cuda.device(self._device):
                self._plan = JesPlan(self._structs, self._m, self._P, self._d, self._bounds,
                                     -1 if self._target is None else self._target, self.estimation_type == "LB2",
                                     _plan.grow(B), self._device)
        return self._plan

    def _check_d(self, X: Tensor) -> None:
        if X.shape[-1] != self._d:
            raise RuntimeError(f"Expected X to have last dimension {self._d} (the model's inputs). Got {X.shape[-1]=}.")

    @t_batch_mode_transform(expected_q=1)
    def forward(self, X: Tensor) -> Tensor:
        self._check_d(X)
        if X.device.type == "cpu":
            return _plan.HostForwardFn.apply(X, self)
        batch = X.shape[:-2]
        Xd = X.reshape(-1, 1, self._d).to(self._device, torch.double)
        return _plan.ForwardFn.apply(Xd, self).to(device=X.device, dtype=X.dtype).reshape(batch)

    def _host_x(self, X: Tensor):
        self._check_d(X)
        if X.dim() > 2 and X.shape[-2] != 1:
            raise ValueError(f"Expected X to be `batch_shape x q=1 x d`, but got X with shape {tuple(X.shape)}.")
        xs = X.detach().to("cpu", torch.double).reshape(-1, self._d)
        batch = X.shape[:-2] if X.dim() > 2 else X.shape[:-1]
        return xs, batch

    def _values_host(self, X: Tensor) -> Tensor:
        xs, batch = self._host_x(X)
        out = self._plan_for(xs.shape[0]).forward(xs.to(self._device))
        return out.cpu().reshape(batch)

    def value_and_grad_host(self, X: Tensor):
        """acq and dacq/dX for host candidates X (``[*batch, 1, d]`` or ``[B, d]``) as host fp64 tensors of
        shapes ``batch`` and ``X.shape``: what one L-BFGS-B evaluation of ``optimize_acqf`` needs back, in one
        device round trip (one copy in, the two launches, one copy of [acq | dacq/dX] out) and no autograd
        graph.  The same bits as ``forward`` + autograd."""
        xs, batch = self._host_x(X)
        B = xs.shape[0]
        out = self._plan_for(B).forward(xs.to(self._device), grad=True).cpu()
        return out[:B].reshape(batch), out[B:].reshape(X.shape)

    def moments(self, X: Tensor):
        """Diagnostics: ``(acq [B], mu, v, tau [P + 1, m, B])`` for candidates X ``[B, d]``, the moments the
        entropy stage read (``dkg_jes_forward``'s ``moments_out``: untransformed space; state 0's ``v`` holds
        ``var + noise``)."""
        self._check_d(X)
        Xd = X.detach().reshape(-1, self._d).to(self._device, torch.double)
        out, mom = self._plan_for(Xd.shape[0]).forward(Xd, moments=True)
        return out, mom[0], mom[1], mom[2]
