"""The Pareto front of a posterior mean, sampled on the device (``csrc/dkg_pareto.hip``).

The reference samples it with pygmo's NSGA-II at every BO iteration (``modules/pareto/sample.py:16-48``; "Record
metrics", ``bo_loop.py:294-332, 480-520``) and once for the test problem's true front (``main.py:174``).  pygmo is
not available and is not restated: the generations here run the published operators (Deb & Agrawal 1995; Deb et al.
2002) with pygmo's documented ``nsga2`` defaults in HIP kernels, every random number drawn on the host from a
``torch.Generator`` of the call's own and uploaded once.  No trajectory parity with pygmo is claimed; what differs is
listed in DESIGN.md 8c (the tournament draws with replacement, the draw layout is this library's).

* ``posterior_mean``                 ``dkg_posterior_mean``: the mean alone, O(P n) per output
* ``nondominated_rank``              ``dkg_pareto_rank`` (up to 16384 points)
* ``posterior_front_on_points``      the non-dominated points of the mean over a candidate set (a grid)
* ``pareto_variation``               ``dkg_pareto_variation``
* ``pareto_nsga2``                   ``dkg_pareto_nsga2``: the whole evolution in one call
* ``sample_points_on_pareto_front``  the reference's entry (numpy in the reference's shapes)
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._plan import hip_device
from ._plan import workspace as _workspace
from .errors import UnsupportedError
from .gp_state import current_stream_ptr, prepare_outputs
from .model import ModelListGPState, SingleTaskGPState

N_PARETO_POINTS = 100  # performance_after_scalarisation.py:14 under SMOKE_TEST (1000 otherwise)
N_GENERATIONS = 100  # pygmo.nsga2(gen=100), sample.py:41


class PreparedModel:
    """A model's device caches for ``dkg_posterior_mean`` (``prepare_outputs`` over an empty discretisation: the
    factorisation and alpha, no Q_D)."""

    def __init__(self, model, device=None):
        self.device = hip_device(device, "Pareto")
        if isinstance(model, SingleTaskGPState):
            model = ModelListGPState(model)
        self.model = model
        self.m, self.d = model.num_outputs, model.input_dim
        if self.m > _lib.MAX_OUTPUTS:
            raise UnsupportedError(f"{self.m} outputs > {_lib.MAX_OUTPUTS}")
        if self.d > _lib.MAX_DIM:
            raise UnsupportedError(f"input dimension {self.d} > {_lib.MAX_DIM}")
        with torch.cuda.device(self.device):
            self.outputs = prepare_outputs(model.models, torch.empty(0, self.d, dtype=torch.double, device=self.device))
        self.structs = (_lib.DkgOutput * self.m)(*[c.struct for c in self.outputs])

    def mean(self, X: torch.Tensor) -> torch.Tensor:
        """[P, d] (model inputs) -> [P, m] on the device."""
        X = torch.as_tensor(X, dtype=torch.double).detach().to(self.device).contiguous()
        if X.dim() != 2 or X.shape[1] != self.d:
            raise ValueError(f"X must be P x {self.d}")
        P = X.shape[0]
        out = torch.empty(P, self.m, dtype=torch.double, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().dkg_posterior_mean(self.structs, self.m, self.d, _lib.ptr(X), P, _lib.ptr(out),
                                                      current_stream_ptr(self.device)), "dkg_posterior_mean")
        return out


def _prepared(model, device) -> PreparedModel:
    return model if isinstance(model, PreparedModel) else PreparedModel(model, device)


def posterior_mean(model, X, device=None) -> torch.Tensor:
    """Posterior mean of every output at X [P, d] (the model's own inputs) -> [P, m] on the device:
    ``y_mean + y_std (c + K(x, X) alpha)``, what ``BoTorchModel.batch_fitness`` (``sample.py:138-144``) and
    ``GPTestProblem.evaluate_true`` (``gp_testproblem.py:76-97``) read off ``model.posterior``.  ``model``: a
    ``ModelListGPState``, a ``SingleTaskGPState`` or a ``PreparedModel`` (to evaluate many batches on one
    factorisation).  A point's result does not depend on the batch it is evaluated in."""
    return _prepared(model, device).mean(X)


def nondominated_rank(F, keep: Optional[int] = None, device=None):
    """Non-dominated ranks, crowding distances and survivor order of the points F [Q, m] (all objectives maximised;
    ``dkg_pareto_rank``) -> (rank int32 [Q], crowding float64 [Q], order int32 [Q]) on the device.  Fronts are
    peeled until ``keep`` (default Q) points are ranked; the others get rank -1 and crowding 0, and ``order`` lists
    the ranked points by (rank, crowding descending, index), then -1.  Q <= 16384: the call brings the workspace
    ``dkg_pareto_rank_workspace`` asks for, so the library ranks Q <= 2048 points with whichever of its two paths
    its rule names and more points with the wide one; the results do not depend on the path."""
    dev = F.device if isinstance(F, torch.Tensor) and F.is_cuda and device is None else hip_device(device, "Pareto")
    F = torch.as_tensor(F, dtype=torch.double).detach().to(dev).contiguous()
    if F.dim() != 2:
        raise ValueError("F must be Q x m")
    Q, m = F.shape
    keep = Q if keep is None else int(keep)
    rank = torch.empty(Q, dtype=torch.int32, device=dev)
    crowd = torch.empty(Q, dtype=torch.double, device=dev)
    order = torch.empty(Q, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = int(lib.dkg_pareto_rank_workspace(Q, m))  # 0 outside the limits: the call below reports which
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.dkg_pareto_rank(_lib.ptr(F), Q, m, keep, _lib.ptr(rank), _lib.ptr(crowd), _lib.ptr(order),
                                       _lib.ptr(work) or None, nbytes, current_stream_ptr(dev)), "dkg_pareto_rank")
    return rank, crowd, order


def posterior_front_on_points(model, X, device=None) -> Tuple[np.ndarray, np.ndarray]:
    """The non-dominated points of the posterior mean over the candidate set X [P, d] (the model's own inputs,
    P <= 16384) -> (x [k, d], f [k, m]) numpy arrays in index order: ``dkg_posterior_mean`` at X, then
    ``dkg_pareto_rank`` with ``keep = 1``, and the rows of rank 0.  The deterministic front of a grid or of any
    candidate set: no random numbers, no generations.  ``model``: a ``ModelListGPState``, a ``SingleTaskGPState``
    or a ``PreparedModel``."""
    pm = _prepared(model, device)
    X = torch.as_tensor(X, dtype=torch.double).detach().to(pm.device).contiguous()
    f = pm.mean(X)
    if X.shape[0] == 0:
        return X.cpu().numpy(), f.cpu().numpy()
    rank, _, _ = nondominated_rank(f, keep=1)
    front = rank == 0
    return X[front].cpu().numpy(), f[front].cpu().numpy()


def pareto_draws(P: int, d: int) -> int:
    """Uniforms one variation of a population of P in d dimensions reads (``dkg_pareto_draws``)."""
    return int(_lib.load().dkg_pareto_draws(int(P), int(d)))


def _dev_vec(v, dev, d):
    t = torch.as_tensor(v, dtype=torch.double).detach().reshape(-1).to(dev).contiguous()
    if t.numel() != d:
        raise ValueError(f"bounds must have {d} entries")
    return t


def pareto_variation(X, rank, crowd, lb, ub, uniforms, cr=0.95, eta_c=10.0, m=0.01, eta_m=50.0) -> torch.Tensor:
    """P children [P, d] of the ranked device population (X, rank, crowd) from ``uniforms`` (device,
    ``pareto_draws(P, d)`` doubles in [0, 1); layout in include/dkg.h): binary tournament with replacement, bounded
    simulated binary crossover, bounded polynomial mutation (``dkg_pareto_variation``)."""
    dev = X.device
    X = X.detach().to(torch.double).contiguous()
    P, d = X.shape
    rank = rank.to(dev, torch.int32).contiguous()
    crowd = crowd.to(dev, torch.double).contiguous()
    lb, ub = _dev_vec(lb, dev, d), _dev_vec(ub, dev, d)
    uniforms = uniforms.to(dev, torch.double).contiguous()
    need = pareto_draws(P, d)
    if need and uniforms.numel() < need:
        raise ValueError(f"{uniforms.numel()} uniforms < {need}")
    out = torch.empty_like(X)
    prm = _lib.DkgNsga2Params(cr, eta_c, m, eta_m)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dkg_pareto_variation(_lib.ptr(X), _lib.ptr(rank), _lib.ptr(crowd), P, d, _lib.ptr(lb),
                                                    _lib.ptr(ub), prm, _lib.ptr(uniforms), _lib.ptr(out),
                                                    current_stream_ptr(dev)), "dkg_pareto_variation")
    return out


def pareto_nsga2(model, lb, ub, P: int, gens: int, uniforms, raw_inputs: bool = False, device=None, cr=0.95,
                 eta_c=10.0, m=0.01, eta_m=50.0):
    """The whole evolution on the device in one call (``dkg_pareto_nsga2``) -> (X [P, d], F [P, m], rank, crowd)
    device tensors.  ``uniforms``: ``P d + gens * pareto_draws(P, d)`` doubles in [0, 1).  ``raw_inputs``: the model
    takes the points as they are (a test problem) instead of normalised with the bounds (a surrogate)."""
    pm = _prepared(model, device)
    prm = _lib.DkgNsga2Params(cr, eta_c, m, eta_m, raw_inputs=1 if raw_inputs else 0)
    return _evolve("dkg_pareto_nsga2", (pm.structs, pm.m, pm.d), "dkg_pareto_workspace", pm.device, (), pm.d, pm.m,
                   lb, ub, P, gens, uniforms, prm)


def _evolve(entry: str, model_args: tuple, workspace: str, dev, lead: tuple, d: int, mo: int, lb, ub, P, gens,
            uniforms, prm):
    """One call of an evolution entry (``dkg_pareto_nsga2``: ``lead = ()``, one population and at least the
    uniforms it reads; ``dkg_pareto_nsga2_paths``: ``lead = (S,)``, uniforms of exactly ``[S, per sample]``) ->
    (X ``lead + [P, d]``, F ``lead + [P, m]``, rank, crowd ``lead + [P]``) device tensors.  ``model_args``: the
    entry's leading arguments; ``workspace``: the entry's workspace query, called with ``lead + (P, d, m)``."""
    lb, ub = _dev_vec(lb, dev, d), _dev_vec(ub, dev, d)
    uniforms = torch.as_tensor(uniforms, dtype=torch.double).to(dev).contiguous()
    P, gens = int(P), int(gens)
    lib = _lib.load()
    draws = int(lib.dkg_pareto_draws(P, d))  # 0 for a P the entry refuses: the call below reports it
    need = P * d + gens * draws
    if draws and lead and tuple(uniforms.shape) != lead + (need,):
        raise ValueError(f"uniforms of shape {tuple(uniforms.shape)}, expected {lead + (need,)}")
    if draws and not lead and uniforms.numel() < need:
        raise ValueError(f"{uniforms.numel()} uniforms < {need}")
    rows = lead + (max(P, 0),)
    X = torch.empty(*rows, d, dtype=torch.double, device=dev)
    F = torch.empty(*rows, mo, dtype=torch.double, device=dev)
    rank = torch.empty(*rows, dtype=torch.int32, device=dev)
    crowd = torch.empty(*rows, dtype=torch.double, device=dev)
    nbytes = int(getattr(lib, workspace)(*lead, P, d, mo))
    work = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*model_args, _lib.ptr(lb), _lib.ptr(ub), P, gens, prm, _lib.ptr(uniforms),
                                       _lib.ptr(X), _lib.ptr(F), _lib.ptr(rank), _lib.ptr(crowd), _lib.ptr(work),
                                       nbytes, current_stream_ptr(dev)), entry)
    return X, F, rank, crowd


def draw_uniforms(seed: Optional[int], n: int) -> torch.Tensor:
    """n uniforms in [0, 1) from a CPU generator of the call's own (seeded with ``seed``, or from the operating
    system's entropy when None); the global torch RNG is not touched."""
    g = torch.Generator()
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed))
    return torch.rand(n, dtype=torch.double, generator=g)


def sample_points_on_pareto_front(model_or_problem, bounds=None, npoints: int = N_PARETO_POINTS,
                                  gen: int = N_GENERATIONS, maximize: bool = True, seed: Optional[int] = None,
                                  device=None) -> Tuple[np.ndarray, np.ndarray]:
    """``sample.sample_points_on_pareto_front`` (``sample.py:16-48``): ``npoints`` points of the final NSGA-II
    population after ``gen`` generations, as numpy arrays (x [npoints, d], f [npoints, m]).

    ``model_or_problem``: a ``GPProblem`` (the reference's ``BoTorchProblem`` wrapper of the test problem,
    ``main.py:174``: its GP takes the points as they are; bounds default to the problem's) or a surrogate
    (``ModelListGPState`` / ``SingleTaskGPState`` / ``PreparedModel``) with ``bounds`` [2, d] (the reference's
    ``BoTorchModel``: inputs normalised with the bounds, ``sample.py:129-130``).  ``npoints``: a multiple of 4
    from 8 to 1024 (pygmo asks for a multiple of 4 too).  The uniforms come from a CPU ``torch.Generator`` made
    here, seeded with ``seed`` (None: operating-system entropy), and are uploaded once; the global torch RNG is
    never touched (pygmo seeds itself from its own global generator).  ``maximize=False`` is not supported (the
    reference never passes it)."""
    if not maximize:
        raise UnsupportedError("sample_points_on_pareto_front: only maximize=True is supported")
    raw = hasattr(model_or_problem, "gp") and hasattr(model_or_problem, "num_objectives")
    if raw:
        model = model_or_problem.gp
        bounds = model_or_problem.bounds if bounds is None else bounds
        device = model_or_problem.device if device is None else device
    else:
        model = model_or_problem
        if bounds is None:
            raise ValueError("a surrogate needs its bounds")
    pm = _prepared(model, device)
    bnd = torch.as_tensor(bounds, dtype=torch.double).reshape(2, pm.d)
    P, gens = int(npoints), int(gen)
    n = P * pm.d + max(gens, 0) * pareto_draws(P, pm.d)
    X, F, _, _ = pareto_nsga2(pm, bnd[0], bnd[1], P, gens, draw_uniforms(seed, n), raw_inputs=raw)
    return X.cpu().numpy(), F.cpu().numpy()
