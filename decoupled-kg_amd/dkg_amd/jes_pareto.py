"""The Pareto samples of joint entropy search, on the device (``csrc/dkg_rff.hip``, ``csrc/dkg_pareto.hip``).

The reference's ``modules/pareto/jes_sample_pareto.py``: per sample a posterior path of the model drawn with random
Fourier features (BoTorch's ``get_gp_samples``, ``:81-86``), pymoo's NSGA-II on the path (``:146-207``) and the
front pruned by repeated crowding distance (``:210-232``), one sample after the other.  Here the weight posteriors of
all samples are factorised in batches, and every generation of every sample runs in the same four launches.  Neither
BoTorch nor pymoo is restated; what differs is listed in DESIGN.md 8e.

* ``sample_rff_paths``                       ``dkg_rff_weights`` -> ``RffPaths`` (``__call__``: ``dkg_rff_eval``)
* ``pareto_nsga2_paths``                     ``dkg_pareto_nsga2_paths``
* ``pareto_prune`` / ``prune_pareto_front``  ``dkg_pareto_prune``
* ``run_nsga2_with_pruning``                 the evolution and the pruning of every sample
* ``sample_discrete_pareto_optimal_points``  the reference's entry

The draws.  Every random number comes from one CPU ``torch.Generator`` made by the call (seeded with ``seed``, or
from the operating system's entropy when None); the global torch RNG is never touched.  ``sample_rff_paths`` draws,
in this order, ``wn = randn(S, m, R, d)``, ``ub = rand(S, m, R)``, ``z = randn(S, m, R)`` and
``g = standard_gamma(nu_i) / nu_i`` of shape ``(S, m, R)`` (for an RBF output the shape parameter 1 is drawn and
not used); ``sample_discrete_pareto_optimal_points`` then draws the evolution's uniforms
``rand(S, P d + gens * pareto_draws(P, d))`` from the same generator.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._plan import hip_device, workspace
from .errors import UnsupportedError
from .gp_state import _base_struct, current_stream_ptr
from .model import ModelListGPState, SingleTaskGPState
from .pareto import _evolve, pareto_draws

# the reference's variation (jes_sample_pareto.py:200-201): SimulatedBinaryCrossover(prob=0.9, eta=15),
# PolynomialMutation(eta=20); the per-coordinate mutation probability is pymoo's default, min(0.5, 1 / d)
SBX_PROB, SBX_ETA, PM_ETA = 0.9, 15.0, 20.0


def _generator(seed: Optional[int]) -> torch.Generator:
    g = torch.Generator()
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed))
    return g


def _model_state(model) -> ModelListGPState:
    if isinstance(model, SingleTaskGPState):
        return ModelListGPState(model)
    if isinstance(model, ModelListGPState):
        return model
    from .discretekg import _as_model_state

    return _as_model_state(model)


def draw_rff_randomness(generator: torch.Generator, nus, S: int, R: int, d: int):
    """(wn [S, m, R, d], g [S, m, R], ub [S, m, R], z [S, m, R]) CPU tensors in the module's documented order;
    ``nus``: per output the Matern smoothness, None for RBF."""
    m = len(nus)
    dd = dict(dtype=torch.double, generator=generator)
    wn = torch.randn(S, m, R, d, **dd)
    ub = torch.rand(S, m, R, **dd)
    z = torch.randn(S, m, R, **dd)
    shape = torch.tensor([1.0 if nu is None else float(nu) for nu in nus], dtype=torch.double)
    conc = shape.reshape(1, m, 1).expand(S, m, R).contiguous()
    g = torch._standard_gamma(conc, generator=generator) / conc
    return wn, g, ub, z


class RffPaths:
    """S sample paths of an m-output model on the device (``struct dkg_rff_paths``): sample s, output i is
    ``offset[s, i] + sum_r coef[s, i, r] cos(omega[s, i, r] . x + bias[s, i, r])`` over model inputs x."""

    def __init__(self, omega: Tensor, bias: Tensor, coef: Tensor, offset: Tensor, jitter=None):
        self.omega, self.bias, self.coef, self.offset = omega, bias, coef, offset
        self.S, self.m, self.R, self.d = omega.shape
        self.device = omega.device
        self.jitter = jitter

    def struct(self, first: int = 0, count: Optional[int] = None) -> _lib.DkgRffPaths:
        """The paths ``first .. first + count`` as the library takes them (views: no copy)."""
        count = self.S - first if count is None else count
        if first < 0 or count < 1 or first + count > self.S:
            raise ValueError(f"samples {first}..{first + count} of {self.S}")
        return _lib.DkgRffPaths(count, self.m, self.d, self.R, _lib.ptr(self.omega[first]), _lib.ptr(self.bias[first]),
                                _lib.ptr(self.coef[first]), _lib.ptr(self.offset[first]))

    def sample(self, s: int) -> "RffPaths":
        """Sample s alone (views of this object's tensors)."""
        return RffPaths(self.omega[s:s + 1], self.bias[s:s + 1], self.coef[s:s + 1], self.offset[s:s + 1])

    def __call__(self, X) -> Tensor:
        """X [P, d] (every sample evaluates it) or [S, P, d] (model inputs) -> [S, P, m] on the device.  A point's
        value has the same bits whatever P, its row and the samples beside it."""
        X = torch.as_tensor(X, dtype=torch.double).detach().to(self.device).contiguous()
        shared = X.dim() == 2
        if X.shape[-1] != self.d or not (shared or (X.dim() == 3 and X.shape[0] == self.S)):
            raise ValueError(f"X must be P x {self.d} or {self.S} x P x {self.d}")
        P = X.shape[-2]
        out = torch.empty(self.S, P, self.m, dtype=torch.double, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().dkg_rff_eval(self.struct(), _lib.ptr(X), P, 1 if shared else 0, _lib.ptr(out),
                                                current_stream_ptr(self.device)), "dkg_rff_eval")
        return out


def rff_weights(model, wn, g, ub, z, device=None, max_tries: int = 3) -> RffPaths:
    """``dkg_rff_weights`` on the caller's draws (shapes of ``draw_rff_randomness``)."""
    state = _model_state(model)
    dev = hip_device(device, "Pareto")
    m, d = state.num_outputs, state.input_dim
    S, mm, R, dd = wn.shape
    if mm != m or dd != d:
        raise ValueError(f"draws of m={mm}, d={dd} for a model of m={m}, d={d}")
    if m > _lib.MAX_OUTPUTS:
        raise UnsupportedError(f"{m} outputs > {_lib.MAX_OUTPUTS}")
    if d > _lib.MAX_DIM:
        raise UnsupportedError(f"input dimension {d} > {_lib.MAX_DIM}")
    lib = _lib.load()
    up = lambda t: torch.as_tensor(t, dtype=torch.double).detach().to(dev).contiguous()  # noqa: E731
    wn, g, ub, z = up(wn), up(g), up(ub), up(z)
    keep, structs, ys = [], [], []
    for st in state.models:
        x, il, y = up(st.train_x), up(1.0 / st.lengthscale), up(st.train_y)
        keep += [x, il, y]
        structs.append(_base_struct(st, il, x))
        ys.append(_lib.ptr(y))
    n_max = max(st.num_train for st in state.models)
    omega = torch.empty(S, m, R, d, dtype=torch.double, device=dev)
    bias = torch.empty(S, m, R, dtype=torch.double, device=dev)
    coef = torch.empty(S, m, R, dtype=torch.double, device=dev)
    offset = torch.empty(S, m, dtype=torch.double, device=dev)
    paths = RffPaths(omega, bias, coef, offset)
    nbytes = int(lib.dkg_rff_workspace(R, n_max))  # 0 outside the limits: the call below reports which
    work = workspace(nbytes, dev)
    jit = (ctypes.c_double * (S * m))()
    outs = (_lib.DkgOutput * m)(*structs)
    with torch.cuda.device(dev):
        ps = _lib.DkgRffPaths(S, m, d, R, _lib.ptr(omega), _lib.ptr(bias), _lib.ptr(coef), _lib.ptr(offset))
        _lib.check(lib.dkg_rff_weights(outs, m, d, (ctypes.c_void_p * m)(*ys), _lib.ptr(wn), _lib.ptr(g), _lib.ptr(ub),
                                       _lib.ptr(z), int(max_tries), ps, _lib.ptr(work), nbytes, jit,
                                       current_stream_ptr(dev)), "dkg_rff_weights")
        torch.cuda.current_stream(dev).synchronize()  # the draws and the training data may go out of scope
    paths.jitter = torch.tensor(list(jit), dtype=torch.double).reshape(S, m)
    return paths


def sample_rff_paths(model, num_samples: int, num_rffs: int = 512, seed: Optional[int] = None, device=None,
                     generator: Optional[torch.Generator] = None) -> RffPaths:
    """``num_samples`` posterior paths of ``model`` with ``num_rffs`` random Fourier features each: what
    ``get_gp_samples(model, num_outputs, n_samples=1, num_rff_features)`` gives the reference, once per sample
    (``jes_sample_pareto.py:81-86``).  The weight posterior is ``dkg_rff_weights``' (include/dkg.h); the draws and
    their order are the module's (above).  ``generator`` (a CPU generator) replaces the one made from ``seed``."""
    state = _model_state(model)
    gen = _generator(seed) if generator is None else generator
    nus = [None if st.kernel == "rbf" else float(st.nu) for st in state.models]
    wn, g, ub, z = draw_rff_randomness(gen, nus, int(num_samples), int(num_rffs), state.input_dim)
    return rff_weights(state, wn, g, ub, z, device=device)


def pareto_nsga2_paths(paths: RffPaths, lb, ub, P: int, gens: int, uniforms, raw_inputs: bool = False,
                       cr=SBX_PROB, eta_c=SBX_ETA, m=None, eta_m=PM_ETA):
    """``dkg_pareto_nsga2_paths``: population s evolves on sample s -> (X [S, P, d], F [S, P, m], rank [S, P],
    crowd [S, P]) device tensors.  ``uniforms``: [S, P d + gens * pareto_draws(P, d)] doubles in [0, 1).  ``m``: the
    per-coordinate mutation probability (None: ``min(0.5, 1 / d)``)."""
    pm = min(0.5, 1.0 / paths.d) if m is None else float(m)
    prm = _lib.DkgNsga2Params(cr, eta_c, pm, eta_m, raw_inputs=1 if raw_inputs else 0)
    return _evolve("dkg_pareto_nsga2_paths", (paths.struct(),), "dkg_pareto_paths_workspace", paths.device,
                   (paths.S,), paths.d, paths.m, lb, ub, P, gens, uniforms, prm)


def pareto_prune(F, rank, k: int):
    """``dkg_pareto_prune``: F [S, Q, m] and rank [S, Q] (device) -> (count int32 [S], index int32 [S, k]): per
    sample the members of rank 0 without bit-equal duplicates, pruned to at most k by repeated crowding distance;
    their indices ascending, then -1."""
    dev = F.device
    F = F.detach().to(torch.double).contiguous()
    rank = rank.to(dev, torch.int32).contiguous()
    if F.dim() != 3 or tuple(rank.shape) != tuple(F.shape[:2]):
        raise ValueError("F must be S x Q x m and rank S x Q")
    S, Q, m = F.shape
    k = int(k)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    index = torch.empty(S, max(k, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dkg_pareto_prune(_lib.ptr(F), _lib.ptr(rank), S, Q, m, k, _lib.ptr(count),
                                                _lib.ptr(index), current_stream_ptr(dev)), "dkg_pareto_prune")
    return count, index


def prune_pareto_front(pareto_set, pareto_front, num_points: int, device=None):
    """``prune_pareto_front`` (``jes_sample_pareto.py:210-232``) of one set [Q, d] and front [Q, m] (arrays or
    tensors) -> the rows that stay, in index order, in the inputs' types.  Dominated and duplicated rows go first
    (the reference is given pymoo's non-dominated, duplicate-free result); ties of the crowding distance retire the
    lowest index where the reference draws at random."""
    from .pareto import nondominated_rank

    as_numpy = not isinstance(pareto_front, torch.Tensor)
    ps = torch.as_tensor(pareto_set, dtype=torch.double)
    pf = torch.as_tensor(pareto_front, dtype=torch.double)
    dev = pf.device if pf.is_cuda and device is None else hip_device(device, "Pareto")
    if pf.dim() != 2 or ps.dim() != 2 or ps.shape[0] != pf.shape[0]:
        raise ValueError("pareto_set must be Q x d and pareto_front Q x m")
    if pf.shape[0] == 0:
        return (ps.numpy(), pf.numpy()) if as_numpy else (ps, pf)
    Fd = pf.to(dev)
    rank, _, _ = nondominated_rank(Fd, keep=1)
    count, index = pareto_prune(Fd.unsqueeze(0), rank.unsqueeze(0), num_points)
    sel = index[0, :int(count[0])].long().to(ps.device)
    ps, pf = ps[sel], pf[sel.to(pf.device)]
    return (ps.cpu().numpy(), pf.cpu().numpy()) if as_numpy else (ps, pf)


def run_nsga2_with_pruning(paths: RffPaths, bounds, num_points: int, maximize: bool = True, *, pop_size: int,
                           generations: int, uniforms=None, seed: Optional[int] = None, mutation_prob=None,
                           generator: Optional[torch.Generator] = None) -> Tuple[List[Tensor], List[Tensor]]:
    """``run_nsga2_with_pruning`` (``jes_sample_pareto.py:101-143``) for every sample of ``paths`` at once: NSGA-II
    on each path over ``bounds`` [2, d] (the path takes the points normalised with them, as a surrogate does), then
    the non-dominated members of each final population pruned to ``num_points``.  -> two lists of S device tensors
    ``k_s x d`` (in the bounds' space) and ``k_s x m`` (the path's values), ``k_s <= num_points``.

    A generation here makes ``pop_size`` children where the reference's pymoo call makes 10 (``n_offsprings=10``),
    so ``generations`` generations evaluate ten times as many points; the reference's defaults are kept.
    ``pop_size``: a multiple of 4 from 8 to 1024."""
    if not maximize:
        raise UnsupportedError("run_nsga2_with_pruning: only maximize=True is supported")
    d = paths.d
    bnd = torch.as_tensor(bounds, dtype=torch.double).detach().cpu().reshape(2, d)
    P, gens = int(pop_size), int(generations)
    if uniforms is None:
        gen = _generator(seed) if generator is None else generator
        uniforms = torch.rand(paths.S, P * d + max(gens, 0) * pareto_draws(P, d), dtype=torch.double, generator=gen)
    X, F, rank, _ = pareto_nsga2_paths(paths, bnd[0], bnd[1], P, gens, uniforms, m=mutation_prob)
    count, index = pareto_prune(F, rank, num_points)
    count = count.cpu().tolist()
    sets, fronts = [], []
    for s in range(paths.S):
        sel = index[s, :count[s]].long()
        sets.append(X[s][sel])
        fronts.append(F[s][sel])
    return sets, fronts


def sample_discrete_pareto_optimal_points(model, bounds, num_samples: int, target_num_points: int, *,
                                          num_rffs: int = 512, nsga2_pop_size: int = 100,
                                          nsga2_generations: int = 500, maximize: bool = True,
                                          seed: Optional[int] = None, device=None,
                                          mutation_prob: Optional[float] = None
                                          ) -> Tuple[List[Tensor], List[Tensor]]:
    """``sample_discrete_pareto_optimal_points`` (``jes_sample_pareto.py:48-98``): ``num_samples`` Pareto sets
    (``k_s x d``, in the space of ``bounds`` [2, d]) and fronts (``k_s x m``, the sampled path's values,
    untransformed), ``k_s <= target_num_points``, as tensors of the bounds' dtype and device.  The model takes its
    inputs normalised with ``bounds`` (the reference passes the unit cube, under which nothing changes).  For one
    output every sample holds its one best point (``1 x d``, ``1 x 1``).  All draws come from one generator seeded
    with ``seed`` (module docstring).  ``maximize=False`` is not supported."""
    if not maximize:
        raise UnsupportedError("sample_discrete_pareto_optimal_points: only maximize=True is supported")
    bounds = torch.as_tensor(bounds)
    gen = _generator(seed)
    paths = sample_rff_paths(model, num_samples, num_rffs, device=device, generator=gen)
    sets, fronts = run_nsga2_with_pruning(paths, bounds, target_num_points, pop_size=nsga2_pop_size,
                                          generations=nsga2_generations, generator=gen, mutation_prob=mutation_prob)
    dt = bounds.dtype if bounds.dtype.is_floating_point else torch.double
    to = lambda t: t.to(device=bounds.device, dtype=dt)  # noqa: E731
    return [to(t) for t in sets], [to(t) for t in fronts]


__all__ = ["RffPaths", "sample_rff_paths", "rff_weights", "draw_rff_randomness", "pareto_nsga2_paths", "pareto_prune",
           "prune_pareto_front", "run_nsga2_with_pruning", "sample_discrete_pareto_optimal_points"]
