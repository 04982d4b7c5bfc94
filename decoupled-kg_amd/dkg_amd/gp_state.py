"""Device-resident GP state for the Discrete-KG kernels.

Builds, per output, the caches GPyTorch's exact prediction keeps behind
``model.posterior`` (``discretekg.py:182-185, 275-284``) — the ones BoTorch's
``fast_pred_var`` posterior uses:

* ``K = s k(X, X) + noise I``, ``L = psd_safe_cholesky(K)`` (linear_operator's
  jitter policy: absolute 1e-8 * 10**i, 3 retries), ``R = L^{-T}``
  (root_inv_decomposition) and ``alpha = K^{-1}(y - c)``:
                                              HIP ``dkg_prepare_output`` (blocked
                                              Cholesky / triangular inverse kernels)
* ``root_frag`` = R in MFMA fragment order    HIP ``dkg_pack_root``
* ``Q_D = K(D, X) R``, ``mu_D = c + K(D,X) alpha`` over the discretisation
                                              HIP ``dkg_cross_root``

All of it runs once per (model, discretisation) — the reference rebuilds the
same caches once per BO iteration — and stays in HBM for every forward call.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List

import torch

from . import _lib
from .errors import UnsupportedError
from .model import ModelListGPState, SingleTaskGPState, kernel_id


def _pad16(x: int) -> int:
    return (x + 15) // 16 * 16


def current_stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def _raw_stream(device) -> int:
    """current_stream_ptr without building a Stream object (the B = 1 host path: ~0.3 instead of ~3 us)."""
    idx = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


@dataclass
class OutputCache:
    """Device tensors of one output; ``struct`` points into them."""

    state: SingleTaskGPState
    inv_ls: torch.Tensor
    train_x: torch.Tensor
    alpha: torch.Tensor
    root_frag: torch.Tensor
    disc_frag: torch.Tensor
    disc_mean: torch.Tensor
    L: torch.Tensor
    jitter: float = 0.0  # absolute jitter psd_safe_cholesky needed (0: none)
    struct: _lib.DkgOutput = field(repr=False, default=None)
    Linv: torch.Tensor = field(repr=False, default=None)  # L^{-1}, row-major n x n (append_observation reads it)


def _base_struct(st: SingleTaskGPState, inv_ls, train_x) -> _lib.DkgOutput:
    o = _lib.DkgOutput()
    o.n = st.num_train
    o.kernel = kernel_id(st.kernel, st.nu)
    o.outputscale = float(st.outputscale)
    o.noise = float(st.noise)
    o.mean_constant = float(st.mean_constant)
    o.y_mean = float(st.y_mean)
    o.y_std = float(st.y_std)
    o.inv_lengthscale = _lib.ptr(inv_ls)
    o.train_x = _lib.ptr(train_x)
    return o


def prepare_outputs(models, D: torch.Tensor) -> List[OutputCache]:
    """Every output's device caches over the discretisation ``D`` (device, N x d): the factorisations of
    all outputs side by side (dkg_prepare_outputs: one chain of launches, one status check), then each
    output's Q_D and mu_D (dkg_cross_root)."""
    lib = _lib.load()
    dev = D.device
    stream = current_stream_ptr(dev)
    N = D.shape[0]
    parts = []
    # every output's training inputs, inverse lengthscales and targets in one host-to-device copy (a copy
    # from pageable memory costs ~3 us each; a model of m outputs had 3 m of them)
    host = []
    for st in models:
        n, d = st.train_x.shape
        if _pad16(n) > 1024:
            raise UnsupportedError(f"n={n} training points > 1024 per output is not supported")
        host += [st.train_x.detach().to(torch.double).reshape(-1), (1.0 / st.lengthscale).detach().to(torch.double)
                 .reshape(-1), st.train_y.detach().to(torch.double).reshape(-1)]
    flat = torch.cat([t.cpu() for t in host]).to(dev) if host else None
    views, off = [], 0
    for t in host:
        views.append(flat[off:off + t.numel()])
        off += t.numel()
    for k, st in enumerate(models):
        n, d = st.train_x.shape
        X = views[3 * k].view(n, d)
        inv_ls = views[3 * k + 1]
        o = _base_struct(st, inv_ls, X)
        y = views[3 * k + 2]
        L = torch.empty(n, n, dtype=torch.double, device=dev)
        work = torch.empty(lib.dkg_prepare_workspace(n), dtype=torch.uint8, device=dev)
        alpha = torch.empty(_pad16(n), dtype=torch.double, device=dev)
        root_frag = torch.empty(lib.dkg_frag_elems(n, n), dtype=torch.double, device=dev)
        parts.append((st, o, X, inv_ls, y, L, work, alpha, root_frag))
    m = len(parts)
    d = D.shape[1]
    outs = (_lib.DkgOutput * m)(*[p[1] for p in parts])
    ptrs = lambda k: (ctypes.c_void_p * m)(*[_lib.ptr(p[k]) for p in parts])  # noqa: E731
    jit = (ctypes.c_double * m)()
    wbytes = (ctypes.c_size_t * m)(*[p[6].numel() for p in parts])
    _lib.check(lib.dkg_prepare_outputs(outs, m, d, ptrs(4), 3, ptrs(5), ptrs(6), wbytes, ptrs(7), ptrs(8), jit, stream),
               "dkg_prepare_outputs")
    caches = []
    for i, (st, o, X, inv_ls, y, L, work, alpha, root_frag) in enumerate(parts):
        o.alpha = _lib.ptr(alpha)
        o.root_frag = _lib.ptr(root_frag)
        disc_frag = torch.empty(max(1, lib.dkg_frag_elems(N, o.n)), dtype=torch.double, device=dev)
        disc_mean = torch.empty(max(16, _pad16(N)), dtype=torch.double, device=dev)
        if N > 0:
            _lib.check(lib.dkg_cross_root(o, d, _lib.ptr(D), N, _lib.ptr(disc_frag), _lib.ptr(disc_mean), stream),
                       "dkg_cross_root")
        o.disc_frag = _lib.ptr(disc_frag)
        o.disc_mean = _lib.ptr(disc_mean)
        n = o.n
        linv = work[: n * n * 8].view(torch.double).view(n, n)  # the head of the preparation's scratch
        caches.append(OutputCache(st, inv_ls, X, alpha, root_frag, disc_frag, disc_mean, L, jit[i], o, linv))
    return caches


def append_observation(cache: OutputCache, D: torch.Tensor, x, train_y) -> OutputCache:
    """The caches of ``([X; x], train_y)`` from those of ``(X, y)`` by the bordered Cholesky update
    (``dkg_append_observation``): no refactorisation, one pass over ``L^{-1}`` and one over ``disc_frag``.
    ``D`` is the device discretisation the cache was built over, ``x`` the new point (d values),
    ``train_y`` the n + 1 targets of the grown output (model space).  Out of place: ``cache`` and its
    tensors are left as they are.  Raises ``NotPSDError`` when the grown covariance is not positive
    definite under the old jitter (rebuild instead: the full preparation applies the jitter policy) and
    ``UnsupportedError`` beyond 1024 training points."""
    lib = _lib.load()
    st = cache.state
    dev = D.device
    n, d = cache.train_x.shape
    N = D.shape[0]
    if _pad16(n + 1) > 1024:
        raise UnsupportedError(f"n={n + 1} training points > 1024 per output is not supported")
    xh = torch.as_tensor(x, dtype=torch.double).detach().cpu().reshape(1, d)
    yh = torch.as_tensor(train_y, dtype=torch.double).detach().cpu().reshape(-1)
    if yh.numel() != n + 1:
        raise ValueError(f"train_y has {yh.numel()} entries for {n + 1} training points")
    new_st = SingleTaskGPState(torch.cat([st.train_x, xh]), yh.clone(), st.lengthscale, st.outputscale, st.noise,
                               st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)
    flat = torch.cat([xh.reshape(-1), yh]).to(dev)  # the new point and the targets in one host-to-device copy
    X = torch.cat([cache.train_x, flat[:d].view(1, d)])
    y = flat[d:]
    n1 = n + 1
    L = torch.empty(n1, n1, dtype=torch.double, device=dev)
    linv = torch.empty(n1, n1, dtype=torch.double, device=dev)
    alpha = torch.empty(_pad16(n1), dtype=torch.double, device=dev)
    root_frag = torch.empty(lib.dkg_frag_elems(n1, n1), dtype=torch.double, device=dev)
    disc_frag = torch.empty(max(1, lib.dkg_frag_elems(N, n1)), dtype=torch.double, device=dev)
    disc_mean = torch.empty(max(16, _pad16(N)), dtype=torch.double, device=dev)
    work = torch.empty(lib.dkg_append_workspace(n, N), dtype=torch.uint8, device=dev)
    _lib.check(lib.dkg_append_observation(cache.struct, d, _lib.ptr(cache.L), _lib.ptr(cache.Linv), _lib.ptr(D), N,
                                          _lib.ptr(X), _lib.ptr(y), float(cache.jitter), _lib.ptr(L), _lib.ptr(linv),
                                          _lib.ptr(alpha), _lib.ptr(root_frag), _lib.ptr(disc_frag),
                                          _lib.ptr(disc_mean), _lib.ptr(work), work.numel(),
                                          current_stream_ptr(dev)), "dkg_append_observation")
    o = _base_struct(new_st, cache.inv_ls, X)
    o.alpha = _lib.ptr(alpha)
    o.root_frag = _lib.ptr(root_frag)
    o.disc_frag = _lib.ptr(disc_frag)
    o.disc_mean = _lib.ptr(disc_mean)
    return OutputCache(new_st, cache.inv_ls, X, alpha, root_frag, disc_frag, disc_mean, L, cache.jitter, o, linv)


def append_observations(caches, D: torch.Tensor, X_new, train_y, check: bool = True):
    """A block of rows appended to each of several fitted outputs in one batched update (``dkg_append_rows``):
    job ``j`` turns ``caches[j]``, the caches of ``(X, y)``, into those of ``([X; X_new[j]], train_y[j])`` --
    exact-GP conditioning on ``K_j = X_new[j].shape[0]`` new rows, no refactorisation.  ``caches``, ``X_new``
    (``[K_j, d]`` each, ``1 <= K_j <= 32``) and ``train_y`` (all ``n_j + K_j`` targets each, model space) are
    sequences of equal length; the same cache may appear in several jobs.  ``D`` is the device discretisation
    every cache was built over, or an empty ``[0, d]`` tensor.  One host-to-device copy carries all new rows
    and targets, one C call runs all jobs, and ``alpha`` is formed from all targets of a job (the old ones
    may change).  Out of place.  Returns the new ``OutputCache`` list.

    Raises ``NotPSDError`` naming the jobs whose grown covariance is not positive definite under the old
    jitter (``.jobs``: their indices; ``.caches``: the list with ``None`` at those jobs), and
    ``UnsupportedError`` beyond 32 rows, 512 jobs or 1024 training points.  ``check=False`` returns the list
    with ``None`` at the failed jobs instead of raising."""
    from .errors import NotPSDError

    lib = _lib.load()
    caches, X_new, train_y = list(caches), list(X_new), list(train_y)
    J = len(caches)
    if not (J == len(X_new) == len(train_y)):
        raise ValueError(f"{J} caches, {len(X_new)} row blocks and {len(train_y)} target vectors")
    if J == 0:
        return []
    if J > _lib.DKG_APPEND_MAX_JOBS:
        raise UnsupportedError(f"{J} jobs > {_lib.DKG_APPEND_MAX_JOBS} per call is not supported")
    dev = D.device
    N, d = D.shape
    host, shapes = [], []
    for j, (c, x, y) in enumerate(zip(caches, X_new, train_y)):
        n = c.train_x.shape[0]
        xh = torch.as_tensor(x, dtype=torch.double).detach().cpu().reshape(-1, d)
        yh = torch.as_tensor(y, dtype=torch.double).detach().cpu().reshape(-1)
        K = xh.shape[0]
        if K < 1:
            raise ValueError(f"job {j}: no new rows")
        if K > _lib.DKG_APPEND_MAX_ROWS:
            raise UnsupportedError(f"job {j}: K={K} new rows > {_lib.DKG_APPEND_MAX_ROWS} per call is not supported")
        if _pad16(n + K) > 1024:
            raise UnsupportedError(f"job {j}: n={n + K} training points > 1024 per output is not supported")
        if yh.numel() != n + K:
            raise ValueError(f"job {j}: train_y has {yh.numel()} entries for {n + K} training points")
        host += [xh.reshape(-1), yh]
        shapes.append((n, K, xh, yh))
    flat = torch.cat(host).to(dev)  # every job's new rows and targets in one host-to-device copy
    jobs = (_lib.DkgAppendJob * J)()
    parts, off = [], 0
    for j, (c, (n, K, xh, yh)) in enumerate(zip(caches, shapes)):
        X = torch.cat([c.train_x, flat[off:off + K * d].view(K, d)])
        y = flat[off + K * d:off + K * d + n + K]
        off += K * d + n + K
        n1 = n + K
        L = torch.empty(n1, n1, dtype=torch.double, device=dev)
        linv = torch.empty(n1, n1, dtype=torch.double, device=dev)
        alpha = torch.empty(_pad16(n1), dtype=torch.double, device=dev)
        root_frag = torch.empty(lib.dkg_frag_elems(n1, n1), dtype=torch.double, device=dev)
        disc_frag = torch.empty(max(1, lib.dkg_frag_elems(N, n1)), dtype=torch.double, device=dev)
        disc_mean = torch.empty(max(16, _pad16(N)), dtype=torch.double, device=dev)
        parts.append((X, y, L, linv, alpha, root_frag, disc_frag, disc_mean))
        b = jobs[j]
        b.o = ctypes.pointer(c.struct)
        b.L, b.Linv, b.disc, b.N, b.K = _lib.ptr(c.L), _lib.ptr(c.Linv), _lib.ptr(D) if N else None, N, K
        b.train_x, b.train_y, b.jitter = _lib.ptr(X), _lib.ptr(y), float(c.jitter)
        b.L_new, b.Linv_new, b.alpha_new, b.root_frag_new = (_lib.ptr(L), _lib.ptr(linv), _lib.ptr(alpha),
                                                             _lib.ptr(root_frag))
        b.disc_frag_new, b.disc_mean_new = _lib.ptr(disc_frag), _lib.ptr(disc_mean)
    work = torch.empty(lib.dkg_append_rows_workspace(jobs, J, d), dtype=torch.uint8, device=dev)
    info = (ctypes.c_int32 * J)()
    status = lib.dkg_append_rows(jobs, J, d, info, _lib.ptr(work), work.numel(), current_stream_ptr(dev))
    if status != _lib.DKG_ERR_NOT_PD:
        _lib.check(status, "dkg_append_rows")
    out = []
    for j, (c, (n, K, xh, yh)) in enumerate(zip(caches, shapes)):
        if info[j] != 0:
            out.append(None)
            continue
        st = c.state
        X, y, L, linv, alpha, root_frag, disc_frag, disc_mean = parts[j]
        new_st = SingleTaskGPState(torch.cat([st.train_x, xh]), yh.clone(), st.lengthscale, st.outputscale, st.noise,
                                   st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)
        o = _base_struct(new_st, c.inv_ls, X)
        o.alpha = _lib.ptr(alpha)
        o.root_frag = _lib.ptr(root_frag)
        o.disc_frag = _lib.ptr(disc_frag)
        o.disc_mean = _lib.ptr(disc_mean)
        out.append(OutputCache(new_st, c.inv_ls, X, alpha, root_frag, disc_frag, disc_mean, L, c.jitter, o, linv))
    failed = [j for j in range(J) if info[j] != 0]
    if failed and check:
        err = NotPSDError(f"dkg_append_rows: covariance not positive definite with the appended rows in jobs {failed} "
                          f"of {J} (pivots {[int(info[j]) for j in failed]}); rebuild those with prepare_outputs")
        err.jobs, err.caches = failed, out
        raise err
    return out


# The opt-in incremental path of discretekg.shared_state (off by default: nothing that exists changes bits)
# and the counters of how the shared device states were made.
_INCREMENTAL = False
_STATS = {"full_builds": 0, "appends": 0, "append_fallbacks": 0}


def set_incremental_state(on: bool) -> bool:
    """With the switch on, a model that extends a cached one (same discretisation and hyperparameters, rows
    added to some outputs) gets its device state by appending the added rows to the cached state
    (``DeviceGPState.with_observation``) instead of a full rebuild.  Returns the previous setting."""
    global _INCREMENTAL
    prev = _INCREMENTAL
    _INCREMENTAL = bool(on)
    return prev


def incremental_state() -> bool:
    return _INCREMENTAL


_GRADIENT_ROWS = "staged"
GRADIENT_ROWS_MODES = ("staged", "auto", "global")


def check_gradient_rows(mode) -> str:
    if mode not in GRADIENT_ROWS_MODES:
        raise ValueError(f"gradient rows mode must be one of {GRADIENT_ROWS_MODES}, got {mode!r}")
    return mode


def set_gradient_rows(mode: str) -> str:
    """Where the gradient plans of ``DiscreteKnowledgeGradient`` (``forward`` with autograd,
    ``value_and_grad_host``, ``forward_targets``, ``value_and_grad_host_targets``, and with them
    ``optimize_acqf``, ``run_mobo`` and ``run_smoke``) take the candidates' Q_X and J rows from, for every
    acquisition built without ``gradient_rows``: ``"staged"`` (the default: LDS, ``UnsupportedError`` where
    they do not fit), ``"auto"`` (the same plans, and global rows where ``"staged"`` refuses) or ``"global"``
    (global rows always; a test hook).  See ``ForwardPlan``.  Returns the previous mode."""
    global _GRADIENT_ROWS
    prev = _GRADIENT_ROWS
    _GRADIENT_ROWS = check_gradient_rows(mode)
    return prev


def gradient_rows() -> str:
    return _GRADIENT_ROWS


def state_stats() -> dict:
    """How the shared device states were made since the last reset: ``full_builds`` (a whole
    ``DeviceGPState``), ``appends`` (rows appended) and ``append_fallbacks`` (an append that was not positive
    definite, answered by a full build)."""
    return dict(_STATS)


def reset_state_stats() -> None:
    for k in _STATS:
        _STATS[k] = 0


def _same_hyperparameters(a: SingleTaskGPState, b: SingleTaskGPState) -> bool:
    return (a.kernel == b.kernel and (a.kernel == "rbf" or float(a.nu) == float(b.nu))
            and float(a.outputscale) == float(b.outputscale) and float(a.noise) == float(b.noise)
            and float(a.mean_constant) == float(b.mean_constant) and float(a.y_mean) == float(b.y_mean)
            and float(a.y_std) == float(b.y_std) and a.lengthscale.shape == b.lengthscale.shape
            and torch.equal(a.lengthscale, b.lengthscale))


def match_extension(old: ModelListGPState, new: ModelListGPState):
    """Whether ``new`` extends ``old``: per output the number of rows added (0: equal data), or ``None`` when
    it does not.  An output extends its old self when it has equal data, or the same hyperparameters, kernel,
    nu, ``y_mean`` and ``y_std``, the old rows of ``train_x`` equal by value, and k >= 1 rows added (its
    targets may all be new).  Pure host code."""
    if old.num_outputs != new.num_outputs or old.input_dim != new.input_dim:
        return None
    added = []
    for a, b in zip(old.models, new.models):
        n = a.num_train
        k = b.num_train - n
        if k < 0 or not _same_hyperparameters(a, b) or not torch.equal(a.train_x, b.train_x[:n]):
            return None
        if k == 0 and not torch.equal(a.train_y, b.train_y):
            return None
        added.append(k)
    return added


def prepare_output(st: SingleTaskGPState, D: torch.Tensor) -> OutputCache:
    """One output's device caches (prepare_outputs of one)."""
    return prepare_outputs([st], D)[0]


class DeviceGPState:
    """All outputs' caches over one discretisation, plus a reusable workspace."""

    def __init__(self, model: ModelListGPState, x_discretisation: torch.Tensor, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise UnsupportedError("the Discrete-KG kernels run on a ROCm (HIP) device; got " + str(self.device))
        if model.num_outputs > _lib.MAX_OUTPUTS:
            raise UnsupportedError(f"{model.num_outputs} outputs > {_lib.MAX_OUTPUTS}")
        if model.input_dim > _lib.MAX_DIM:
            raise UnsupportedError(f"input dimension {model.input_dim} > {_lib.MAX_DIM}")
        self.model = model
        self.D = x_discretisation.detach().to(self.device, torch.double).contiguous()
        self.N, self.d = self.D.shape
        self.outputs: List[OutputCache] = prepare_outputs(model.models, self.D)
        self.m = len(self.outputs)
        self.structs = (_lib.DkgOutput * self.m)(*[c.struct for c in self.outputs])
        self._ws = None
        self._ws_key = None

    def with_observation(self, output_ix: int, x, y=None, train_y=None) -> "DeviceGPState":
        """A new state with ``x`` appended to output ``output_ix``: that output's caches by the bordered
        update (``append_observation``), the other outputs' ``OutputCache`` objects shared, not copied.
        Give the new target ``y`` (appended to the output's targets) or the n + 1 targets ``train_y``.  This
        state, and every plan or captured graph on it, stays valid.  Raises ``NotPSDError`` /
        ``UnsupportedError`` as ``append_observation``."""
        if not 0 <= int(output_ix) < self.m:
            raise IndexError(f"output index {output_ix} out of range for {self.m} outputs")
        if (y is None) == (train_y is None):
            raise ValueError("give exactly one of y (the new target) and train_y (all n + 1 targets)")
        i = int(output_ix)
        old = self.outputs[i]
        if train_y is None:
            train_y = torch.cat([old.state.train_y, torch.as_tensor(y, dtype=torch.double).detach().cpu().reshape(1)])
        with torch.cuda.device(self.device):
            new = append_observation(old, self.D, x, train_y)
        return self._with_output(i, new)

    def with_observations(self, output_ix: int, X, y=None, train_y=None) -> "DeviceGPState":
        """``with_observation`` for a block of rows ``X`` (``[K, d]``, ``1 <= K <= 32``) in one batched update
        (``append_observations``).  Give the K new targets ``y`` (appended to the output's targets) or all
        n + K targets ``train_y``.  Raises ``NotPSDError`` / ``UnsupportedError`` as ``append_observations``."""
        if not 0 <= int(output_ix) < self.m:
            raise IndexError(f"output index {output_ix} out of range for {self.m} outputs")
        if (y is None) == (train_y is None):
            raise ValueError("give exactly one of y (the K new targets) and train_y (all n + K targets)")
        i = int(output_ix)
        old = self.outputs[i]
        if train_y is None:
            train_y = torch.cat([old.state.train_y, torch.as_tensor(y, dtype=torch.double).detach().cpu().reshape(-1)])
        with torch.cuda.device(self.device):
            (new,) = append_observations([old], self.D, [X], [train_y])
        return self._with_output(i, new)

    def _with_output(self, i: int, new: OutputCache) -> "DeviceGPState":
        """A state that shares every output's caches with this one but output ``i``'s."""
        st = object.__new__(DeviceGPState)
        st.device = self.device
        st.D, st.N, st.d, st.m = self.D, self.N, self.d, self.m
        st.outputs = list(self.outputs)
        st.outputs[i] = new
        st.model = ModelListGPState(*[c.state for c in st.outputs])
        st.structs = (_lib.DkgOutput * st.m)(*[c.struct for c in st.outputs])
        st._ws = None
        st._ws_key = None
        return st

    def plan(self, W: torch.Tensor, target, max_B: int, grad: bool = False, force_walk: bool = False,
             f32: bool = False, fused: bool = False, no_chain: bool = False, targets=None,
             grad_rows: str = "staged") -> "ForwardPlan":
        return ForwardPlan(self, W, target, max_B, grad, force_walk, f32, fused, no_chain, targets=targets,
                           grad_rows=grad_rows)

    def forward(self, X: torch.Tensor, W: torch.Tensor, target, kg_pairs=None, timed: bool = False):
        """One-shot forward (builds a plan on the fly); see ForwardPlan for the fast path."""
        p = ForwardPlan(self, W, target, max(1, X.shape[0]))
        return p.forward(X, kg_pairs=kg_pairs, timed=timed)


F32_CROSS_KERNELS = ("cross_root_plan_kernel<DM, float>", "cross_big32_kernel")
F32_COV_KERNELS = ("posterior_cov_kernel<DM, float>", "posterior_cov_big32_kernel<DM>")


def f32_dispatch(max_n_pad: int, d: int, N: int, m: int, B: int, geom_B: int = 0) -> dict:
    """Which fp32 kernels the cross and covariance stages of an fp32 plan launch for a shape, by the launcher's
    own predicates (dkg_debug_f32_dispatch; host only): ``cross`` / ``cov`` are "narrow" or "big32" (``*_kernel``
    the kernel's name), ``DM`` the dimension bucket, ``nbx`` / ``nby`` the covariance launch's line and candidate
    blocks and ``order`` the 64 x 64 blocks' order (-1: the narrow kernel's 32 x 32 blocks have none)."""
    out = (ctypes.c_int * 6)()
    if _lib.load().dkg_debug_f32_dispatch(int(max_n_pad), int(d), int(N), int(m), int(B), int(geom_B), out) != 0:
        _lib.check(_lib.DKG_ERR_ARG, "dkg_debug_f32_dispatch")
    names = ("narrow", "big32")
    return {"cross": names[out[0]], "cov": names[out[1]], "cross_kernel": F32_CROSS_KERNELS[out[0]],
            "cov_kernel": F32_COV_KERNELS[out[1]], "DM": out[2], "nbx": out[3], "nby": out[4], "order": out[5]}


# ForwardPlan(grad_rows=...): the plan flag of each mode
GRAD_ROWS_FLAGS = {"staged": 0, "auto": _lib.DKG_PLAN_GRAD_GLOBAL_ROWS, "global": _lib.DKG_PLAN_FORCE_GLOBAL_ROWS}


class ForwardPlan:
    """A DKG plan (include/dkg.h "Plan API"): weights, target and workspace for
    up to ``max_B`` candidates, device copy written once; ``forward`` is one
    C call that launches the forward on the current stream: the three stage
    kernels, or with ``fused=True`` one launch whose stages hand off inside it
    (dkg_fused.h; same bits, not faster on MI355X: DESIGN.md 4.8).  With ``grad=True`` the
    workspace also holds the gradient buffers and ``forward_grad`` returns
    dKG/dx alongside KG.

    ``targets`` (a sequence of ``None`` / output indices, distinct; ``target`` is then ignored): a plan of
    T targets (``dkg_plan_init_targets``).  Every call runs the cross and covariance stages once and the
    envelope once per (target, candidate), and ``forward`` / ``forward_into`` / ``forward_grad`` /
    ``forward_grad_host`` / ``forward_host`` / ``forward_stats`` return tensors with a leading T axis, row
    tau bit for bit what a single-target plan of ``targets[tau]`` returns.  Not with ``fused`` or
    ``forward_batches_into`` (``UnsupportedError``); ``lines`` exports the lines of ``targets[0]``.

    ``grad_rows`` (gradient plans; ignored without ``grad``): where the envelope takes the candidates' Q_X and J
    rows from.  ``"staged"``: LDS, and ``UnsupportedError`` for a model whose rows do not fit there.
    ``"auto"`` (``DKG_PLAN_GRAD_GLOBAL_ROWS``): the same plan wherever ``"staged"`` builds one, and where it
    refuses for the rows a streaming plan that reads them from the workspace.  ``"global"``
    (``DKG_PLAN_FORCE_GLOBAL_ROWS``, a test hook): that streaming plan on any shape.  ``grad_rows_global``
    tells which the plan runs."""

    def __init__(self, state: DeviceGPState, W: torch.Tensor, target, max_B: int, grad: bool = False,
                 force_walk: bool = False, f32: bool = False, fused: bool = False, no_chain: bool = False,
                 targets=None, grad_rows: str = "staged"):
        if grad_rows not in GRAD_ROWS_FLAGS:
            raise ValueError(f"grad_rows must be one of {GRADIENT_ROWS_MODES}, got {grad_rows!r}")
        self.grad_rows = grad_rows
        lib = _lib.load()
        self.state = state
        self.device = state.device
        # a snapshot: the plan's intercept cache and top hints (Plan::icpt / itop, built at init) are derived from
        # these weights, so a caller editing its own weights tensor in place must not reach the plan's copy
        self.W = W.detach().to(self.device, torch.double, copy=True).contiguous()
        if self.W.dim() != 2 or self.W.shape[1] != state.m:
            raise ValueError(f"weights must be S x {state.m}")
        self.S = self.W.shape[0]
        self.targets = None  # a plan of several targets: their C values (-1: all outputs), else None
        if targets is not None:
            tl = []
            for t in targets:
                if t is not None and not (0 <= int(t) < state.m):
                    raise ValueError(f"targets must be None (all outputs) or in [0, {state.m}), got {t}")
                tl.append(-1 if t is None else int(t))
            if not tl:
                raise ValueError("targets is empty")
            if len(set(tl)) != len(tl):
                raise ValueError(f"targets repeats an entry: {list(targets)}")
            self.targets = tuple(tl)
            target = None if tl[0] < 0 else tl[0]
        self._nt = 1 if self.targets is None else len(self.targets)
        if target is not None and not (0 <= int(target) < state.m):
            # the C ABI's -1 means "all outputs observed": a negative index never reaches it
            raise ValueError(f"target must be None (all outputs) or in [0, {state.m}), got {target}")
        self.target = -1 if target is None else int(target)
        self.max_B = int(max_B)
        self.grad = bool(grad)
        self.f32 = bool(f32)
        flags = ((_lib.DKG_PLAN_GRAD if self.grad else 0) | (_lib.DKG_PLAN_FORCE_WALK if force_walk else 0)
                 | (_lib.DKG_PLAN_F32 if self.f32 else 0) | (_lib.DKG_PLAN_FUSED if fused else 0)
                 | (_lib.DKG_PLAN_NO_CHAIN if no_chain else 0) | (GRAD_ROWS_FLAGS[grad_rows] if self.grad else 0))
        nbytes = lib.dkg_plan_bytes()
        self.host = ctypes.create_string_buffer(nbytes)
        if self.targets is not None:
            T = self._nt
            tl = (ctypes.c_int * T)(*self.targets)
            need = lib.dkg_plan_workspace_targets(state.structs, state.m, state.d, state.N, self.max_B, self.S, T,
                                                  flags)
            self.ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=self.device)
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.dkg_plan_init_targets(state.structs, state.m, state.d, _lib.ptr(state.D), state.N,
                                                 _lib.ptr(self.W), self.S, tl, T, self.max_B, flags,
                                                 _lib.ptr(self.ws), self.ws.numel(), self.host, _lib.ptr(self.dev),
                                                 current_stream_ptr(self.device)), "dkg_plan_init_targets")
        else:
            need = lib.dkg_plan_workspace(state.structs, state.m, state.d, state.N, self.max_B, self.S, flags)
            self.ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=self.device)
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.dkg_plan_init(state.structs, state.m, state.d, _lib.ptr(state.D), state.N,
                                         _lib.ptr(self.W), self.S, self.target, self.max_B, flags, _lib.ptr(self.ws),
                                         self.ws.numel(), self.host, _lib.ptr(self.dev),
                                         current_stream_ptr(self.device)), "dkg_plan_init")
        self.fused = bool(lib.dkg_plan_fused(self.host))  # forward_into is one fused launch
        self.grad_rows_global = bool(lib.dkg_plan_grad_rows_of(self.host))  # the envelope reads global rows
        self._fwd = lib.dkg_plan_forward
        self._fwd_batches = lib.dkg_plan_forward_batches
        self._fwd_timed = lib.dkg_plan_forward_timed
        self._fwd_grad_hostx = lib.dkg_plan_forward_grad_hostx
        self._dev_ptr = _lib.ptr(self.dev)

    def _lead(self, *shape):
        """The shape of a result: with a leading T axis on a plan of several targets."""
        return shape if self.targets is None else (self._nt,) + shape

    def envelope_geometry(self) -> dict:
        """Which envelope kernel the plan launches (dkg_debug_plan_envelope; host only): ``slots`` (register
        slots per lane of the staged envelope, 2 / 8 / 17 / 33; 0 when streaming), ``stream`` (1: the lines are
        streamed from global memory), ``sw`` (waves per workgroup) and ``split`` (workgroups per candidate)."""
        out = (ctypes.c_int * 4)()
        if _lib.load().dkg_debug_plan_envelope(self.host, out) != 0:
            _lib.check(_lib.DKG_ERR_ARG, "dkg_debug_plan_envelope")
        return {"slots": out[0], "stream": out[1], "sw": out[2], "split": out[3]}

    def qx32(self, output: int, B: int) -> torch.Tensor:
        """The fp32 ``Q_X = K(x, X) R`` of ``output`` as the last ``lines`` / forward of ``B`` candidates left it
        (dkg_debug_plan_qx32; fp32 plans only): host float32 [pad16(B), n_pad], padding included."""
        out = torch.empty(_pad16(B), _pad16(self.state.outputs[output].struct.n), dtype=torch.float32)
        _lib.check(_lib.load().dkg_debug_plan_qx32(self.host, int(output), int(B), out.data_ptr(),
                                                   current_stream_ptr(self.device)), "dkg_debug_plan_qx32")
        return out

    def f32_dispatch(self, B: int, geom_B: int = 0) -> dict:
        """Which fp32 kernels a launch of ``B`` candidates of this plan's shape takes (``f32_dispatch``)."""
        return f32_dispatch(max(_pad16(c.struct.n) for c in self.state.outputs), self.state.d, self.state.N,
                            self.state.m, B, geom_B)

    def status(self, reset: bool = False) -> int:
        """The bits of the fused launches' in-launch waits that gave up since the last reset (0: every hand-off
        matched; dkg_plan_status); synchronises the plan's stream."""
        err = ctypes.c_int(0)
        _lib.check(_lib.load().dkg_plan_status(self.host, ctypes.byref(err), int(reset),
                                               current_stream_ptr(self.device)), "dkg_plan_status")
        return err.value

    def _check_handoffs(self) -> None:
        """A fused launch whose bounded in-launch waits gave up computed on unready data: raise on the call
        that produced it (and reset the bits, so the next call starts clean)."""
        bits = self.status(reset=True)
        if bits:
            raise RuntimeError(f"fused Discrete-KG forward: in-launch hand-off wait gave up (bits 0x{bits:x}); "
                               "the result is invalid")

    def forward_into(self, X: torch.Tensor, kg: torch.Tensor, kg_pairs=None) -> None:
        """Hot path: X (device, B x d, contiguous fp64) -> kg (device, B; [T, B] on a plan of T targets, with
        kg_pairs [T, B, S])."""
        st = self._fwd(self.host, self._dev_ptr, X.data_ptr(), X.shape[0], kg.data_ptr(),
                       0 if kg_pairs is None else kg_pairs.data_ptr(),
                       torch.cuda.current_stream(self.device).cuda_stream)
        if st:
            _lib.check(st, "dkg_plan_forward")

    def forward_batches_into(self, X: torch.Tensor, kg: torch.Tensor, B: int) -> None:
        """K = X.shape[0] // B forward batches of B candidates in one launch per stage
        (``dkg_plan_forward_batches``): X (device, K*B x d, contiguous fp64, batch k = rows kB .. kB+B-1)
        -> kg (device, K*B).  Bit-for-bit the results of K ``forward_into`` calls, one per batch."""
        n = X.shape[0]
        if B < 1 or n % B:
            raise ValueError(f"{n} candidates are not whole batches of {B}")
        st = self._fwd_batches(self.host, self._dev_ptr, X.data_ptr(), B, n // B, kg.data_ptr(),
                               torch.cuda.current_stream(self.device).cuda_stream)
        if st:
            _lib.check(st, "dkg_plan_forward_batches")

    def forward_stats(self, X: torch.Tensor):
        """One forward with diagnostics: KG [B], KG per (candidate, scalarisation) [B, S] and the number
        of upper-envelope lines per pair [B, S] (int32; 1 = short-circuit), all on the device."""
        X = X.detach().to(self.device, torch.double).contiguous()
        B = X.shape[0]
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        kg = torch.empty(self._lead(B), dtype=torch.double, device=self.device)
        pairs = torch.empty(self._lead(B, self.S), dtype=torch.double, device=self.device)
        hull = torch.empty(self._lead(B, self.S), dtype=torch.int32, device=self.device)
        self.forward_into(X, kg, pairs)
        _lib.check(_lib.load().dkg_plan_hull_sizes(self.host, _lib.ptr(hull), B, current_stream_ptr(self.device)),
                   "dkg_plan_hull_sizes")
        if self.fused:
            self._check_handoffs()
        return kg, pairs, hull

    def lines(self, X: torch.Tensor):
        """The lines the envelope stage builds for candidates X (B x d), bit for bit:
        (intercepts, slopes), each [B, S, N + 1] on the device (line 0 = the candidate; dkg_plan_lines)."""
        X = X.detach().to(self.device, torch.double).contiguous()
        B = X.shape[0]
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        a = torch.empty(B, self.S, self.state.N + 1, dtype=torch.double, device=self.device)
        b = torch.empty_like(a)
        _lib.check(_lib.load().dkg_plan_lines(self.host, self._dev_ptr, _lib.ptr(X), B, _lib.ptr(a), _lib.ptr(b),
                                              current_stream_ptr(self.device)), "dkg_plan_lines")
        return a, b

    def forward_grad(self, X: torch.Tensor):
        """KG[B] and dKG/dx [B, d] for candidates X (B x d): one C call."""
        if not self.grad:
            raise ValueError("plan was built without grad=True")
        X = X.detach().to(self.device, torch.double).contiguous()
        B = X.shape[0]
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        kg = torch.empty(self._lead(B), dtype=torch.double, device=self.device)
        dkg = torch.empty(self._lead(B, self.state.d), dtype=torch.double, device=self.device)
        _lib.check(_lib.load().dkg_plan_forward_grad(self.host, self._dev_ptr, _lib.ptr(X), B, _lib.ptr(kg),
                                                     _lib.ptr(dkg), current_stream_ptr(self.device)),
                   "dkg_plan_forward_grad")
        return kg, dkg

    def forward_grad_host(self, X_host: torch.Tensor, graph: bool = False):
        """KG[B] and dKG/dx [B, d] for host candidates X (B x d), returned as host tensors: the L-BFGS-B
        evaluation of ``optimize_acqf`` (``bo_loop.py:127-129``), whose host needs both back every call.

        B x d <= DKG_XARG_MAX (the default path): one C call (``dkg_plan_forward_grad_hostx``) -- the
        candidates travel in the first kernel's arguments, the envelope kernel writes [KG | dKG/dx] into a
        plan-owned pinned buffer, the call returns after the stream has finished -- then one host copy
        out.  Larger batches, or ``graph``: one pinned H2D copy of X, the launches of
        ``dkg_plan_forward_grad`` (eager, or a HIP graph captured once per batch size; measured slower than
        eager launches at B = 1), one pinned D2H copy and one event wait.  Everything is
        ordered on the current stream of the plan's device; the results are the same bits as
        ``forward_grad``."""
        if not self.grad:
            raise ValueError("plan was built without grad=True")
        B, d = X_host.shape[0], self.state.d
        if X_host.dim() != 2 or X_host.shape[1] != d:
            raise ValueError(f"X must be B x {d}")
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        if B == 0:
            return (torch.empty(self._lead(0), dtype=torch.double),
                    torch.empty(self._lead(0, d), dtype=torch.double))
        if not graph and B * d <= _lib.DKG_XARG_MAX and torch.cuda.current_device() == self.device.index:
            return self._forward_grad_hostx(X_host, B, d)
        with torch.cuda.device(self.device):
            if not graph and B * d <= _lib.DKG_XARG_MAX:
                return self._forward_grad_hostx(X_host, B, d)
            return self._forward_grad_host(X_host, B, d, graph)

    def forward_grad_host_shaped(self, X_host: torch.Tensor, B: int, kshape, xshape):
        """``forward_grad_host`` for a contiguous fp64 host tensor holding B candidates in any shape (e.g. the
        ``[*batch, 1, d]`` X of ``optimize_acqf``), the results viewed as ``kshape`` / ``xshape``: the
        B = 1 L-BFGS-B path, with no reshape of X and the results copied out once through numpy (a torch
        slice or view costs about a microsecond of host time each, on a call whose device chain is ~30 us)."""
        d = self.state.d
        if (self.targets is None and self.grad and 0 < B <= self.max_B and B * d <= _lib.DKG_XARG_MAX
                and torch.cuda.current_device() == self.device.index):
            r = self._forward_grad_hostx_raw(X_host, B, d)
            return torch.from_numpy(r[:B].reshape(kshape)), torch.from_numpy(r[B:].reshape(xshape))
        kg, dkg = self.forward_grad_host(X_host.reshape(B, d))
        return kg.reshape(self._lead(*kshape)), dkg.reshape(self._lead(*xshape))

    def _forward_grad_hostx(self, X_host: torch.Tensor, B: int, d: int):
        r = self._forward_grad_hostx_raw(X_host, B, d)
        n = self._nt * B
        return torch.from_numpy(r[:n].reshape(self._lead(B))), torch.from_numpy(r[n:].reshape(self._lead(B, d)))

    def _forward_grad_hostx_raw(self, X_host: torch.Tensor, B: int, d: int):
        # the plan's device is current; one C call launches, lets the envelope kernel write the pinned
        # buffer and synchronises the stream; returns a numpy copy of [KG | dKG/dx]
        io = self._io.get(B) if getattr(self, "_io", None) is not None else None
        if io is None:
            self._host_buffers(d)
            dx = self._dx[:B * d]
            n = self._nt * B  # [kg (T x B) | dKG/dx (T x B x d)]
            out = self._hout[:n * (d + 1)]
            io = self._io[B] = (dx.data_ptr(), self._dout[:n].data_ptr(), self._dout[n:n * (d + 1)].data_ptr(),
                                out.data_ptr(), out.numpy())
        xc = X_host
        if xc.dtype != torch.double or not xc.is_contiguous():
            xc = xc.to(torch.double).contiguous()
        st = self._fwd_grad_hostx(self.host, self._dev_ptr, xc.data_ptr(), io[0], B, io[1], io[2], io[3],
                                  _raw_stream(self.device))
        if st:
            _lib.check(st, "dkg_plan_forward_grad_hostx")
        return io[4].copy()

    def _host_buffers(self, d: int):
        """The pinned host and device staging buffers of the host entries (made once, sized for max_B)."""
        if getattr(self, "_hx", None) is None:
            self._hx = torch.empty(self.max_B * d, dtype=torch.double).pin_memory()
            self._hout = torch.empty(self._nt * self.max_B * (d + 1), dtype=torch.double).pin_memory()
            self._dx = torch.empty(self.max_B * d, dtype=torch.double, device=self.device)
            self._dout = torch.empty(self._nt * self.max_B * (d + 1), dtype=torch.double, device=self.device)
            self._done = torch.cuda.Event()
            self._graphs = {}
            self._io = {}

    def _forward_grad_host(self, X_host: torch.Tensor, B: int, d: int, graph: bool):
        # runs with the plan's device current: the copies, the launches and the event share its stream
        stream = torch.cuda.current_stream(self.device)
        self._host_buffers(d)
        dx = self._dx[:B * d].view(B, d)
        n = self._nt * B
        kg, dkg = self._dout[:n], self._dout[n:n * (d + 1)].view(n, d)
        lib = _lib.load()

        def launch(stream):
            _lib.check(lib.dkg_plan_forward_grad(self.host, self._dev_ptr, _lib.ptr(dx), B, _lib.ptr(kg),
                                                 _lib.ptr(dkg), stream), "dkg_plan_forward_grad")

        hx = self._hx[:B * d].view(B, d)
        hx.copy_(X_host.detach().reshape(B, d))
        dx.copy_(hx, non_blocking=True)
        if graph:
            g = self._graphs.get(B)
            if g is None:
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    launch(torch.cuda.current_stream(self.device).cuda_stream)
                self._graphs[B] = g
                torch.cuda.synchronize(self.device)
            g.replay()
        else:
            launch(stream.cuda_stream)
        out = self._hout[:n * (d + 1)]
        out.copy_(self._dout[:n * (d + 1)], non_blocking=True)
        self._done.record(stream)
        self._done.synchronize()
        return out[:n].clone().view(self._lead(B)), out[n:].clone().view(self._lead(B, d))

    def forward_host(self, X_host: torch.Tensor) -> torch.Tensor:
        """KG[B] for host candidates X (B x d) as a host tensor: one pinned H2D copy, the forward's launches
        and one pinned D2H copy on the plan device's current stream (``forward`` of a host X without grad)."""
        B, d = X_host.shape[0], self.state.d
        if X_host.dim() != 2 or X_host.shape[1] != d:
            raise ValueError(f"X must be B x {d}")
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        if B == 0:
            return torch.empty(self._lead(0), dtype=torch.double)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            self._host_buffers(d)
            hx = self._hx[:B * d].view(B, d)
            hx.copy_(X_host.detach().reshape(B, d))
            dx = self._dx[:B * d].view(B, d)
            dx.copy_(hx, non_blocking=True)
            kg = self._dout[:self._nt * B]
            st = self._fwd(self.host, self._dev_ptr, dx.data_ptr(), B, kg.data_ptr(), 0, stream.cuda_stream)
            if st:
                _lib.check(st, "dkg_plan_forward")
            out = self._hout[:self._nt * B]
            out.copy_(kg, non_blocking=True)
            self._done.record(stream)
            self._done.synchronize()
            if self.fused:
                self._check_handoffs()
            return out.clone().view(self._lead(B))

    def time_stage(self, X: torch.Tensor, stage: int, reps: int) -> float:
        """Average duration (ms) of ``reps`` back-to-back launches of one kernel
        (0 cross_root, 1 posterior_cov, 2 envelope; 3 the whole forward as ``forward_into`` launches it),
        HIP events on the launch stream."""
        X = X.detach().to(self.device, torch.double).contiguous()
        kg = torch.empty(self._nt * X.shape[0], dtype=torch.double, device=self.device)
        ms = _lib.c_float()
        _lib.check(_lib.load().dkg_plan_time_stage(self.host, self._dev_ptr, _lib.ptr(X), X.shape[0], _lib.ptr(kg),
                                                   None, current_stream_ptr(self.device), stage, reps,
                                                   ctypes.byref(ms)), "dkg_plan_time_stage")
        return ms.value

    def time_stage_batches(self, X: torch.Tensor, B: int, stage: int, reps: int) -> float:
        """time_stage for the launches of ``forward_batches_into`` (X: K*B candidates, K batches of B)."""
        X = X.detach().to(self.device, torch.double).contiguous()
        if B < 1 or X.shape[0] % B:
            raise ValueError(f"{X.shape[0]} candidates are not whole batches of {B}")
        kg = torch.empty(X.shape[0], dtype=torch.double, device=self.device)
        ms = _lib.c_float()
        _lib.check(_lib.load().dkg_plan_time_stage_batches(self.host, self._dev_ptr, _lib.ptr(X), B, X.shape[0] // B,
                                                           _lib.ptr(kg), current_stream_ptr(self.device), stage,
                                                           reps, ctypes.byref(ms)), "dkg_plan_time_stage_batches")
        return ms.value

    def forward(self, X: torch.Tensor, kg_pairs=None, timed: bool = False):
        X = X.detach().to(self.device, torch.double).contiguous()
        B = X.shape[0]
        if B > self.max_B:
            raise ValueError(f"{B} candidates > plan capacity {self.max_B}")
        kg = torch.empty(self._lead(B), dtype=torch.double, device=self.device)
        if timed:
            ms = (_lib.c_float * 3)()
            _lib.check(self._fwd_timed(self.host, self._dev_ptr, _lib.ptr(X), B, _lib.ptr(kg), _lib.ptr(kg_pairs),
                                       current_stream_ptr(self.device), ms), "dkg_plan_forward_timed")
            return kg, list(ms)
        self.forward_into(X, kg, kg_pairs)
        return kg
