"""Dominated-space boxes and the hypervolume of large fronts on MI355X, one to three objectives -- host mirror.

* ``dominated_boxes(pareto_fronts, maximize=True, ref_point=None, device=None) -> [P, 2, J, m]``: the box
  decomposition of the space each front dominates, what BoTorch's ``compute_sample_box_decomposition`` gives the
  reference's JES through ``DominatedPartitioning`` (``jes_sample_pareto.py:235-347``).  At m <= 2 these are the
  boxes of ``jes.compute_sample_box_decomposition``, bit for bit; at m = 3 a front of K points gives at most
  2K - 1 boxes.
* ``hypervolume_front(points, ref_point, device=None)``: the exact dominated hypervolume of sets of up to 16384
  points, the number ``metrics.hypervolume`` computes on the host.

Both are one sweep (``include/dkg.h`` "Dominated-space boxes") through the C ABI's
``dkg_dominated_boxes`` and ``dkg_hypervolume_front``.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from ._plan import hip_device, workspace
from .gp_state import current_stream_ptr

NEG_INF = -1e10  # the reference point of the JES box decompositions (jes.NEG_INF)


def box_count_bound(K: int, m: int) -> int:
    """The most boxes K points of m objectives give (include/dkg.h): 1, K and 2K - 1 at m = 1, 2 and 3."""
    return 1 if m == 1 else (K if m == 2 else 2 * K - 1)


def _ref_array(ref: Sequence[float], m: int):
    return (ctypes.c_double * m)(*[float(v) for v in ref])


def dominated_boxes_device(Y: Tensor, ref_point: Sequence[float], J: Optional[int] = None):
    """``dkg_dominated_boxes`` on device sets ``Y [S, K, m]`` (fp64): ``bounds [S, 2, J, m]`` and ``count [S]``
    (int32), both on the device; J defaults to the count bound.  Rows that are not strictly above ``ref_point``
    give nothing."""
    lib = _lib.load()
    if Y.dim() != 3 or Y.dtype is not torch.double or Y.device.type != "cuda":
        raise ValueError("Expected a device fp64 tensor of shape `S x K x m`.")
    S, K, m = Y.shape
    Y = Y.contiguous()
    if J is None:
        J = box_count_bound(K, m)
    bounds = torch.empty(S, 2, max(J, 0), m, dtype=torch.double, device=Y.device)
    count = torch.empty(S, dtype=torch.int32, device=Y.device)
    work = workspace(lib.dkg_dominated_boxes_workspace(S, K, m), Y.device)
    with torch.cuda.device(Y.device):
        _lib.check(lib.dkg_dominated_boxes(_lib.ptr(Y), S, K, m, _ref_array(ref_point, m), int(J), _lib.ptr(bounds),
                                           _lib.ptr(count), _lib.ptr(work), work.numel(),
                                           current_stream_ptr(Y.device)), "dkg_dominated_boxes")
    return bounds, count


def dominated_boxes(pareto_fronts: List[Tensor], maximize: bool = True, ref_point=None, device=None) -> Tensor:
    """The box decomposition of the space dominated by each front of ``pareto_fronts`` (``[k_i, m]`` each, of
    unequal lengths, m <= 3) above ``ref_point`` (default -1e10 everywhere, as for JES): ``[P, 2, J, m]`` with
    ``[:, 0]`` the lower and ``[:, 1]`` the upper corners, J the largest number of boxes of a front, fronts with
    fewer padded with ``[0, 0]`` boxes, in the fronts' dtype and on their device.  Every corner is a copy of a
    front's value or of the reference point.  ``maximize=False``: the fronts (and ``ref_point``) are negated,
    decomposed, and the boxes mirrored back, as ``compute_sample_box_decomposition`` does."""
    if len(pareto_fronts) == 0:
        raise ValueError("Expected at least one Pareto front.")
    if not all(pf.dim() == 2 for pf in pareto_fronts):
        raise ValueError("The Pareto fronts should have a shape of `num_pareto_points_i x num_objectives`.")
    m = pareto_fronts[0].shape[-1]
    if not all(pf.shape[-1] == m and pf.shape[0] >= 1 for pf in pareto_fronts):
        raise ValueError("Expected every Pareto front to hold at least one point of the same number of objectives.")
    dev = hip_device(device, "box", *pareto_fronts)
    weight = 1.0 if maximize else -1.0
    if ref_point is None:
        ref = torch.full((m,), NEG_INF, dtype=torch.double)
    else:
        ref = weight * torch.as_tensor(ref_point).detach().to("cpu", torch.double).reshape(-1)
        if ref.shape[0] != m:
            raise ValueError(f"Expected ref_point of {m} entries. Got {ref.shape[0]}.")
    K = max(pf.shape[0] for pf in pareto_fronts)
    # shorter fronts are padded with the reference point itself: not strictly above it, so it gives no box
    Y = ref.to(dev).repeat(len(pareto_fronts), K, 1)
    for p, pf in enumerate(pareto_fronts):
        Y[p, : pf.shape[0]] = weight * pf.detach().to(dev, torch.double)
    bounds, count = dominated_boxes_device(Y, ref.tolist())
    J = max(int(count.max().item()), 1)
    bounds = bounds[:, :, :J]
    if not maximize:
        filled = (torch.arange(J, device=dev)[None, :] < count[:, None])[:, None, :, None]
        bounds = torch.where(filled, -bounds.flip(1), torch.zeros_like(bounds))
    return bounds.contiguous().to(device=pareto_fronts[0].device, dtype=pareto_fronts[0].dtype)


def hypervolume_front_device(Y: Tensor, ref_point: Sequence[float]) -> Tensor:
    """``dkg_hypervolume_front`` on device sets ``Y [S, K, m]`` (fp64) -> ``hv [S]`` on the device."""
    lib = _lib.load()
    if Y.dim() != 3 or Y.dtype is not torch.double or Y.device.type != "cuda":
        raise ValueError("Expected a device fp64 tensor of shape `S x K x m`.")
    S, K, m = Y.shape
    Y = Y.contiguous()
    hv = torch.empty(S, dtype=torch.double, device=Y.device)
    work = workspace(lib.dkg_hypervolume_front_workspace(S, K, m), Y.device)
    with torch.cuda.device(Y.device):
        _lib.check(lib.dkg_hypervolume_front(_lib.ptr(Y), S, K, m, _ref_array(ref_point, m), _lib.ptr(hv),
                                             _lib.ptr(work), work.numel(), current_stream_ptr(Y.device)),
                   "dkg_hypervolume_front")
    return hv


def hypervolume_front(points, ref_point, device=None) -> Tensor:
    """The exact hypervolume dominated by ``points`` above ``ref_point [m]`` (m <= 3, all maximised): one set
    ``[K, m]`` -> a 0-d fp64 tensor, a batch ``[S, K, m]`` -> ``[S]``, on the device.  Points that are not strictly
    above the reference point contribute nothing.  Up to 16384 points per set."""
    P = torch.as_tensor(points)
    if P.dim() not in (2, 3):
        raise ValueError(f"Expected points of shape `K x m` or `S x K x m`. Got {tuple(P.shape)}.")
    ref = torch.as_tensor(ref_point).detach().to("cpu", torch.double).reshape(-1)
    if ref.shape[0] != P.shape[-1]:
        raise ValueError(f"Expected ref_point of {P.shape[-1]} entries. Got {ref.shape[0]}.")
    dev = hip_device(device, "box", P)
    Y = P.detach().to(dev, torch.double)
    if P.shape[-2] == 0:
        return torch.zeros(P.shape[:-2], dtype=torch.double, device=dev)
    hv = hypervolume_front_device(Y if Y.dim() == 3 else Y.unsqueeze(0), ref.tolist())
    return hv if P.dim() == 3 else hv[0]
